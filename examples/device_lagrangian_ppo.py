#!/usr/bin/env python3
"""One Lagrangian PPO update without a host copy: `device_ppo_update.py` plus the constraint signals of the rollout -- per transition
the thermal and the voltage cost, a cost critic for each, their cost advantages -- one clipped-surrogate epoch on
adv - sum_c lambda_c adv_c, and a dual step on the multipliers, all in torch on zero-copy views.

    python examples/device_lagrangian_ppo.py [--batch 1024] [--steps 32] [--minibatch 4096]

PyTorch(-ROCm) is the CONSUMER here -- the library itself neither imports nor needs it.  `rollout_costs` reads the first
2 n + 2 m + 1 columns of every next observation where the rollout lies (the terminal observation where an episode ended) and leaves
margins, violation counts and costs [3, T, B]; `evaluate_rollout_costs` runs the cost critics `env.set_cost_value` installed over the
collection and the GAE recurrence with the costs as rewards.  The reference's constrained learners (algorithms/safe.py) take these
signals from constraint functions on the host; the dual step is lambda_c <- max(0, lambda_c + lr (mean cost_c - d_c)).
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import grid_fed_rl_gym_amd as G
from device_ppo_update import log_prob, mlp

CHANNELS = {"voltage": 0, "thermal": 2}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024); ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--minibatch", type=int, default=4096); ap.add_argument("--clip", type=float, default=0.2)
    ap.add_argument("--dual-lr", type=float, default=0.05)
    a = ap.parse_args()
    spec = G.ieee13_like("epsilon")
    env = G.BatchedGridEnvironment(spec, num_envs=a.batch, solver="fbs", stochastic_loads=True, weather_variation=True, episode_length=24)
    D, A = spec.obs_dim, spec.action_dim
    torch.manual_seed(0)
    actor, critic = mlp([D, 256, 256, 2 * A]), mlp([D, 256, 256, 1])
    cost_critics = {name: mlp([D, 256, 256, 1]) for name in CHANNELS}
    # cost limits d_c per transition (mean excess allowed) and the multipliers
    budget = {"voltage": 1e-3, "thermal": 1e-2}
    lam = {name: 1.0 for name in CHANNELS}

    # a normalisation to train under: the statistics of a short random rollout, reduced on the device
    G.rollout_device(env, 8, seed=0)
    ds = G.DeviceGridDataset(env)
    mean, std = ds.obs_mean, ds.policy_obs_std

    # the on-policy collection: actor and critics as they are now
    policy = G.MLPPolicy.from_sequential(actor, obs_mean=mean, obs_std=std, compute="float32")
    G.rollout_device(env, a.steps, seed=1, policy=policy, stochastic=True)
    env.set_value(G.MLPValue.from_sequential(critic, obs_mean=mean, obs_std=std))
    for name, net in cost_critics.items():
        env.set_cost_value(name, G.MLPValue.from_sequential(net, obs_mean=mean, obs_std=std))
    stream = torch.cuda.current_stream().cuda_stream
    on = G.evaluate_rollout(env, gamma=0.99, lam=0.95, bootstrap=("terminated", "truncated"), stream=stream)
    # tighter limits than the environment's own, so that there is something to constrain
    limits = G.ConstraintLimits.of(env, voltage=(0.97, 1.03), thermal=0.5)
    sig = G.rollout_costs(env, limits, kinds="excess", stream=stream)
    con = G.evaluate_rollout_costs(env, gamma=0.99, lam=0.95, bootstrap=("terminated", "truncated"), stream=stream)
    N = a.steps * a.batch
    view = lambda x: torch.as_tensor(x, device="cuda")                                # zero copy, float64
    old_logp, adv_all, ret_all = view(on.log_probs).reshape(N), view(on.advantages).reshape(N), view(on.returns).reshape(N)
    costs = view(sig.costs).reshape(3, N)
    cadv = {name: view(con.advantages[c]).reshape(N) for name, c in CHANNELS.items()}
    cret = {name: view(con.returns[c]).reshape(N) for name, c in CHANNELS.items()}
    n_viol = view(sig.n_violating)
    print("violating transitions (voltage, frequency, thermal):", [int(x) for x in n_viol.tolist()], "of", N)
    batches = G.DeviceGridDataset(env, normalize=False)                               # raw rows of THIS rollout, terminal observations in place

    actor, critic = actor.cuda(), critic.cuda()
    cost_critics = {name: net.cuda() for name, net in cost_critics.items()}
    params = list(actor.parameters()) + list(critic.parameters()) + [p for net in cost_critics.values() for p in net.parameters()]
    opt = torch.optim.Adam(params, lr=3e-4)
    mean_t, inv_std_t = torch.as_tensor(mean, device="cuda"), torch.as_tensor(1.0 / std, device="cuda")
    perm = np.random.default_rng(0).permutation(N)
    for k in range(0, N, a.minibatch):
        idx = perm[k:k + a.minibatch]
        batch = batches.sample_batch(len(idx), indices=idx, stream=stream)
        obs_n = ((torch.as_tensor(batch["observations"], device="cuda") - mean_t) * inv_std_t).float()   # the policy's own normalisation
        actions = torch.as_tensor(batch["actions"], device="cuda").float()
        sel = torch.as_tensor(idx, device="cuda")
        lp_old = old_logp[sel].float()
        # the Lagrangian's advantage: the reward's minus the multipliers' share of the costs'
        adv = adv_all[sel] - sum(lam[name] * cadv[name][sel] for name in CHANNELS)
        adv = ((adv - adv.mean()) / (adv.std() + 1e-8)).float()
        ratio = torch.exp(log_prob(actor, obs_n, actions, A) - lp_old)
        surrogate = torch.minimum(ratio * adv, torch.clamp(ratio, 1.0 - a.clip, 1.0 + a.clip) * adv).mean()
        value_loss = (critic(obs_n).squeeze(-1) - ret_all[sel].float()).pow(2).mean()
        cost_loss = sum((cost_critics[name](obs_n).squeeze(-1) - cret[name][sel].float()).pow(2).mean() for name in CHANNELS)
        loss = -surrogate + 0.5 * value_loss + 0.5 * cost_loss
        opt.zero_grad(); loss.backward(); opt.step()
        print(f"minibatch {k // a.minibatch}: ratio {ratio.mean().item():.4f}  surrogate {surrogate.item():+.4f}  value loss {value_loss.item():.4f}"
              f"  cost loss {cost_loss.item():.4f}")
    # the dual step, on the rollout's mean cost per transition
    for name, c in CHANNELS.items():
        mean_cost = costs[c].mean().item()
        lam[name] = max(0.0, lam[name] + a.dual_lr * (mean_cost - budget[name]))
        print(f"{name}: mean cost {mean_cost:.5f}  budget {budget[name]:.5f}  lambda -> {lam[name]:.4f}")
    env.close()


if __name__ == "__main__":
    main()
