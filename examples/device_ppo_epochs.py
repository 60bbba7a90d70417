#!/usr/bin/env python3
"""`device_lagrangian_ppo.py`'s update written on `OnPolicyBatches`: TWO clipped-surrogate epochs over the rollout, every transition
exactly once per epoch, with the shuffle, the gather, the policy's observation normalisation, the Lagrangian advantage
adv - sum_c lambda_c adv_c and its normalisation done by the library where the collection lies; torch sees float32 minibatches.

    python examples/device_ppo_epochs.py [--batch 1024] [--steps 32] [--minibatch 4096] [--epochs 2]

PyTorch(-ROCm) is the CONSUMER here -- the library itself neither imports nor needs it.  `rollout_costs` reads the first
2 n + 2 m + 1 columns of every next observation where the rollout lies (the terminal observation where an episode ended) and leaves
margins, violation counts and costs [3, T, B]; `evaluate_rollout_costs` runs the cost critics `env.set_cost_value` installed over the
collection and the GAE recurrence with the costs as rewards.  The reference's constrained learners (algorithms/safe.py) take these
signals from constraint functions on the host; the dual step is lambda_c <- max(0, lambda_c + lr (mean cost_c - d_c)).

`OnPolicyBatches.prepare()` combines and reduces the advantages once per rollout (`gs_onpolicy_prepare`); `epoch(e)` evaluates the
keyed permutation `permutation_np(seed, e, N)` per position on the device and gathers each minibatch with one kernel
(`gs_onpolicy_batch`): no host permutation, no index upload, no next observations, no float64 fancy indexing in torch.
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
    ap.add_argument("--dual-lr", type=float, default=0.05); ap.add_argument("--epochs", type=int, default=2)
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
    G.evaluate_rollout(env, gamma=0.99, lam=0.95, bootstrap=("terminated", "truncated"), stream=stream)
    # tighter limits than the environment's own, so that there is something to constrain
    limits = G.ConstraintLimits.of(env, voltage=(0.97, 1.03), thermal=0.5)
    sig = G.rollout_costs(env, limits, kinds="excess", stream=stream)
    G.evaluate_rollout_costs(env, gamma=0.99, lam=0.95, bootstrap=("terminated", "truncated"), stream=stream)
    N = a.steps * a.batch
    view = lambda x: torch.as_tensor(x, device="cuda")                                # zero copy
    costs = view(sig.costs).reshape(3, N)
    print("violating transitions (voltage, frequency, thermal):", [int(x) for x in view(sig.n_violating).tolist()], "of", N)

    # the epochs: observations in the policy's normalisation, the Lagrangian advantage normalised per minibatch, everything float32
    batches = G.OnPolicyBatches(env, a.minibatch, policy=policy, lambdas=lam, adv_norm="minibatch", dtype=np.float32, seed=0)
    batches.prepare()
    st = batches.stats
    print(f"combined advantage over {st.n} transitions: mean {st.adv_mean:+.4f}  std {st.adv_std:.4f}; {len(batches)} minibatches an epoch")

    actor, critic = actor.cuda(), critic.cuda()
    cost_critics = {name: net.cuda() for name, net in cost_critics.items()}
    params = list(actor.parameters()) + list(critic.parameters()) + [p for net in cost_critics.values() for p in net.parameters()]
    opt = torch.optim.Adam(params, lr=3e-4)
    for epoch in range(a.epochs):
        for k, batch in enumerate(batches.epoch(epoch, stream=stream)):
            obs_n, actions = view(batch["observations"]), view(batch["actions"])
            lp_old, adv, ret = view(batch["log_probs"]), view(batch["advantages"]), view(batch["returns"])
            ratio = torch.exp(log_prob(actor, obs_n, actions, A) - lp_old)
            surrogate = torch.minimum(ratio * adv, torch.clamp(ratio, 1.0 - a.clip, 1.0 + a.clip) * adv).mean()
            value_loss = (critic(obs_n).squeeze(-1) - ret).pow(2).mean()
            cost_loss = sum((cost_critics[name](obs_n).squeeze(-1) - view(batch["cost_returns"][c])).pow(2).mean() for name, c in CHANNELS.items())
            loss = -surrogate + 0.5 * value_loss + 0.5 * cost_loss
            opt.zero_grad(); loss.backward(); opt.step()
            torch.cuda.current_stream().synchronize()                                  # the next batch reuses the handle's buffers
            print(f"epoch {epoch} minibatch {k}: ratio {ratio.mean().item():.4f}  surrogate {surrogate.item():+.4f}  value loss {value_loss.item():.4f}"
                  f"  cost loss {cost_loss.item():.4f}")
    # the dual step, on the rollout's mean cost per transition
    for name, c in CHANNELS.items():
        mean_cost = costs[c].mean().item()
        lam[name] = max(0.0, lam[name] + a.dual_lr * (mean_cost - budget[name]))
        print(f"{name}: mean cost {mean_cost:.5f}  budget {budget[name]:.5f}  lambda -> {lam[name]:.4f}")
    env.close()


if __name__ == "__main__":
    main()
