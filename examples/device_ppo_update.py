#!/usr/bin/env python3
"""One on-policy update without a host copy: a stochastic rollout on the device, its log-probabilities, values, advantages and
returns computed there, and one clipped-surrogate (PPO) epoch in torch on zero-copy views.

    python examples/device_ppo_update.py [--batch 1024] [--steps 32] [--minibatch 4096]

PyTorch(-ROCm) is the CONSUMER here -- the library itself neither imports nor needs it.  The actor and the critic are torch
modules; `MLPPolicy.from_sequential` / `MLPValue.from_sequential` hand their weights to the device, `gs_rollout` samples the actor
between the steps and records log pi_old(a | s), `evaluate_rollout` runs the critic over the whole collection and the GAE
recurrence.  Minibatch rows come from `DeviceGridDataset.sample_batch(indices=...)` (terminal observations in their place);
the on-policy arrays are [T * B] in the same transition order and are indexed with the same indices.
Advantage normalisation is the learner's business and is done per minibatch below.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import grid_fed_rl_gym_amd as G


def mlp(sizes):
    layers = []
    for i in range(len(sizes) - 1):
        layers.append(torch.nn.Linear(sizes[i], sizes[i + 1]))
        if i < len(sizes) - 2:
            layers.append(torch.nn.ReLU())
    return torch.nn.Sequential(*layers)


def log_prob(actor, obs_n, actions, A):
    """log pi(a | s) of stored actions under the current actor: the device's formula with eps recovered from the action"""
    mean, log_std = torch.chunk(actor(obs_n), 2, dim=-1)
    log_std = torch.clamp(log_std, -20.0, 2.0)
    x = torch.atanh(torch.clamp(actions, -1.0 + 1e-7, 1.0 - 1e-7))
    eps = (x - mean) * torch.exp(-log_std)
    return (-0.5 * eps * eps - log_std - 0.5 * np.log(2.0 * np.pi) - torch.log(1.0 - actions * actions + 1e-6)).sum(dim=-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024); ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--minibatch", type=int, default=4096); ap.add_argument("--clip", type=float, default=0.2)
    a = ap.parse_args()
    spec = G.ieee13_like("epsilon")
    env = G.BatchedGridEnvironment(spec, num_envs=a.batch, solver="fbs", stochastic_loads=True, weather_variation=True, episode_length=24)
    D, A = spec.obs_dim, spec.action_dim
    torch.manual_seed(0)
    actor, critic = mlp([D, 256, 256, 2 * A]), mlp([D, 256, 256, 1])

    # a normalisation to train under: the statistics of a short random rollout, reduced on the device
    G.rollout_device(env, 8, seed=0)
    ds = G.DeviceGridDataset(env)
    mean, std = ds.obs_mean, ds.policy_obs_std

    # the on-policy collection: actor and critic as they are now
    policy = G.MLPPolicy.from_sequential(actor, obs_mean=mean, obs_std=std, compute="float32")
    value = G.MLPValue.from_sequential(critic, obs_mean=mean, obs_std=std)
    G.rollout_device(env, a.steps, seed=1, policy=policy, stochastic=True)
    env.set_value(value)
    stream = torch.cuda.current_stream().cuda_stream
    on = G.evaluate_rollout(env, gamma=0.99, lam=0.95, bootstrap=("terminated", "truncated"), stream=stream)
    N = a.steps * a.batch
    old_logp = torch.as_tensor(on.log_probs, device="cuda").reshape(N)              # zero copy, float64
    adv_all = torch.as_tensor(on.advantages, device="cuda").reshape(N)
    ret_all = torch.as_tensor(on.returns, device="cuda").reshape(N)
    batches = G.DeviceGridDataset(env, normalize=False)                             # raw rows of THIS rollout, terminal observations in place

    actor, critic = actor.cuda(), critic.cuda()
    opt = torch.optim.Adam(list(actor.parameters()) + list(critic.parameters()), lr=3e-4)
    mean_t, inv_std_t = torch.as_tensor(mean, device="cuda"), torch.as_tensor(1.0 / std, device="cuda")
    perm = np.random.default_rng(0).permutation(N)
    for k in range(0, N, a.minibatch):
        idx = perm[k:k + a.minibatch]
        batch = batches.sample_batch(len(idx), indices=idx, stream=stream)
        obs_n = ((torch.as_tensor(batch["observations"], device="cuda") - mean_t) * inv_std_t).float()   # the policy's own normalisation
        actions = torch.as_tensor(batch["actions"], device="cuda").float()
        sel = torch.as_tensor(idx, device="cuda")
        adv, ret, lp_old = adv_all[sel].float(), ret_all[sel].float(), old_logp[sel].float()
        adv = (adv - adv.mean()) / (adv.std() + 1e-8)
        ratio = torch.exp(log_prob(actor, obs_n, actions, A) - lp_old)
        surrogate = torch.minimum(ratio * adv, torch.clamp(ratio, 1.0 - a.clip, 1.0 + a.clip) * adv).mean()
        value_loss = (critic(obs_n).squeeze(-1) - ret).pow(2).mean()
        loss = -surrogate + 0.5 * value_loss
        opt.zero_grad(); loss.backward(); opt.step()
        print(f"minibatch {k // a.minibatch}: ratio {ratio.mean().item():.4f}  surrogate {surrogate.item():+.4f}  value loss {value_loss.item():.4f}")
    env.close()


if __name__ == "__main__":
    main()
