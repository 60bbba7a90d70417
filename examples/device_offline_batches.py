#!/usr/bin/env python3
"""An offline learner fed from the GPU: rollout, statistics and minibatches never leave the device.

    python examples/device_offline_batches.py [--batch 1024] [--steps 64] [--updates 20]

The reference's offline learners call `dataset.sample_batch(256)` thousands of times per epoch (algorithms/offline.py:276-279) on a
`GridDataset` that lives in host memory.  Here `gs_rollout` leaves the collection on the GPU, `DeviceGridDataset` reduces its
normalisation statistics there, and every `sample_batch` is one kernel that gathers, puts the terminal observations in place and
normalises into float32 tensors the learner owns.  PyTorch(-ROCm) is the CONSUMER -- the library neither imports nor needs it; the
two sides are ordered on the device (`stream=`).  The only host copies are the statistics (a few kilobytes) and the printed loss.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import grid_fed_rl_gym_amd as G


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024); ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--updates", type=int, default=20); ap.add_argument("--minibatch", type=int, default=256)
    a = ap.parse_args()
    spec = G.ieee123_like()
    env = G.BatchedGridEnvironment(spec, num_envs=a.batch, solver="fbs", stochastic_loads=True, weather_variation=True, episode_length=24)
    G.rollout_device(env, a.steps, seed=0)                       # random actions; the collection stays on the GPU
    ds = G.DeviceGridDataset(env)
    print(f"{ds.size} transitions, {int(ds.constant_columns.sum())} of {spec.obs_dim} observation columns never vary")

    D, A, n = spec.obs_dim, spec.action_dim, a.minibatch
    critic = torch.nn.Sequential(torch.nn.Linear(D + A, 256), torch.nn.ReLU(), torch.nn.Linear(256, 1)).cuda()
    opt = torch.optim.Adam(critic.parameters(), lr=3e-4)
    out = {k: torch.empty(shape, dtype=torch.float32, device="cuda") for k, shape in
           dict(observations=(n, D), actions=(n, A), rewards=(n,), next_observations=(n, D), terminals=(n,)).items()}
    stream = torch.cuda.current_stream().cuda_stream
    for step in range(a.updates):
        b = ds.sample_batch(n, seed=1, dtype=np.float32, out=out, stream=stream)      # one launch; `out` now holds the batch
        obs, act, rew, nxt, term = (out[k] for k in ("observations", "actions", "rewards", "next_observations", "terminals"))
        with torch.no_grad():                                                          # a one-step TD target under the behaviour actions
            target = rew + 0.99 * (1.0 - term) * critic(torch.cat([nxt, act], dim=1)).squeeze(1)
        loss = torch.nn.functional.mse_loss(critic(torch.cat([obs, act], dim=1)).squeeze(1), target)
        opt.zero_grad(); loss.backward(); opt.step()
        # the learner's stream must be done with `out` before the next gather overwrites it
        torch.cuda.current_stream().synchronize()
        if step % 5 == 0 or step == a.updates - 1:
            print(f"update {step}: TD loss {loss.item():.4f}")
    # without `out` the handle lends its own buffers, wrapped without a copy
    b = ds.sample_batch(n, seed=1)
    obs64 = torch.as_tensor(b["observations"], device="cuda")
    print("a float64 batch in the handle's buffer:", tuple(obs64.shape), obs64.dtype, f"|mean| {obs64.mean().abs().item():.3f}")
    # the same normalisation for a device policy (a column that never varies is divided by 1, not by 1e-6)
    actor = torch.nn.Sequential(torch.nn.Linear(D, 64), torch.nn.ReLU(), torch.nn.Linear(64, 2 * A)).double()
    policy = G.MLPPolicy.from_sequential(actor, obs_mean=ds.obs_mean, obs_std=ds.policy_obs_std)
    G.rollout_device(env, a.steps, seed=1, policy=policy)
    ds.rebuild(keep_stats=True)                                 # the new rollout's terminal map, the same normalisation
    print("after a policy rollout:", ds.size, "transitions, reward mean kept at", f"{ds.reward_mean:.4f}")
    env.close()


if __name__ == "__main__":
    main()
