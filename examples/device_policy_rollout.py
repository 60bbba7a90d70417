#!/usr/bin/env python3
"""On-policy collection at device rate: the policy network is evaluated on the GPU between two env steps of one rollout.

    python examples/device_policy_rollout.py [--batch 8192] [--steps 64] [--compute float64|float32]

`MLPPolicy` carries the actor's weights (here random ones; `MLPPolicy.from_sequential(actor_net, ...)` reads a torch
`nn.Sequential` without importing torch), `collect_policy_data` is `collect_random_data` under that policy: same dictionary, one
download at the end.  `--compute float32` evaluates the layers at the precision of a torch actor (float32 weights and sums on the
f32 matrix instructions, the normalisation as a float64 stage of its own, the head in float64).  Compare examples/device_policy_loop.py, where Python drives every step and torch evaluates the network.
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import grid_fed_rl_gym_amd as G


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8192); ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--compute", choices=("float64", "float32"), default="float64")
    a = ap.parse_args()
    spec = G.ieee123_like()
    env = G.BatchedGridEnvironment(spec, num_envs=a.batch, solver="fbs", stochastic_loads=True, weather_variation=True)
    # observation statistics from a short random rollout (GridDataset's normalisation), folded into the first layer
    ds = G.GridDataset(**G.collect_random_data(env, 8))
    still = ds.obs_std <= 2e-6                       # columns that never change (the static load powers) carry nothing: leave them out
    rng = np.random.default_rng(0)
    dims = [spec.obs_dim, 256, 256, 2 * spec.action_dim]
    ws = [rng.normal(0.0, 1.0 / np.sqrt(dims[l]), (dims[l + 1], dims[l])) for l in range(3)]
    bs = [np.zeros(dims[l + 1]) for l in range(3)]
    ws[0][:, still] = 0.0
    policy = G.MLPPolicy(ws, bs, activation="relu", head="gaussian_tanh", obs_mean=ds.obs_mean, obs_std=np.where(still, 1.0, ds.obs_std),
                         compute=a.compute)
    # evaluation: tanh(mean) on the observation the environment stands at
    env.reset(seed=0)
    env.set_policy(policy)
    print("policy compute path:", env.policy_compute)
    print("first actions of instance 0:", np.round(env.policy_actions()[0], 3))
    # collection: a = tanh(mean + std * eps), eps drawn on the device
    G.rollout_device(env, a.steps, policy=policy, stochastic=True, seed=1)
    env.handle.synchronize()
    t0 = time.perf_counter()
    G.rollout_device(env, a.steps, policy=True, seed=2, reset=False)
    env.handle.synchronize()
    dt = time.perf_counter() - t0
    print(f"{a.batch * a.steps / dt / 1e6:.1f} M env-steps/s under the policy, {dt / a.steps * 1e6:.1f} us per step")
    data = G.collect_policy_data(env, policy, a.steps, stochastic=True, seed=3)
    print({k: v.shape for k, v in data.items()}, "episodes finished:", int(data["terminals"].sum()))
    env.close()


if __name__ == "__main__":
    main()
