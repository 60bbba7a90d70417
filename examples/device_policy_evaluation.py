#!/usr/bin/env python3
"""Evaluate a torch actor per EPISODE without a host copy of the rollout, and take the Lagrangian dual step on the mean EPISODIC cost.

    python examples/device_policy_evaluation.py [--batch 1024] [--steps 32] [--rollouts 6] [--episodes 2]

PyTorch(-ROCm) is the CONSUMER here -- the library itself neither imports nor needs it.  `evaluate_policy` is the reference's
`BenchmarkSuite._run_evaluation` (benchmarking/benchmark_suite.py:360-429), batched: reset, rollouts under the deterministic policy,
and after each rollout `rollout_costs` and `rollout_episodes`, which keep every instance's running return, length and costs on the
device, so an episode of 24 steps that straddles two rollouts of 32 is one episode.  `EpisodeMonitor` does the same bookkeeping for a
training loop: `device_lagrangian_ppo.py` takes its dual step on the mean cost per TRANSITION; the constrained formulation limits
the expected cost per EPISODE, lambda_c <- max(0, lambda_c + lr (mean episodic cost_c - d_c)), which is what is done here.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import grid_fed_rl_gym_amd as G
from device_ppo_update import mlp

CHANNELS = {"voltage": 0, "thermal": 2}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024); ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--rollouts", type=int, default=6); ap.add_argument("--episodes", type=int, default=2)
    ap.add_argument("--dual-lr", type=float, default=0.05)
    a = ap.parse_args()
    spec = G.ieee13_like("epsilon")
    env = G.BatchedGridEnvironment(spec, num_envs=a.batch, solver="fbs", stochastic_loads=True, weather_variation=True, episode_length=24)
    D, A = spec.obs_dim, spec.action_dim
    torch.manual_seed(0)
    actor = mlp([D, 256, 256, 2 * A])
    # a normalisation to act under: the statistics of a short random rollout, reduced on the device
    G.rollout_device(env, 8, seed=0)
    ds = G.DeviceGridDataset(env)
    policy = G.MLPPolicy.from_sequential(actor, obs_mean=ds.obs_mean, obs_std=ds.policy_obs_std, compute="float32")
    # tighter limits than the environment's own, so that there is something to constrain
    limits = G.ConstraintLimits.of(env, voltage=(0.97, 1.03), thermal=0.5)

    # 1. the evaluation: `--episodes` episodes of every instance under the deterministic policy
    ev = G.evaluate_policy(env, policy, episodes_per_instance=a.episodes, deterministic=True, seed=100, limits=limits, kinds="excess",
                           rollout_steps=a.steps)
    print(f"evaluation: {ev['episodes']} episodes in {ev['steps']} steps per instance: return {ev['mean_return']:.3f} +- {ev['std_return']:.3f}, "
          f"{ev['safety_violations']} violating steps, success rate {ev['success_rate']:.3f}, "
          f"mean episodic cost (voltage, frequency, thermal) {[round(float(x), 5) for x in ev['mean_cost']]}")

    # 2. a training loop's view: stochastic rollouts that continue where the last one stopped, a monitor across them
    budget = {"voltage": 0.02, "thermal": 0.2}          # d_c: the episodic excess allowed
    lam = {name: 1.0 for name in CHANNELS}
    monitor = G.EpisodeMonitor(env, window=100)
    env.reset(seed=1)
    monitor.after_reset()
    env.set_policy(policy, stochastic=True)
    for r in range(a.rollouts):
        G.rollout_device(env, a.steps, seed=1 + r, reset=False, policy=True)
        G.rollout_costs(env, limits, kinds="excess")
        rec = monitor.update(costs=True)
        # the records stay on the device for a learner: e.g. the returns of the episodes this rollout finished
        returns = torch.as_tensor(rec.episode_return, device="cuda") if rec.n_episodes else torch.empty(0, device="cuda")
        print(f"rollout {r}: {rec.n_episodes} episodes finished (max return {returns.max().item() if len(returns) else float('nan'):.3f}); "
              f"so far {monitor.count} episodes, return {monitor.mean_return:.3f} +- {monitor.std_return:.3f}, length {monitor.mean_length:.2f}, "
              f"success rate {monitor.success_rate:.3f}")
        # the dual step, on the mean cost per episode of the episodes finished so far
        if monitor.count:
            for name, c in CHANNELS.items():
                mean_cost = float(monitor.mean_cost[c])
                lam[name] = max(0.0, lam[name] + a.dual_lr * (mean_cost - budget[name]))
                print(f"  {name}: mean episodic cost {mean_cost:.5f}  budget {budget[name]:.5f}  lambda -> {lam[name]:.4f}")
    env.close()


if __name__ == "__main__":
    main()
