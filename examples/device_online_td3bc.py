#!/usr/bin/env python3
"""Online off-policy RL on the device: the TD3 + BC / SAC-form learner of device_offline_td3bc.py on a REPLAY WINDOW that slides.

    python examples/device_online_td3bc.py [--batch 256] [--steps 16] [--window 64] [--iterations 40] [--minibatches 4] [--alpha 0.0]

Every iteration the CURRENT stochastic policy collects `--steps` new steps behind the last `window - steps` ones
(`ReplayWindow.collect`, `gs_rollout_continue`: the kept steps move to the front on the device); then a few
minibatches over the whole window train the twin critics on the policy-action Bellman target, recomputed per minibatch
(`fresh_targets=True`, section 27), and the actor through the twins (section 23); `update_targets` follows every step.  The window's
first steps are random actions, which also give the networks their normalisation.  No transition, no weight and no sample crosses
the host; the evaluation runs on an environment of its own, so the collecting one is never moved between two collections.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import grid_fed_rl_gym_amd as G


def layers(dims, rng):
    return ([rng.normal(0.0, 1.0 / np.sqrt(dims[l]), (dims[l + 1], dims[l])) for l in range(len(dims) - 1)],
            [np.zeros(dims[l + 1]) for l in range(len(dims) - 1)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256); ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--window", type=int, default=64); ap.add_argument("--iterations", type=int, default=40)
    ap.add_argument("--minibatches", type=int, default=4); ap.add_argument("--minibatch", type=int, default=2048)
    ap.add_argument("--bc-coef", type=float, default=0.0); ap.add_argument("--alpha", type=float, default=0.0)
    ap.add_argument("--lr", type=float, default=1e-3); ap.add_argument("--tau", type=float, default=0.005)
    ap.add_argument("--gamma", type=float, default=0.99)
    a = ap.parse_args()
    spec = G.ieee13_like("epsilon")
    D, A = spec.obs_dim, spec.action_dim
    make = lambda: G.BatchedGridEnvironment(spec, num_envs=a.batch, solver="fbs", stochastic_loads=True, weather_variation=True, episode_length=24)
    env, evaluator = make(), make()

    # the window's first steps: random actions; their statistics are the networks' normalisation
    window = G.ReplayWindow(env, a.window)
    window.collect(a.steps, seed=0)
    ds = G.DeviceGridDataset(env)
    mean, std = ds.obs_mean, ds.policy_obs_std

    rng = np.random.default_rng(0)
    ws, bs = layers([D, 128, 128, 2 * A], rng)
    bs[-1][A:] = -0.5
    policy = G.MLPPolicy(ws, bs, activation="tanh", obs_mean=mean, obs_std=std, compute="float32")
    value = G.MLPValue(*layers([D, 16, 1], rng), activation="tanh", obs_mean=mean, obs_std=std)      # (not trained: the minibatches are prepared over an evaluated rollout)
    twins = [G.MLPQ(*layers([D + A, 128, 128, 1], rng), D, activation="tanh", obs_mean=mean, obs_std=std) for _ in range(2)]
    before = G.evaluate_policy(evaluator, policy, seed=100)["mean_return"]

    bootstrap = ("terminated", "truncated")
    env.set_policy(policy, stochastic=True)       # (installing a network does not move the environment: the window goes on)
    env.set_value(value)
    for w in range(2):
        env.set_q(w, twins[w])
    learner = G.DeviceLearner(env, nets=("q1", "q2", "policy"), lr=a.lr, max_grad_norm=0.5, policy_loss="pathwise", alpha=a.alpha, bc_coef=a.bc_coef,
                              pathwise_stochastic=True, pathwise_seed=7, q_target="policy", fresh_targets=True, gamma=a.gamma, bootstrap=bootstrap,
                              target_seed=11)
    batches = G.OnPolicyBatches(env, a.minibatch, policy=policy, adv_norm="none", dtype=np.float32, seed=0, fields=["observations", "indices"])

    for it in range(a.iterations):
        # the installed policy IS the learner's: the new steps are collected by the network as it stands now
        window.collect(a.steps, seed=1, policy=True)
        info = env.handle.rollout_window_info()
        # the window is a new rollout to every track: evaluate and prepare again, then the targets once (every step refreshes its own rows)
        G.evaluate_rollout(env, gamma=a.gamma, lam=0.95, bootstrap=bootstrap)
        batches.prepare()
        G.evaluate_rollout_q_next(env, gamma=a.gamma, alpha=a.alpha, bootstrap=bootstrap, stochastic=True, seed=11, draw=it)
        for i, batch in enumerate(batches.epoch(it)):
            if i >= a.minibatches:
                break
            learner.step(batch)
            learner.update_targets(a.tau)
        print(f"iteration {it}: window {info['T']} steps ({info['kept']} kept), Q1 loss {learner.stats('q1')['value_loss']:.4f}, "
              f"actor loss {learner.stats('policy')['loss']:+.4f}, min Q at the policy's actions {learner.stats('policy')['surrogate']:+.3f}")

    after = G.evaluate_policy(evaluator, learner.policy(), seed=100)["mean_return"]
    print(f"mean evaluated return {before:+.3f} before, {after:+.3f} after {a.iterations} iterations of {a.steps} new steps on a window of {a.window} "
          f"(alpha {a.alpha}, bc_coef {a.bc_coef}, tau {a.tau}; Adam step {learner.info('policy')['step']})")
    env.close()
    evaluator.close()


if __name__ == "__main__":
    main()
