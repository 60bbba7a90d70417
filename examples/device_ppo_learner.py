#!/usr/bin/env python3
"""Several full on-policy iterations with nothing but the library in the loop: rollout -> evaluate -> minibatch epochs -> learner.

    python examples/device_ppo_learner.py [--batch 1024] [--steps 32] [--minibatch 4096] [--epochs 2] [--iterations 5]

`device_ppo_epochs.py` hands every minibatch to torch for the actor's and the critic's forward pass, the clipped surrogate, two
backward passes and Adam, and brings the weights back through the host before the next rollout.  Here `DeviceLearner.step(batch)`
does that where the networks lie (`gs_learner_step`: forward with saved activations, loss, backward pass on the matrix cores, a
deterministic gradient reduction, Adam), and Adam rewrites the image the rollout and critic kernels read: the next
`rollout_device(policy=True)` acts with the updated policy.  No torch, and no weight ever crosses the host; `learner.policy()`
rebuilds an `MLPPolicy` from the device's parameters when a checkpoint is wanted.

The policy reads the rollout's float64 actions and log-probabilities through the minibatch's indices, not the float32 copies in the
batch: a saturated action rounded to float32 loses 1 - a^2, and with it the importance ratio.
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
    ap.add_argument("--batch", type=int, default=1024); ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--minibatch", type=int, default=4096); ap.add_argument("--epochs", type=int, default=2)
    ap.add_argument("--iterations", type=int, default=5); ap.add_argument("--lr", type=float, default=3e-4)
    a = ap.parse_args()
    spec = G.ieee13_like("epsilon")
    env = G.BatchedGridEnvironment(spec, num_envs=a.batch, solver="fbs", stochastic_loads=True, weather_variation=True, episode_length=24)
    D, A = spec.obs_dim, spec.action_dim
    rng = np.random.default_rng(0)

    # a normalisation to train under: the statistics of a short random rollout, reduced on the device
    G.rollout_device(env, 8, seed=0)
    ds = G.DeviceGridDataset(env)
    mean, std = ds.obs_mean, ds.policy_obs_std

    ws, bs = layers([D, 256, 256, 2 * A], rng)
    bs[-1][A:] = -0.5                                                  # an initial standard deviation of exp(-0.5)
    policy = G.MLPPolicy(ws, bs, activation="tanh", obs_mean=mean, obs_std=std, compute="float32")
    env.set_policy(policy, stochastic=True)
    env.set_value(G.MLPValue(*layers([D, 256, 256, 1], rng), activation="tanh", obs_mean=mean, obs_std=std))
    learner = G.DeviceLearner(env, nets=("policy", "value"), lr=a.lr, clip=0.2, ent_coef=0.0, max_grad_norm=0.5)
    batches = G.OnPolicyBatches(env, a.minibatch, policy=policy, adv_norm="minibatch", dtype=np.float32, seed=0)
    monitor = G.EpisodeMonitor(env)

    env.reset(seed=1)
    monitor.after_reset()
    for it in range(a.iterations):
        G.rollout_device(env, a.steps, seed=100 + it, reset=False, policy=True)       # the policy as the learner left it
        ep = monitor.update().stats
        G.evaluate_rollout(env, gamma=0.99, lam=0.95, bootstrap=("terminated", "truncated"))
        batches.prepare()
        for epoch in range(a.epochs):
            for batch in batches.epoch(a.epochs * it + epoch):
                learner.step(batch)
        p, v = learner.stats("policy"), learner.stats("value")
        print(f"iteration {it}: mean episodic return {ep.return_mean:+.3f} over {ep.count} episodes (running {monitor.mean_return:+.3f}) | surrogate {p['surrogate']:+.4f}"
              f"  kl {p['approx_kl']:+.5f}  clipped {p['clip_fraction']:.3f}  entropy {p['entropy']:+.3f}  |g| {p['grad_norm']:.3f}"
              f" | value loss {v['value_loss']:.4f}  step {p['step']}")
    final = learner.policy()                                           # a current MLPPolicy, for a checkpoint
    print("first-layer weights moved by", float(np.abs(final.weight0 - policy.weight0).max()))
    env.close()


if __name__ == "__main__":
    main()
