#!/usr/bin/env python3
"""Continual learning on the device: a second task with and without elastic weight consolidation.

    python examples/device_continual_ewc.py [--batch 512] [--steps 32] [--iterations 6] [--ewc-lambda 400] [--min-importance 1e-3]

Task A is the 13-bus feeder under light loading (`randomized_load_powers` in 0.6 .. 0.9 of nominal), task B the same feeder under heavy
loading (1.2 .. 1.5): a new season.  PPO trains on A; `DeviceLearner.consolidate` then takes the per-sample Fisher diagonal of the
policy's and the critic's own losses over one epoch of A's last rollout and keeps it with the parameters as they stand.  Training goes
on under B twice from that same point -- once freely, once with `set_anchor(ewc_lambda=...)`, which adds
`ewc_lambda / 2 sum F (w - w_A)^2` to every step on the device -- and the evaluated return on A is printed before B and after it for
both.  The reference's `ElasticWeightConsolidation` (algorithms/continual_learning.py) squares a whole batch's gradient of a
placeholder loss; here the Fisher is per sample and of the loss the learner trains with.  No torch, no weight on the host.
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
    ap.add_argument("--batch", type=int, default=512); ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--minibatch", type=int, default=2048); ap.add_argument("--epochs", type=int, default=2)
    ap.add_argument("--iterations", type=int, default=6); ap.add_argument("--lr", type=float, default=3e-4)
    ap.add_argument("--ewc-lambda", type=float, default=400.0); ap.add_argument("--min-importance", type=float, default=1e-3)
    a = ap.parse_args()
    spec = G.ieee13_like("epsilon")
    D, A = spec.obs_dim, spec.action_dim
    loads = {"A": G.randomized_load_powers(spec, a.batch, 0.6, 0.9, seed=1), "B": G.randomized_load_powers(spec, a.batch, 1.2, 1.5, seed=2)}
    make = lambda task: G.BatchedGridEnvironment(spec, num_envs=a.batch, solver="fbs", stochastic_loads=True, weather_variation=True,
                                                 episode_length=24, load_powers=loads[task])
    env, eval_a, eval_b = make("A"), make("A"), make("B")

    G.rollout_device(env, 8, seed=0)                                   # one normalisation for both tasks: task A's statistics
    ds = G.DeviceGridDataset(env)
    mean, std = ds.obs_mean, ds.policy_obs_std
    rng = np.random.default_rng(0)
    ws, bs = layers([D, 128, 128, 2 * A], rng)
    bs[-1][A:] = -0.5
    policy = G.MLPPolicy(ws, bs, activation="tanh", obs_mean=mean, obs_std=std, compute="float32")
    value = G.MLPValue(*layers([D, 128, 128, 1], rng), activation="tanh", obs_mean=mean, obs_std=std)
    nets = ("policy", "value")

    def start(policy, value):
        env.set_policy(policy, stochastic=True)
        env.set_value(value)
        learner = G.DeviceLearner(env, nets=nets, lr=a.lr, clip=0.2, max_grad_norm=0.5)
        return learner, G.OnPolicyBatches(env, a.minibatch, policy=policy, adv_norm="minibatch", dtype=np.float32, seed=0)

    def collect(batches, seed):
        G.rollout_device(env, a.steps, seed=seed, reset=False, policy=True)
        G.evaluate_rollout(env, gamma=0.99, lam=0.95, bootstrap=("terminated", "truncated"))
        batches.prepare()

    def train(learner, batches, task, seed0):
        env.set_load_powers(loads[task])
        env.reset(seed=seed0)
        for it in range(a.iterations):
            collect(batches, seed0 + it)
            for epoch in range(a.epochs):
                for batch in batches.epoch(a.epochs * it + epoch):
                    learner.step(batch)

    score = lambda e, p: G.evaluate_policy(e, p, seed=100)["mean_return"]

    learner, batches = start(policy, value)
    print(f"before any training: return on A {score(eval_a, policy):+.3f}, on B {score(eval_b, policy):+.3f}")
    train(learner, batches, "A", 1000)
    policy_a, value_a = learner.policy(), learner.value("value")
    on_a = score(eval_a, policy_a)
    print(f"after task A:        return on A {on_a:+.3f}, on B {score(eval_b, policy_a):+.3f}")

    for lam in (0.0, a.ewc_lambda):
        learner, batches = start(policy_a, value_a)                    # both runs continue from the end of task A
        env.set_load_powers(loads["A"])
        env.reset(seed=2000)
        collect(batches, 2000)                                         # the end of task A: the Fisher diagonal over one epoch of its data
        samples = [learner.consolidate(net, batches.epoch(0), min_importance=a.min_importance) for net in nets]
        if lam > 0.0:
            for net in nets:
                learner.set_anchor(net, ewc_lambda=lam)
        train(learner, batches, "B", 3000)
        after = learner.policy()
        line = f"task B with ewc_lambda {lam:g}: return on A {on_a:+.3f} -> {score(eval_a, after):+.3f}, on B {score(eval_b, after):+.3f}"
        if lam > 0.0:
            s = learner.anchor_stats("policy")
            imp = learner.anchor_arrays("policy", ("ewc_importance",))["ewc_importance"]
            line += (f" | Fisher over {samples[0]} samples, {int((imp > np.float32(a.min_importance)).sum())} of {imp.size} entries above the floor,"
                     f" last penalty {s['penalty_ewc']:.3e}, loss gradient norm {s['grad_norm_loss']:.3f}")
        print(line)
    for e in (env, eval_a, eval_b):
        e.close()


if __name__ == "__main__":
    main()
