#!/usr/bin/env python3
"""Offline RL on the device: implicit Q-learning (IQL) on ONE fixed random-action dataset.

    python examples/device_offline_iql.py [--batch 256] [--steps 48] [--epochs 8] [--temperature 3.0] [--expectile 0.7] [--tau 0.005]
    python examples/device_offline_iql.py --clients 4 [--rounds 4] [--clip-norm 0.5]

The set-up of device_offline_awr.py -- one `rollout_device(env, steps)` with uniform random actions as the dataset an offline client
holds, a second environment to evaluate on -- with the learner the reference's federated offline clients run by default
(algorithms/offline.py IQL.update, lines 454-545): twin Q networks over concat(observation, action) with target networks, a value
network, a Gaussian policy.  Per epoch `evaluate_rollout` gives V on the rollout and `evaluate_rollout_q` the twins' values under
the online and the target images, `q_adv = min(Q1, Q2) - V` and the one-step TD target `r + gamma V(s')`; per minibatch
`DeviceLearner.step` fits V by expectile regression on the target networks' min(Q1, Q2), each Q by mean squared error on the TD
target and the policy by the advantage-weighted log-likelihood of the STORED actions with weights `fmin(exp(q_adv / temperature),
weight_max)`, and `update_targets` moves the target networks.  Q, V and the advantages are those of the epoch's evaluation, not
recomputed inside every minibatch.  No torch in the loop, no weight and no sample on the host.

With `--clients K` every client has its own `load_powers=` (its own dataset) and one `FederatedLearners.round` over all four
networks follows each client's local epochs; the target networks stay local.
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
    ap.add_argument("--clients", type=int, default=1); ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--steps", type=int, default=48); ap.add_argument("--epochs", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=4); ap.add_argument("--minibatch", type=int, default=2048)
    ap.add_argument("--temperature", type=float, default=3.0); ap.add_argument("--weight-max", type=float, default=100.0)
    ap.add_argument("--expectile", type=float, default=0.7); ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--tau", type=float, default=0.005); ap.add_argument("--gamma", type=float, default=0.99)
    ap.add_argument("--fresh-targets", action="store_true", help="recompute Q, V and the targets per minibatch, as the reference's update(batch) does")
    ap.add_argument("--clip-norm", type=float, default=0.5)
    a = ap.parse_args()
    spec = G.ieee13_like("epsilon")
    D, A = spec.obs_dim, spec.action_dim
    K = a.clients
    make = lambda k: G.BatchedGridEnvironment(spec, num_envs=a.batch, solver="fbs", stochastic_loads=True, weather_variation=True, episode_length=24,
                                              load_powers=G.randomized_load_powers(spec, a.batch, 0.6, 1.4, seed=10 + k) if K > 1 else None)
    envs, evals = [make(k) for k in range(K)], [make(k) for k in range(K)]

    # the fixed datasets: one random-action rollout per client; ONE normalisation (client 0's) for every network of the federation
    for k, env in enumerate(envs):
        G.rollout_device(env, a.steps, seed=k)
    ds = G.DeviceGridDataset(envs[0])
    mean, std = ds.obs_mean, ds.policy_obs_std

    rng = np.random.default_rng(0)
    ws, bs = layers([D, 128, 128, 2 * A], rng)
    bs[-1][A:] = -0.5
    policy = G.MLPPolicy(ws, bs, activation="tanh", obs_mean=mean, obs_std=std, compute="float32")
    value = G.MLPValue(*layers([D, 128, 128, 1], rng), activation="tanh", obs_mean=mean, obs_std=std)
    twins = [G.MLPQ(*layers([D + A, 128, 128, 1], rng), D, activation="tanh", obs_mean=mean, obs_std=std) for _ in range(2)]
    before = [G.evaluate_policy(e, policy, seed=100 + k)["mean_return"] for k, e in enumerate(evals)]

    nets = ("value", "q1", "q2", "policy")
    learners, batches = [], []
    for env in envs:                                                   # installed but not acting: the dataset is already there
        env.set_policy(policy, stochastic=True)
        env.set_value(value)
        for w in range(2):
            env.set_q(w, twins[w])
        learners.append(G.DeviceLearner(env, nets=nets, lr=a.lr, max_grad_norm=0.5, policy_loss="awr", temperature=a.temperature,
                                        weight_max=a.weight_max, value_loss="expectile", expectile=a.expectile, advantage_source="q",
                                        value_target="q", fresh_targets=a.fresh_targets, gamma=a.gamma, bootstrap=("terminated", "truncated")))
        batches.append(G.OnPolicyBatches(env, a.minibatch, policy=policy, adv_norm="none", dtype=np.float32, seed=0, fields=["observations", "indices"]))
        G.evaluate_rollout(env, gamma=a.gamma, lam=0.95, bootstrap=("terminated", "truncated"))
        batches[-1].prepare()                                          # (once: observations and indices do not change with the evaluations)
    fed = G.FederatedLearners(learners) if K > 1 else None

    rounds = a.rounds if K > 1 else 1
    bootstrap = ("terminated", "truncated")
    for r in range(rounds):
        for k, env in enumerate(envs):
            for epoch in range(a.epochs):
                # V, the twins under both images, q_adv and the TD target as the networks stand now, on the SAME rollout
                # (--fresh-targets: once, before the first epoch; every step then refreshes its own minibatch's rows: section 27)
                if not a.fresh_targets or (r == 0 and epoch == 0):
                    G.evaluate_rollout(env, gamma=a.gamma, lam=0.95, bootstrap=bootstrap)
                    G.evaluate_rollout_q(env, gamma=a.gamma, bootstrap=bootstrap)
                for batch in batches[k].epoch(a.epochs * r + epoch):
                    learners[k].step(batch)
                    learners[k].update_targets(a.tau)
        line = " | ".join(f"client {k}: V loss {l.stats('value')['value_loss']:.4f}, Q1 loss {l.stats('q1')['value_loss']:.4f}, "
                          f"weighted log-likelihood {l.stats('policy')['surrogate']:+.3f}, capped {l.stats('policy')['clip_fraction']:.3f}"
                          for k, l in enumerate(learners))
        if fed is not None:
            out = fed.round(weights=[a.batch * a.steps] * K, clip_norm=a.clip_norm)
            line += " | update norms (q1) " + " ".join(f"{x:.3f}" for x in out["q1"]["norms"])
        print(f"round {r}: {line}")

    for k, (e, l) in enumerate(zip(evals, learners)):
        after = G.evaluate_policy(e, l.policy(), seed=100 + k)["mean_return"]
        print(f"client {k}: mean evaluated return {before[k]:+.3f} before, {after:+.3f} after {rounds * a.epochs} epochs on {a.batch * a.steps} stored transitions"
              f" (IQL: expectile {a.expectile}, temperature {a.temperature}, tau {a.tau}; Adam step {l.info('policy')['step']})")
    if fed is not None:
        fed.close()
    for env in envs + evals:
        env.close()


if __name__ == "__main__":
    main()
