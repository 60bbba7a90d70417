#!/usr/bin/env python3
"""Offline RL on the device: TD3 + BC (or, with `--alpha`, the SAC form) on ONE fixed dataset -- actor and critics of one kind.

    python examples/device_offline_td3bc.py [--batch 256] [--steps 48] [--epochs 8] [--bc-coef 2.5] [--alpha 0.0] [--deterministic]
    python examples/device_offline_td3bc.py --clients 4 [--rounds 4] [--clip-norm 0.5]

The dataset is a random-action rollout.  The twin critics regress on the POLICY-ACTION Bellman target
`r + gamma (min Q_target(s', pi(s')) - alpha log pi(a' | s'))` of `evaluate_rollout_q_next` (the reference's
CQL._update_critic without its conservative penalty), `q_target="policy"`; the actor is the pathwise step
`mean(alpha lp - min(Q1, Q2)(s, pi(s)) + bc_coef |a - a_stored|^2)` (section 23); `update_targets` moves the target networks.  No V
is learnt -- device_offline_pathwise.py borrows IQL's critics instead.  `--alpha` > 0 is the entropy-regularised (SAC) form with a
fixed temperature, `--deterministic` takes a' = tanh(mean) in the target and in the actor.  The targets are those of the last
evaluation: they are re-evaluated between epochs, with a fresh draw of the noise, where the reference resamples per minibatch.
No torch in the loop, no weight and no sample on the host.

With `--clients K` every client has its own `load_powers=` (its own dataset) and one `FederatedLearners.round` over the policy and
the twins follows each client's local epochs; the target networks stay local.
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
    ap.add_argument("--bc-coef", type=float, default=2.5); ap.add_argument("--alpha", type=float, default=0.0)
    ap.add_argument("--deterministic", action="store_true")
    ap.add_argument("--lr", type=float, default=1e-3); ap.add_argument("--tau", type=float, default=0.005)
    ap.add_argument("--gamma", type=float, default=0.99); ap.add_argument("--clip-norm", type=float, default=0.5)
    ap.add_argument("--fresh-targets", action="store_true", help="recompute the Bellman target per minibatch, as the reference's update(batch) does")
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
    value = G.MLPValue(*layers([D, 16, 1], rng), activation="tanh", obs_mean=mean, obs_std=std)      # (not trained: see below)
    twins = [G.MLPQ(*layers([D + A, 128, 128, 1], rng), D, activation="tanh", obs_mean=mean, obs_std=std) for _ in range(2)]
    before = [G.evaluate_policy(e, policy, seed=100 + k)["mean_return"] for k, e in enumerate(evals)]

    nets = ("q1", "q2", "policy")
    bootstrap = ("terminated", "truncated")
    learners, batches = [], []
    for env in envs:                                                   # installed but not acting: the dataset is already there
        env.set_policy(policy, stochastic=True)
        for w in range(2):
            env.set_q(w, twins[w])
        learners.append(G.DeviceLearner(env, nets=nets, lr=a.lr, max_grad_norm=0.5, policy_loss="pathwise", alpha=a.alpha, bc_coef=a.bc_coef,
                                        pathwise_stochastic=not a.deterministic, pathwise_seed=7, q_target="policy",
                                        fresh_targets=a.fresh_targets, gamma=a.gamma, bootstrap=bootstrap, target_seed=11))
        batches.append(G.OnPolicyBatches(env, a.minibatch, policy=policy, adv_norm="none", dtype=np.float32, seed=0, fields=["observations", "indices"]))
        # (the minibatches are prepared over an evaluated rollout; neither field asked for here depends on that evaluation, and no
        # learner reads V)
        env.set_value(value)
        G.evaluate_rollout(env, gamma=a.gamma, lam=0.95, bootstrap=bootstrap)
        batches[-1].prepare()
    fed = G.FederatedLearners(learners) if K > 1 else None

    rounds = a.rounds if K > 1 else 1
    for r in range(rounds):
        for k, env in enumerate(envs):
            for epoch in range(a.epochs):
                e = a.epochs * r + epoch
                # pi(s'), the target twins on it and the Bellman target as the networks stand now, on the SAME rollout
                # (--fresh-targets: once, before the first epoch; every step then refreshes its own minibatch's rows: section 27)
                if not a.fresh_targets or e == 0:
                    G.evaluate_rollout_q_next(env, gamma=a.gamma, alpha=a.alpha, bootstrap=bootstrap, stochastic=not a.deterministic, seed=11, draw=e)
                for batch in batches[k].epoch(e):
                    learners[k].step(batch)                            # Q1, Q2 on the target; the pathwise actor through the twins
                    learners[k].update_targets(a.tau)
        line = " | ".join(f"client {k}: Q1 loss {l.stats('q1')['value_loss']:.4f}, Q2 loss {l.stats('q2')['value_loss']:.4f}, "
                          f"actor loss {l.stats('policy')['loss']:+.4f}, min Q at the policy's actions {l.stats('policy')['surrogate']:+.3f}"
                          for k, l in enumerate(learners))
        if fed is not None:
            out = fed.round(weights=[a.batch * a.steps] * K, clip_norm=a.clip_norm)
            line += " | update norms (q1) " + " ".join(f"{x:.3f}" for x in out["q1"]["norms"])
        print(f"round {r}: {line}")

    for k, (e, l) in enumerate(zip(evals, learners)):
        after = G.evaluate_policy(e, l.policy(), seed=100 + k)["mean_return"]
        print(f"client {k}: mean evaluated return {before[k]:+.3f} before, {after:+.3f} after {rounds * a.epochs} epochs on {a.batch * a.steps} stored transitions"
              f" (policy-action targets, pathwise actor: bc_coef {a.bc_coef}, alpha {a.alpha}, tau {a.tau}; Adam step {l.info('policy')['step']})")
    if fed is not None:
        fed.close()
    for env in envs + evals:
        env.close()


if __name__ == "__main__":
    main()
