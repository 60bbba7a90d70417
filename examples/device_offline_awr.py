#!/usr/bin/env python3
"""Offline RL on the device: advantage-weighted regression with an expectile critic on ONE fixed random-action dataset.

    python examples/device_offline_awr.py [--batch 256] [--steps 48] [--epochs 8] [--temperature 1.0] [--expectile 0.7]
    python examples/device_offline_awr.py --clients 4 [--rounds 4] [--clip-norm 0.5] [--prox-mu 0.01]

An offline client of the reference (algorithms/offline.py under federated/core.py's FederatedOfflineRL) holds a dataset some
behaviour policy collected -- `collect_random_data` is the reference's own way to make one -- and never acts while it learns.  Here
the dataset is one `rollout_device(env, steps)` with uniform random actions, which stays on the device: `evaluate_rollout` gives the
critic's values and the returns on it, `OnPolicyBatches` serves it in shuffled minibatches, and `DeviceLearner(policy_loss="awr",
value_loss="expectile")` fits the critic by IQL's expectile regression and the policy by the advantage-weighted log-likelihood of the
STORED actions.  A random rollout records no log-probabilities and the loss needs none.  Between epochs the critic and the advantages
are evaluated again on the same rollout; no new data is collected.  `evaluate_policy` runs the policy before and after on a second
environment with the same feeders, so that the dataset is left alone.

With `--clients K` every client has its own `load_powers=` (its own feeders, hence its own dataset) and one
`FederatedLearners.round` follows each client's local epochs: the reference's FederatedOfflineRL with AWR (`--prox-mu` > 0: with
FedProx's proximal term on the clients' local steps).  No torch in the loop, no weight and no sample on the host.
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
    ap.add_argument("--temperature", type=float, default=1.0); ap.add_argument("--weight-max", type=float, default=20.0)
    ap.add_argument("--expectile", type=float, default=0.7); ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--clip-norm", type=float, default=0.5); ap.add_argument("--prox-mu", type=float, default=0.0)
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
    before = [G.evaluate_policy(e, policy, seed=100 + k)["mean_return"] for k, e in enumerate(evals)]

    learners, batches = [], []
    for env in envs:                                                   # installed but not acting: the dataset is already there
        env.set_policy(policy, stochastic=True)
        env.set_value(value)
        learners.append(G.DeviceLearner(env, nets=("policy", "value"), lr=a.lr, max_grad_norm=0.5, policy_loss="awr", temperature=a.temperature,
                                        weight_max=a.weight_max, value_loss="expectile", expectile=a.expectile))
        batches.append(G.OnPolicyBatches(env, a.minibatch, policy=policy, adv_norm="rollout", dtype=np.float32, seed=0,
                                         fields=["observations", "actions", "advantages", "returns", "values", "indices"]))
    fed = G.FederatedLearners(learners) if K > 1 else None

    rounds = a.rounds if K > 1 else 1
    for r in range(rounds):
        for k, env in enumerate(envs):
            for epoch in range(a.epochs):
                # the critic as it stands now, on the SAME rollout: values, Monte-Carlo-mixed returns and advantages
                G.evaluate_rollout(env, gamma=0.99, lam=0.95, bootstrap=("terminated", "truncated"))
                batches[k].prepare()
                for batch in batches[k].epoch(a.epochs * r + epoch):
                    learners[k].step(batch)
        line = " | ".join(f"client {k}: value loss {l.stats('value')['value_loss']:.4f}, weighted log-likelihood {l.stats('policy')['surrogate']:+.3f}, "
                          f"capped {l.stats('policy')['clip_fraction']:.3f}" for k, l in enumerate(learners))
        if fed is not None:
            out = fed.round(weights=[a.batch * a.steps] * K, clip_norm=a.clip_norm, prox_mu=a.prox_mu if a.prox_mu > 0.0 else None)
            line += " | update norms " + " ".join(f"{x:.3f}" for x in out["policy"]["norms"])
        print(f"round {r}: {line}")

    for k, (e, l) in enumerate(zip(evals, learners)):
        after = G.evaluate_policy(e, l.policy(), seed=100 + k)["mean_return"]
        print(f"client {k}: mean evaluated return {before[k]:+.3f} before, {after:+.3f} after {rounds * a.epochs} epochs on {a.batch * a.steps} stored transitions"
              f" (loss {l.loss('policy')['name']}, Adam step {l.info('policy')['step']})")
    if fed is not None:
        fed.close()
    for env in envs + evals:
        env.close()


if __name__ == "__main__":
    main()
