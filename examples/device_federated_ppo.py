#!/usr/bin/env python3
"""Federated PPO over four utilities on one GPU: every client trains on its own feeders, a round averages them where they lie.

    python examples/device_federated_ppo.py [--clients 4] [--batch 256] [--steps 32] [--rounds 3] [--clip-norm 0.25] [--noise-std 1e-4] [--prox-mu 0.01]

A utility of the reference (federated/core.py) is a client with its own data.  Here it is an environment handle with its own
`load_powers=` -- `randomized_load_powers` under the client's seed -- and its own `DeviceLearner`.  A round is
{rollout, evaluate, two epochs of `DeviceLearner.step`, `FederatedLearners.round`}: the round measures every client's update against
the global model, clips it to `--clip-norm`, averages by the number of samples, adds Gaussian noise of `--noise-std` and writes the new
global model into every client's master parameters and packed images (`gs_fed_aggregate`).  Adam's moments survive the round, the next
rollout acts with the averaged policy, and there is no torch in the loop and no weight on the host.  `--prox-mu` > 0 is FedProx: after
every round each client is anchored at the global model and its local steps are pulled back by `prox_mu (w - g)`.
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
    ap.add_argument("--clients", type=int, default=4); ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--steps", type=int, default=32); ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--epochs", type=int, default=2); ap.add_argument("--minibatch", type=int, default=2048)
    ap.add_argument("--clip-norm", type=float, default=0.25); ap.add_argument("--noise-std", type=float, default=1e-4)
    ap.add_argument("--lr", type=float, default=3e-4); ap.add_argument("--prox-mu", type=float, default=0.0)
    a = ap.parse_args()
    spec = G.ieee13_like("epsilon")
    D, A = spec.obs_dim, spec.action_dim
    envs = [G.BatchedGridEnvironment(spec, num_envs=a.batch, solver="fbs", stochastic_loads=True, weather_variation=True, episode_length=24,
                                     load_powers=G.randomized_load_powers(spec, a.batch, 0.6, 1.4, seed=10 + k)) for k in range(a.clients)]

    # ONE normalisation for the federation (the library refuses to average networks behind different ones): client 0's statistics
    G.rollout_device(envs[0], 8, seed=0)
    ds = G.DeviceGridDataset(envs[0])
    mean, std = ds.obs_mean, ds.policy_obs_std

    rng = np.random.default_rng(0)
    ws, bs = layers([D, 128, 128, 2 * A], rng)
    bs[-1][A:] = -0.5
    policy = G.MLPPolicy(ws, bs, activation="tanh", obs_mean=mean, obs_std=std, compute="float32")
    value = G.MLPValue(*layers([D, 128, 128, 1], rng), activation="tanh", obs_mean=mean, obs_std=std)
    learners, batches, monitors = [], [], []
    for env in envs:                                                   # every client starts from the same global model
        env.set_policy(policy, stochastic=True)
        env.set_value(value)
        learners.append(G.DeviceLearner(env, nets=("policy", "value"), lr=a.lr, clip=0.2, max_grad_norm=0.5))
        batches.append(G.OnPolicyBatches(env, a.minibatch, policy=policy, adv_norm="minibatch", dtype=np.float32, seed=0))
        monitors.append(G.EpisodeMonitor(env))
    fed = G.FederatedLearners(learners)

    for k, env in enumerate(envs):
        env.reset(seed=1 + k)
        monitors[k].after_reset()
    for r in range(a.rounds):
        returns = []
        for k, env in enumerate(envs):                                 # the clients' local updates: queued, nobody waits
            G.rollout_device(env, a.steps, seed=100 * r + k, reset=False, policy=True)
            returns.append(monitors[k].update().stats.return_mean)
            G.evaluate_rollout(env, gamma=0.99, lam=0.95, bootstrap=("terminated", "truncated"))
            batches[k].prepare()
            for epoch in range(a.epochs):
                for batch in batches[k].epoch(a.epochs * r + epoch):
                    learners[k].step(batch)
        out = fed.round(weights=[a.batch * a.steps] * a.clients, clip_norm=a.clip_norm, noise_std=a.noise_std, seed=7,
                        prox_mu=a.prox_mu if a.prox_mu > 0.0 else None)
        print(f"round {r}: mean episodic return per client " + " ".join(f"{x:+.3f}" for x in returns))
        for net in fed.nets:
            s = out[net]
            print(f"    {net:6s} update norms " + " ".join(f"{x:.4f}" for x in s["norms"]) + "  clip scales " + " ".join(f"{x:.3f}" for x in s["clip_scales"])
                  + f"  Adam step {learners[0].info(net)['step']}")
            if a.prox_mu > 0.0 and r:                                  # (the local steps of this round ran under the last round's anchor)
                print("           proximal penalty per client " + " ".join(f"{l.anchor_stats(net)['penalty_prox']:.3e}" for l in learners))
    final = learners[0].policy()                                       # every client holds the global model now
    print("first-layer weights moved by", float(np.abs(final.weight0 - policy.weight0).max()),
          "| sigma for (epsilon 1, delta 1e-5) at this clip:", G.gaussian_sigma(1.0, 1e-5, a.clip_norm / a.clients))
    fed.close()
    for env in envs:
        env.close()


if __name__ == "__main__":
    main()
