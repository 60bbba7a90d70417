#!/usr/bin/env python3
"""A federated round on the device against the only route the library had before it, and the round's kernels'
own times.  The protocol of tools/learner_rate.py: every visit a fresh process with warm-up and its own median of five; the legs
ALTERNATE for ROUNDS rounds, a leg's figure is the median of its rounds, every round is kept.  Set-up: 123-bus feeder, policy
684 -> 256 -> 256 -> 16 plus the reward critic, K = 8 clients of B = 1024.  The bar, stated before measuring: fed <= 1.0 x host.
    fed        ms per round: gs_fed_aggregate for the policy and the reward critic with clip and noise on, host clock from the first
               call to the point where a client's stream has run past the round (a synchronise of client 0)
    host       ms per round of what the library offered before: learner.policy() / .value() on every client (K downloads, unpacked
               on the host), the NumPy mean, set_policy / set_value on every client (packed on the host, uploaded) and a new
               DeviceLearner on every client -- which also loses Adam's moments, as the federation does not
    trace      rocprofv3 --kernel-trace --stats of a run of its own (no counters): the gs_k_fed_* kernels per dispatch
    python tools/fed_rate.py [K] [--out profiles/fed_rate.json]     (on the GPU box)
    python tools/fed_rate.py --child LEG [K]                         one leg in this process"""
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = 1024
ROUNDS = 3
LEGS = ("host", "fed")
HIDDEN = [256, 256]
KERNELS = ("gs_k_fed_gram", "gs_k_fed_sum", "gs_k_fed_apply")


def child(leg, K):
    import time
    import numpy as np
    sys.path.insert(0, ROOT)
    import grid_fed_rl_gym_amd as P
    fs = P.ieee123_like()
    rng = np.random.default_rng(2)
    mean, std = rng.normal(0.0, 1.0, fs.obs_dim), rng.uniform(0.5, 2.0, fs.obs_dim)
    envs, learners = [], []

    def nets_of(k):
        r = np.random.default_rng(10 + k)
        out = []
        for last in (2 * fs.action_dim, 1):
            dims = [fs.obs_dim] + HIDDEN + [last]
            out.append(([r.normal(0.0, 1.0 / np.sqrt(dims[l]), (dims[l + 1], dims[l])) for l in range(3)], [r.normal(0.0, 0.1, dims[l + 1]) for l in range(3)]))
        return out

    hyper = dict(lr=3e-4, clip=0.2)
    for k in range(K):
        env = P.BatchedGridEnvironment(fs, num_envs=B, solver="fbs", stochastic_loads=True, weather_variation=True, episode_length=24)
        pol, val = nets_of(k)
        env.set_policy(P.MLPPolicy(*pol, activation="relu", compute="float32", obs_mean=mean, obs_std=std), stochastic=True)
        env.set_value(P.MLPValue(*val, activation="relu", obs_mean=mean, obs_std=std))
        envs.append(env)
        learners.append(P.DeviceLearner(env, nets=("policy", "value"), **hyper))
    fed = P.FederatedLearners(learners) if leg in ("fed", "trace_child") else None
    part, weights = list(range(K)), [float(B)] * K

    def round_fed(r):
        for net in ("policy", "value"):
            fed.aggregate(net, part, weights, clip_norm=0.5, noise_std=1e-4, seed=3, round=r)
        envs[0].handle.synchronize()

    def round_host(r):
        pols, vals = [l.policy() for l in learners], [l.value("value") for l in learners]
        raw = lambda n: ([n.weight0] + n.weights[1:], [n.bias0] + n.biases[1:]) if isinstance(n, P.MLPPolicy) else (n.weights, n.biases)
        mean_of = lambda nets, i: [np.mean([raw(n)[i][l] for n in nets], axis=0) for l in range(len(raw(nets[0])[i]))]
        pol = P.MLPPolicy(mean_of(pols, 0), mean_of(pols, 1), activation="relu", compute="float32", obs_mean=mean, obs_std=std)
        val = P.MLPValue(mean_of(vals, 0), mean_of(vals, 1), activation="relu", obs_mean=mean, obs_std=std)
        for k, env in enumerate(envs):
            env.set_policy(pol, stochastic=True)
            env.set_value(val)
            learners[k] = P.DeviceLearner(env, nets=("policy", "value"), **hyper)
        envs[0].handle.synchronize()

    res = dict(leg=leg, K=K, B=B, params=[learners[0].info(n)["param_count"] for n in ("policy", "value")])
    if leg == "trace_child":
        for r in range(6):
            round_fed(r)
    elif leg in LEGS:
        run = round_fed if leg == "fed" else round_host
        for r in range(2):
            run(r)
        ms = []
        for r in range(5):
            for env in envs:
                env.handle.synchronize()
            t0 = time.perf_counter()
            run(2 + r)
            ms.append((time.perf_counter() - t0) * 1e3)
        res.update(ms_per_round=sorted(ms)[2], ms_per_round_min=min(ms), ms_per_round_max=max(ms))
    else:
        raise SystemExit(f"unknown leg {leg}")
    print(json.dumps(res), flush=True)
    if fed is not None:
        fed.close()
    for env in envs:
        env.close()


def run(leg, K):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", leg, str(K)], capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        raise SystemExit(f"{leg} failed ({r.returncode}): {r.stderr.strip()[-600:]}")
    line = r.stdout.strip().splitlines()[-1]
    print(line, flush=True)
    return json.loads(line)


def trace(K):
    """the round's kernels' dispatches from a rocprofv3 --kernel-trace --stats run of its own"""
    rocprof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    tmp = tempfile.mkdtemp(prefix="fed_trace_")
    try:
        r = subprocess.run([rocprof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--", sys.executable, os.path.abspath(__file__),
                            "--child", "trace_child", str(K)], capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            return dict(unavailable=f"rocprofv3 failed ({r.returncode}): {r.stderr.strip()[-300:]}")
        seen = {k: [] for k in KERNELS}
        for f in glob.glob(os.path.join(tmp, "**", "*kernel_trace.csv"), recursive=True):
            for row in csv.DictReader(open(f)):
                name = row["Kernel_Name"].split("(")[0]
                if name in seen:
                    seen[name].append(int(row["End_Timestamp"]) - int(row["Start_Timestamp"]))
        if not seen["gs_k_fed_apply"]:
            return dict(unavailable="no gs_k_fed_apply dispatches in kernel_trace.csv")
        med = lambda v: sorted(v)[len(v) // 2]
        # (policy and critic alternate: the policy's dispatches are the slower half of each kernel's)
        return dict(dispatches={k: dict(n=len(v), median_ns=med(v), min_ns=min(v), max_ns=max(v), policy_median_ns=med(sorted(v)[len(v) // 2:]))
                                for k, v in seen.items() if v})
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def main():
    args = sys.argv[1:]
    out = None
    if "--out" in args:
        k = args.index("--out")
        out = args[k + 1]
        del args[k:k + 2]
    if args and args[0] == "--child":
        return child(args[1], int(args[2]) if len(args) > 2 else 8)
    K = int(args[0]) if args else 8
    rounds = {}
    for r in range(ROUNDS):
        for leg in LEGS:
            rounds.setdefault(leg, []).append(run(leg, K))
    mid = lambda v: sorted(v)[len(v) // 2]
    per_round = {leg: [r["ms_per_round"] for r in rs] for leg, rs in rounds.items()}
    ms = {leg: mid(v) for leg, v in per_round.items()}
    summary = dict(K=K, B=B, params=rounds["fed"][0]["params"], rounds_per_leg=ROUNDS, feeder="ieee123_like", hidden=HIDDEN, ms_per_round=ms,
                   rounds=per_round, spread=max((max(v) - min(v)) / mid(v) for v in per_round.values()), fed_over_host=ms["fed"] / ms["host"],
                   trace=trace(K))
    print(json.dumps(summary), flush=True)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            json.dump(summary, f, indent=1); f.write("\n")


if __name__ == "__main__":
    main()
