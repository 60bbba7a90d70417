#!/usr/bin/env python3
"""Per-minibatch targets on the device: what DeviceLearner(fresh_targets=True) costs.  The protocol of
tools/cql_rate.py: 123-bus feeder, sweep solver, B = 8192, T = 64, minibatch 4096 (128 minibatches), float32, nets 692 -> 256 -> 256 -> 1
(Q), 684 -> 256 -> 256 -> 16 (policy); every visit a fresh process, under a time limit of its own, with two warm-up epochs and its own
median of five; the legs ALTERNATE for ROUNDS rounds and every round is kept.
    fresh      (a) the device CQL epoch with fresh_targets=True: per minibatch gs_learner_refresh(TD_POLICY), the conservative steps of Q1
               and Q2, the pathwise actor, update_targets; evaluate_rollout_q_next ran ONCE, before the first epoch
    torch      (b) the torch leg of tools/cql_rate.py, unchanged (run from that file): it recomputes pi(s') and the target twins per
               minibatch, so it does the work of (a)
    epoch      (c) the device leg of tools/cql_rate.py, unchanged: one evaluate_rollout_q_next per epoch
The bar, stated before measuring: (a) <= 1.0 x (b) in EVERY round.  (a) / (c) is recorded without a bar: the per-minibatch passes run
64 workgroups on 256 compute units where the per-epoch pass fills them.
    iql_fresh / iql_epoch    the same for the IQL wiring against the device leg of tools/q_rate.py (its torch leg gathers its regression
               targets from the device's per-epoch arrays, so no torch leg does the work of iql_fresh: (a) / (c) alone)
    trace      rocprofv3 --kernel-trace --stats, a run of its own per wiring (no counters), two fresh epochs each
    python tools/refresh_rate.py [B] [--out profiles/refresh_rate.json]     (on the GPU box)
    python tools/refresh_rate.py --child LEG [B]                             one leg in this process"""
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import cql_rate as CQ      # noqa: E402  (the protocol's constants and the layers' recipe)
import q_rate as IQ        # noqa: E402

T, MINIBATCH, ROUNDS, LEG_SECONDS = CQ.T, CQ.MINIBATCH, CQ.ROUNDS, CQ.LEG_SECONDS
# leg -> (file whose --child runs it, that file's name of the leg)
LEGS = {"fresh": (__file__, "fresh"), "torch": (CQ.__file__, "torch"), "epoch": (CQ.__file__, "device"),
        "iql_fresh": (__file__, "iql_fresh"), "iql_epoch": (IQ.__file__, "device")}
ORDER = (("torch", "fresh", "epoch"), ("iql_epoch", "iql_fresh"))
NEW = ("gs_k_refresh_terms", "gs_k_refresh_rows", "gs_k_refresh_td_policy", "gs_k_refresh_td_value", "gs_k_refresh_combine")
KERNELS = NEW + ("gs_k_policy_rows_f32", "gs_k_value_mlp_f32", "gs_k_q_mlp_f32", "gs_k_q_mlp_rows_f32", "gs_k_q_gather", "gs_k_ds_map_fill", "gs_k_ds_map_scatter")


def child(leg, B):
    import time
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import grid_fed_rl_gym_amd as P
    iql = leg.startswith("iql")
    M = IQ if iql else CQ
    fs = P.ieee123_like()
    D, A = fs.obs_dim, fs.action_dim
    env = P.BatchedGridEnvironment(fs, num_envs=B, solver="fbs", stochastic_loads=True, weather_variation=True, episode_length=M.EPISODE_LENGTH)
    h = env.handle
    rng = np.random.default_rng(1)
    # (the networks, the normalisation and the rollout of the file whose device leg this one is measured against)
    pol_l = M._layers([D] + M.HIDDEN + [2 * A], rng) if iql else M._layers([D] + M.HIDDEN + [2 * A], rng, 0.3)
    val_l = M._layers([D] + M.HIDDEN + [1], rng)
    q_l = [M._layers([D + A] + M.HIDDEN + [1], rng) for _ in range(2)]
    mean, std = rng.normal(0.0, 1.0, D), rng.uniform(0.5, 2.0, D)
    policy = P.MLPPolicy(*pol_l, activation="relu", compute="float32", obs_mean=mean, obs_std=std)
    env.set_policy(policy, stochastic=True)
    env.set_value(P.MLPValue(*val_l, activation="relu", obs_mean=mean, obs_std=std))
    for w in range(2):
        env.set_q(w, P.MLPQ(*q_l[w], D, activation="relu", obs_mean=mean, obs_std=std))
    env.reset(seed=np.arange(B, dtype=np.uint64))
    h.rollout(T, "random", seed=7)
    bootstrap = ("terminated", "truncated") if iql else ()
    P.evaluate_rollout(env, gamma=M.GAMMA, bootstrap=bootstrap)
    batches = P.OnPolicyBatches(env, MINIBATCH, policy=policy, adv_norm="none", dtype=np.float32, fields=["observations", "actions", "indices"])
    batches.prepare()
    fresh = dict(fresh_targets=True, gamma=M.GAMMA, bootstrap=bootstrap, target_seed=11)
    if iql:
        learner = P.DeviceLearner(env, nets=("value", "q1", "q2", "policy"), lr=3e-4, policy_loss="awr", temperature=IQ.TEMPERATURE, weight_max=IQ.WEIGHT_MAX,
                                  value_loss="expectile", expectile=IQ.EXPECTILE, advantage_source="q", value_target="q", **fresh)
        P.evaluate_rollout_q(env, gamma=M.GAMMA, bootstrap=bootstrap)                                   # once, before the first epoch
    else:
        learner = P.DeviceLearner(env, nets=("q1", "q2", "policy"), lr=3e-4, policy_loss="pathwise", alpha=CQ.ALPHA, pathwise_seed=7, q_target="policy",
                                  conservative_weight=CQ.CW, conservative_seed=13, **fresh)
        P.evaluate_rollout_q_next(env, gamma=M.GAMMA, alpha=CQ.ALPHA, bootstrap=bootstrap, seed=11, draw=0)    # once

    def epoch(e):
        for b in batches.epoch(e):
            learner.step(b)
            learner.update_targets(M.TAU)
        h.synchronize()

    res = dict(leg=leg, B=B, T=T, minibatch=MINIBATCH, obs_dim=D, action_dim=A, minibatches=len(batches))
    if leg.endswith("trace_child"):
        for e in range(2):
            epoch(e)
    else:
        for e in range(2):
            epoch(e)
        ms = []
        for e in range(5):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            epoch(2 + e)
            ms.append((time.perf_counter() - t0) * 1e3)
        res.update(ms_per_epoch=sorted(ms)[2], ms_per_epoch_min=min(ms), ms_per_epoch_max=max(ms),
                   stats={net: {k: (None if x != x else x) for k, x in learner.stats(net).items()} for net in learner.nets})
    print(json.dumps(res), flush=True)
    env.close()


def run(leg, B):
    path, name = LEGS[leg]
    r = subprocess.run(["timeout", "-k", "10", str(LEG_SECONDS), sys.executable, os.path.abspath(path), "--child", name, str(B)], capture_output=True, text=True)
    if r.returncode != 0:
        raise SystemExit(f"{leg} failed ({r.returncode}): {r.stderr.strip()[-600:]}")
    line = r.stdout.strip().splitlines()[-1]
    print(f"{leg}: {line}", flush=True)
    return json.loads(line)


def trace(leg, B):
    """the kernels' dispatches from a rocprofv3 --kernel-trace --stats run of its own"""
    rocprof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    tmp = tempfile.mkdtemp(prefix="refresh_trace_")
    try:
        r = subprocess.run(["timeout", "-k", "10", str(LEG_SECONDS), rocprof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--", sys.executable,
                            os.path.abspath(__file__), "--child", leg + "_trace_child", str(B)], capture_output=True, text=True)
        if r.returncode != 0:
            return dict(unavailable=f"rocprofv3 failed ({r.returncode}): {r.stderr.strip()[-300:]}")
        seen = {k: [] for k in KERNELS}
        for f in glob.glob(os.path.join(tmp, "**", "*kernel_trace.csv"), recursive=True):
            for row in csv.DictReader(open(f)):
                name = row["Kernel_Name"].split("(")[0]
                if name in seen:
                    seen[name].append(int(row["End_Timestamp"]) - int(row["Start_Timestamp"]))
        if not seen["gs_k_refresh_rows"]:
            return dict(unavailable="no gs_k_refresh_rows dispatches in kernel_trace.csv")
        med = lambda v: sorted(v)[len(v) // 2]
        return dict(dispatches={k: dict(n=len(v), median_ns=med(v), min_ns=min(v), max_ns=max(v)) for k, v in seen.items() if v},
                    sum_ns={k: sum(v) for k, v in seen.items() if v})
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
        return child(args[1], int(args[2]) if len(args) > 2 else 8192)
    B = int(args[0]) if args else 8192
    rounds = {}
    for group in ORDER:
        for r in range(ROUNDS):
            for leg in group:
                rounds.setdefault(leg, []).append(run(leg, B))
    mid = lambda v: sorted(v)[len(v) // 2]
    per_round = {leg: [r["ms_per_epoch"] for r in rs] for leg, rs in rounds.items()}
    ms = {leg: mid(v) for leg, v in per_round.items()}
    ratio = lambda a, b: [x / y for x, y in zip(per_round[a], per_round[b])]
    summary = dict(B=B, T=T, minibatch=MINIBATCH, minibatches=rounds["fresh"][0]["minibatches"], rounds_per_leg=ROUNDS, feeder="ieee123_like", solver="fbs",
                   dtype="float32", ms_per_epoch=ms, rounds=per_round, bar="fresh <= 1.0 x torch in every round",
                   fresh_over_torch_per_round=ratio("fresh", "torch"), bar_met=all(x <= 1.0 for x in ratio("fresh", "torch")),
                   fresh_over_epoch_per_round=ratio("fresh", "epoch"), iql_fresh_over_epoch_per_round=ratio("iql_fresh", "iql_epoch"),
                   stats=dict(fresh=rounds["fresh"][-1]["stats"], iql_fresh=rounds["iql_fresh"][-1]["stats"]))
    summary["trace"] = dict(fresh=trace("fresh", B), iql_fresh=trace("iql_fresh", B))
    print(json.dumps(summary), flush=True)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            json.dump(summary, f, indent=1); f.write("\n")


if __name__ == "__main__":
    main()
