#!/usr/bin/env python3
"""Episode accounting on the device: gs_rollout_episodes without and with costs against the host route it
replaces (download rewards and terminals -- plus costs and margins -- and episodes_np), and the kernels' own times beside gs_k_gae's.
123-bus feeder, sweep solver, B = 8192, T = 64, episode_length = 24, a stochastic float32 policy rollout; every visit a fresh
process with warm-up and its own median of five (the protocol of tools/costs_rate.py).  Recorded, not asserted.
    episodes / episodes_costs   ms per call of gs_rollout_episodes, host clock around the call and a synchronise; a rollout can be
                                accounted once, so every repetition accounts a rollout of its own (collected and, with costs,
                                evaluated by gs_rollout_costs before the clock starts)
    host / host_costs           ms per call of rollout_download(rewards, terminals) [+ rollout_costs_download(costs, margins)] and
                                episodes_np over them, the same rollouts
                                The four legs ALTERNATE for ROUNDS rounds; a leg's figure is the median of its rounds, every round is
                                kept, and `spread` is the largest (max - min) / median over the rounds of one leg
    trace                       rocprofv3 --kernel-trace --stats of a run of its own (five rollouts, each evaluated by a critic,
                                costed and accounted with costs, then five accounted without): the gs_k_ep_* kernels and gs_k_gae,
                                median ns per dispatch, and each one's ratio to gs_k_gae in the same trace
    python tools/episodes_rate.py [B] [--out profiles/episodes_rate.json]     (on the GPU box)
    python tools/episodes_rate.py --child LEG [B]                              one leg in this process"""
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = 64
ROUNDS = 3
EPISODE_LENGTH = 24          # examples/device_lagrangian_ppo.py's: two or three episode ends per instance and rollout
LEGS = ("host", "episodes", "host_costs", "episodes_costs")
KERNELS = ("gs_k_ep_count", "gs_k_ep_offsets", "gs_k_ep_accumulate", "gs_k_ep_accumulate_costs", "gs_k_ep_stats", "gs_k_gae")


def _networks(fs):
    import numpy as np
    rng = np.random.default_rng(1)
    out = []
    for last in (2 * fs.action_dim, 1):
        dims = [fs.obs_dim, 256, 256, last]
        out.append(([rng.normal(0.0, 1.0 / np.sqrt(dims[l]), (dims[l + 1], dims[l])) for l in range(3)],
                    [rng.normal(0.0, 0.1, dims[l + 1]) for l in range(3)]))
    return out


def child(leg, B):
    import time
    import numpy as np
    sys.path.insert(0, ROOT)
    import grid_fed_rl_gym_amd as P
    fs = P.ieee123_like()
    env = P.BatchedGridEnvironment(fs, num_envs=B, solver="fbs", stochastic_loads=True, weather_variation=True, episode_length=EPISODE_LENGTH)
    h = env.handle
    nets = _networks(fs)
    env.set_policy(P.MLPPolicy(*nets[0], activation="relu", compute="float32"), stochastic=True)
    env.reset(seed=np.arange(B, dtype=np.uint64))
    cost_cfg = P._lib.cost_config(P.ConstraintLimits.of(env), "excess")
    with_costs = leg.endswith("_costs")
    state = dict(calls=0, carry=None)

    def collect():
        h.rollout(T, "mlp", seed=7 + state["calls"])
        if with_costs:
            h.rollout_costs(cost_cfg)
        h.synchronize()

    def account():
        start = "fresh" if state["calls"] == 0 else "continue"
        if leg.startswith("episodes"):
            h.rollout_episodes(P._lib.episode_config(start, with_costs))
            h.synchronize()
        else:
            d = h.rollout_download(("rewards", "terminals"))
            c = h.rollout_costs_download(("costs", "margins")) if with_costs else {}
            _, _, state["carry"] = P.episodes_np(d["rewards"], d["terminals"], c.get("costs"), c.get("margins"), carry=state["carry"], start=start)
        state["calls"] += 1

    res = dict(leg=leg, B=B, T=T)
    if leg == "trace_child":
        env.set_value(P.MLPValue(*nets[1], activation="relu"))
        for rep in range(10):
            costs = rep < 5
            h.rollout(T, "mlp", seed=7 + rep)
            if costs:
                h.rollout_evaluate(0.99, 0.95, 3)
                h.rollout_costs(cost_cfg)
            h.rollout_episodes(P._lib.episode_config("fresh", costs))
        h.synchronize()
        res["n_terminal"] = int(h.rollout_device_view().n_terminal)
    elif leg in LEGS:
        for rep in range(2):
            collect(); account()
        ms = []
        for rep in range(5):
            collect()
            t0 = time.perf_counter()
            account()
            ms.append((time.perf_counter() - t0) * 1e3)
        res.update(ms_per_call=sorted(ms)[2], ms_per_call_min=min(ms), ms_per_call_max=max(ms), n_terminal=int(h.rollout_device_view().n_terminal))
    else:
        raise SystemExit(f"unknown leg {leg}")
    print(json.dumps(res), flush=True)
    env.close()


def run(leg, B):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", leg, str(B)], capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        raise SystemExit(f"{leg} failed ({r.returncode}): {r.stderr.strip()[-600:]}")
    line = r.stdout.strip().splitlines()[-1]
    print(line, flush=True)
    return json.loads(line)


def trace(B):
    """the gs_k_ep_* dispatches and gs_k_gae's from a rocprofv3 --kernel-trace --stats run of its own"""
    rocprof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    tmp = tempfile.mkdtemp(prefix="episodes_trace_")
    try:
        r = subprocess.run([rocprof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--", sys.executable, os.path.abspath(__file__),
                            "--child", "trace_child", str(B)], capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            return dict(unavailable=f"rocprofv3 failed ({r.returncode}): {r.stderr.strip()[-300:]}")
        seen = {k: [] for k in KERNELS}
        for f in glob.glob(os.path.join(tmp, "**", "*kernel_trace.csv"), recursive=True):
            for row in csv.DictReader(open(f)):
                name = row["Kernel_Name"].split("(")[0]
                if name in seen:
                    seen[name].append(int(row["End_Timestamp"]) - int(row["Start_Timestamp"]))
        if not seen["gs_k_gae"] or not seen["gs_k_ep_accumulate"]:
            return dict(unavailable="no gs_k_gae / gs_k_ep_accumulate dispatches in kernel_trace.csv")
        med = lambda v: sorted(v)[len(v) // 2]
        gae = med(seen["gs_k_gae"])
        out = dict(n_terminal=json.loads(r.stdout.strip().splitlines()[-1])["n_terminal"],
                   dispatches={k: dict(n=len(v), median_ns=med(v), min_ns=min(v), max_ns=max(v), over_gae=med(v) / gae) for k, v in seen.items() if v})
        d = out["dispatches"]
        out["accounting_us"] = sum(d[k]["median_ns"] for k in ("gs_k_ep_count", "gs_k_ep_offsets", "gs_k_ep_accumulate", "gs_k_ep_stats")) / 1e3
        out["accounting_costs_us"] = sum(d[k]["median_ns"] for k in ("gs_k_ep_count", "gs_k_ep_offsets", "gs_k_ep_accumulate_costs", "gs_k_ep_stats")) / 1e3
        return out
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
    for r in range(ROUNDS):
        for leg in LEGS:
            rounds.setdefault(leg, []).append(run(leg, B))
    mid = lambda v: sorted(v)[len(v) // 2]
    per_round = {leg: [r["ms_per_call"] for r in rs] for leg, rs in rounds.items()}
    ms = {leg: mid(v) for leg, v in per_round.items()}
    summary = dict(B=B, T=T, episode_length=EPISODE_LENGTH, rounds_per_leg=ROUNDS, feeder="ieee123_like", solver="fbs", n_terminal=rounds["episodes"][0]["n_terminal"],
                   ms_per_call=ms, rounds=per_round, spread=max((max(v) - min(v)) / mid(v) for v in per_round.values()),
                   host_over_device=ms["host"] / ms["episodes"], host_over_device_costs=ms["host_costs"] / ms["episodes_costs"], trace=trace(B))
    print(json.dumps(summary), flush=True)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            json.dump(summary, f, indent=1); f.write("\n")


if __name__ == "__main__":
    main()
