#!/usr/bin/env python3
"""A sliding window on the device: gs_rollout_continue against the host route it replaces, and gs_rollout itself
on this tree and, with --parent, on a checkout of the parent commit (nothing in that path changes, so the two must agree within the
rounds' own spread).  123-bus feeder, sweep solver, B = 8192, random actions; every visit a fresh process with warm-up and its own
median of five (the protocol of tools/episodes_rate.py).  Recorded, not asserted.
    rollout / rollout_parent    ms per gs_rollout(64) and a synchronise
    continue                    ms per gs_rollout_continue(T = 64, keep = 192) and a synchronise, on a window of 256 steps that has its
                                capacity: the shift of 192 steps in three launches of 64, the terminal list's compaction, 64 steps
    host                        ms for the same window by the host route: download_rollout, the same 64 steps collected by gs_rollout,
                                their download, rollout_window_np, load_rollout_data
                                The legs ALTERNATE for ROUNDS rounds (the two gs_rollout legs taking turns going first); a leg's
                                figure is the median of its rounds, every round is kept, and `spread` is (max - min) / median over
                                the rounds of each leg
    trace                       rocprofv3 --kernel-trace --stats of a run of its own (five continues): the gs_k_window_* dispatches,
                                ns per dispatch and per continue, the shift's bytes (read + written) and its rate against the 6.0 TB/s
                                streaming rate the project measures against
    python tools/window_rate.py [B] [--parent DIR] [--out profiles/window_rate.json]     (on the GPU box)
    python tools/window_rate.py --child LEG [B]                                           one leg in this process"""
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, KEEP = 64, 192
ROUNDS = 3
STREAM_TBS = 6.0
LEGS = ("rollout", "continue", "host")
KERNELS = ("gs_k_window_shift", "gs_k_window_terms", "gs_k_window_term_rows")


def child(leg, B, root):
    import time
    import numpy as np
    sys.path.insert(0, root)
    import grid_fed_rl_gym_amd as P
    fs = P.ieee123_like()
    env = P.BatchedGridEnvironment(fs, num_envs=B, solver="fbs", stochastic_loads=True, weather_variation=True)
    h = env.handle
    env.reset(seed=np.arange(B, dtype=np.uint64))
    res = dict(leg=leg, B=B, T=T, keep=KEEP)

    def timed(call, reps=5, warm=2):
        ms = []
        for rep in range(warm + reps):
            t0 = time.perf_counter()
            call()
            h.synchronize()
            if rep >= warm:
                ms.append((time.perf_counter() - t0) * 1e3)
        return dict(ms_per_call=sorted(ms)[len(ms) // 2], ms_per_call_min=min(ms), ms_per_call_max=max(ms))

    if leg == "rollout":
        res.update(timed(lambda: h.rollout(T, "random", seed=7)))
    elif leg in ("continue", "trace_child"):
        h.rollout(KEEP + T, "random", seed=7)
        h.synchronize()
        res.update(timed(lambda: h.rollout_continue(T, KEEP, "random", seed=7), warm=0 if leg == "trace_child" else 2))
        res.update(window=h.rollout_window_info(), n_terminal=int(h.rollout_device_view().n_terminal))
        res["shift_bytes"] = 2 * 8 * B * ((KEEP + 1) * fs.obs_dim + KEEP * (fs.action_dim + 1)) + 2 * KEEP * B
    elif leg == "host":
        h.rollout(KEEP + T, "random", seed=7)
        h.synchronize()

        def route():
            old = P.download_rollout(env)
            h.rollout(T, "random", seed=7)
            P.load_rollout_data(env, P.rollout_window_np(old, P.download_rollout(env), KEEP))
        res.update(timed(route, reps=3, warm=1))
        res["window_bytes"] = 8 * B * ((KEEP + T) * (2 * fs.obs_dim + fs.action_dim + 1) + fs.obs_dim) + (KEEP + T) * B
    else:
        raise SystemExit(f"unknown leg {leg}")
    print(json.dumps(res), flush=True)
    env.close()


def run(leg, B, root=ROOT):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", leg, str(B), root], capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        raise SystemExit(f"{leg} failed ({r.returncode}): {r.stderr.strip()[-600:]}")
    line = r.stdout.strip().splitlines()[-1]
    print(line, flush=True)
    return json.loads(line)


def trace(B):
    """the gs_k_window_* dispatches of five continues from a rocprofv3 --kernel-trace --stats run of its own"""
    rocprof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    tmp = tempfile.mkdtemp(prefix="window_trace_")
    try:
        r = subprocess.run([rocprof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--", sys.executable, os.path.abspath(__file__),
                            "--child", "trace_child", str(B), ROOT], capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            return dict(unavailable=f"rocprofv3 failed ({r.returncode}): {r.stderr.strip()[-300:]}")
        seen = {k: [] for k in KERNELS}
        for f in glob.glob(os.path.join(tmp, "**", "*kernel_trace.csv"), recursive=True):
            for row in csv.DictReader(open(f)):
                name = row["Kernel_Name"].split("(")[0]
                if name in seen:
                    seen[name].append(int(row["End_Timestamp"]) - int(row["Start_Timestamp"]))
        if not seen["gs_k_window_shift"]:
            return dict(unavailable="no gs_k_window_shift dispatches in kernel_trace.csv")
        res = json.loads(r.stdout.strip().splitlines()[-1])
        calls = 5
        med = lambda v: sorted(v)[len(v) // 2]
        out = dict(continues=calls, dispatches={k: dict(n=len(v), median_ns=med(v), min_ns=min(v), max_ns=max(v), ns_per_continue=sum(v) / calls) for k, v in seen.items() if v})
        shift_s = out["dispatches"]["gs_k_window_shift"]["ns_per_continue"] * 1e-9
        out.update(shift_bytes=res["shift_bytes"], shift_us_per_continue=shift_s * 1e6, shift_tb_per_s=res["shift_bytes"] / shift_s / 1e12,
                   shift_over_streaming=res["shift_bytes"] / shift_s / 1e12 / STREAM_TBS)
        return out
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def main():
    args = sys.argv[1:]
    opts = {}
    for flag in ("--out", "--parent"):
        if flag in args:
            k = args.index(flag)
            opts[flag] = args[k + 1]
            del args[k:k + 2]
    if args and args[0] == "--child":
        return child(args[1], int(args[2]) if len(args) > 2 else 8192, args[3] if len(args) > 3 else ROOT)
    B = int(args[0]) if args else 8192
    legs = [(leg, leg, ROOT) for leg in LEGS]
    if "--parent" in opts:
        legs.insert(0, ("rollout_parent", "rollout", os.path.abspath(opts["--parent"])))
    rounds = {}
    for r in range(ROUNDS):
        order = legs if r % 2 == 0 or "--parent" not in opts else [legs[1], legs[0]] + legs[2:]      # (the two gs_rollout legs take turns going first)
        for name, leg, root in order:
            rounds.setdefault(name, []).append(run(leg, B, root))
    mid = lambda v: sorted(v)[len(v) // 2]
    per_round = {name: [r["ms_per_call"] for r in rs] for name, rs in rounds.items()}
    ms = {name: mid(v) for name, v in per_round.items()}
    summary = dict(B=B, T=T, keep=KEEP, rounds_per_leg=ROUNDS, feeder="ieee123_like", solver="fbs", policy="random", ms_per_call=ms, rounds=per_round,
                   spread={name: (max(v) - min(v)) / mid(v) for name, v in per_round.items()}, window=rounds["continue"][0]["window"],
                   n_terminal=rounds["continue"][0]["n_terminal"], window_bytes=rounds["host"][0]["window_bytes"], host_over_continue=ms["host"] / ms["continue"],
                   continue_minus_rollout_ms=ms["continue"] - ms["rollout"], trace=trace(B))
    if "rollout_parent" in ms:
        summary["rollout_new_over_parent"] = ms["rollout"] / ms["rollout_parent"]
    print(json.dumps(summary), flush=True)
    if "--out" in opts:
        os.makedirs(os.path.dirname(os.path.abspath(opts["--out"])), exist_ok=True)
        with open(opts["--out"], "w") as f:
            json.dump(summary, f, indent=1); f.write("\n")


if __name__ == "__main__":
    main()
