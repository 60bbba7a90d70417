#!/usr/bin/env python3
"""What gs_rollout_load costs.  The headline shape: 123-bus feeder, B = 8192, T = 64 (524288 transitions of 684
observation columns: 2.9 GB of observations and as much of next observations in float64).  The dataset is a random-action rollout of the
environment itself, downloaded; it is loaded back
    f64 / f32          from float64 / float32 source arrays
    pageable / pinned  in ordinary NumPy memory / in page-locked memory (gs_host_alloc)
The yardstick, in the same process and the same visit: plain hipMemcpy calls of the same arrays' bytes, from the same host memory, to
a device buffer -- what moving the bytes costs with nothing checked, nothing filed and nothing widened.  Every variant a fresh process
under a time limit of its own, two warm-up loads, the median of five of each; both times and the ratio are recorded.  No bar is set:
nobody has measured this before.
    trace              where the load's time goes when it takes more than 1.5 x the copies: rocprofv3 --kernel-trace --stats, a run of
                       its own (no counters), three loads
    python tools/load_rate.py [B] [--out profiles/load_rate.json]     (on the GPU box)
    python tools/load_rate.py --child VARIANT [B]                      one variant in this process"""
import csv
import ctypes as C
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, REPEATS, WARMUP, LEG_SECONDS = 64, 5, 2, 240
VARIANTS = ("f64_pageable", "f64_pinned", "f32_pageable", "f32_pinned")
KEYS = ("observations", "actions", "rewards", "next_observations", "terminals", "final_observation")
KERNELS = ("gs_k_load_next_f64", "gs_k_load_next_f32", "gs_k_load_widen")


def child(variant, B, loads_only=0):
    import time
    import numpy as np
    sys.path.insert(0, ROOT)
    import grid_fed_rl_gym_amd as P
    from grid_fed_rl_gym_amd import _lib
    dtype, memory = variant.split("_")[:2]
    fs = P.ieee123_like()
    env = P.BatchedGridEnvironment(fs, num_envs=B, solver="fbs", stochastic_loads=True, weather_variation=True, episode_length=24)
    h = env.handle
    P.rollout_device(env, T, seed=1)
    d = h.rollout_download(want=KEYS)
    n_terminal = d.pop("n_terminal")
    if dtype == "f32":
        d = {k: (v.astype(np.float32) if v.dtype == np.float64 else v) for k, v in d.items()}
    lib, hip = _lib.load(), _lib._hip_runtime()
    pinned = []
    if memory == "pinned":
        for k, v in list(d.items()):
            p = C.c_void_p()
            if lib.gs_host_alloc(C.byref(p), max(v.nbytes, 8)) != 0:
                raise SystemExit("gs_host_alloc failed")
            pinned.append(p)
            w = np.frombuffer((C.c_char * v.nbytes).from_address(p.value), dtype=v.dtype, count=v.size).reshape(v.shape)
            w[...] = v
            d[k] = w
    nbytes = sum(v.nbytes for v in d.values())
    hip.hipMalloc.restype = C.c_int
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipFree.argtypes = [C.c_void_p]
    hip.hipDeviceSynchronize.restype = C.c_int
    dst = C.c_void_p()
    if hip.hipMalloc(C.byref(dst), max(v.nbytes for v in d.values())) != 0:
        raise SystemExit("hipMalloc failed")

    def load():
        t0 = time.perf_counter()
        P.load_rollout_data(env, d)          # (synchronises before it returns)
        return time.perf_counter() - t0

    def copies():
        t0 = time.perf_counter()
        for v in d.values():
            if hip.hipMemcpy(dst, C.c_void_p(v.ctypes.data), C.c_size_t(v.nbytes), 1) != 0:      # hipMemcpyHostToDevice
                raise SystemExit("hipMemcpy failed")
        hip.hipDeviceSynchronize()
        return time.perf_counter() - t0

    if loads_only:
        for _ in range(loads_only):
            load()
        out = dict(loads=loads_only)
    else:
        for _ in range(WARMUP):
            load(); copies()
        tl, tc = [], []
        for _ in range(REPEATS):          # alternating: what the host and the link do at that moment is in both
            tl.append(load()); tc.append(copies())
        med = lambda x: float(sorted(x)[len(x) // 2])
        assert h.rollout_device_view().n_terminal == n_terminal
        out = dict(variant=variant, B=B, T=T, obs_dim=env.obs_dim, transitions=B * T, n_terminal=int(n_terminal), bytes=int(nbytes),
                   load_s=med(tl), copies_s=med(tc), ratio=med(tl) / med(tc), load_GBps=nbytes / med(tl) / 1e9, copies_GBps=nbytes / med(tc) / 1e9,
                   load_all_s=tl, copies_all_s=tc)
    hip.hipFree(dst)
    env.close()
    for p in pinned:
        lib.gs_host_free(p)
    print(json.dumps(out), flush=True)


def run(variant, B):
    r = subprocess.run(["timeout", "-k", "10", str(LEG_SECONDS), sys.executable, os.path.abspath(__file__), "--child", variant, str(B)], capture_output=True, text=True)
    if r.returncode != 0:
        raise SystemExit(f"{variant} failed ({r.returncode}): {r.stderr.strip()[-600:]}")
    line = r.stdout.strip().splitlines()[-1]
    print(f"{variant}: {line}", flush=True)
    return json.loads(line)


def trace(variant, B):
    """the load kernels' dispatches from a rocprofv3 --kernel-trace --stats run of its own"""
    rocprof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    tmp = tempfile.mkdtemp(prefix="load_trace_")
    try:
        r = subprocess.run(["timeout", "-k", "10", str(LEG_SECONDS), rocprof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--", sys.executable,
                            os.path.abspath(__file__), "--child", variant + "_trace", str(B)], capture_output=True, text=True)
        if r.returncode != 0:
            return dict(unavailable=f"rocprofv3 failed ({r.returncode}): {r.stderr.strip()[-300:]}")
        seen = {k: [] for k in KERNELS}
        for f in glob.glob(os.path.join(tmp, "**", "*kernel_trace.csv"), recursive=True):
            for row in csv.DictReader(open(f)):
                name = row["Kernel_Name"].split("(")[0]
                if name in seen:
                    seen[name].append(int(row["End_Timestamp"]) - int(row["Start_Timestamp"]))
        return dict(loads=3, kernels={k: dict(dispatches=len(v), total_us=sum(v) / 1e3, median_us=sorted(v)[len(v) // 2] / 1e3) for k, v in seen.items() if v})
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def main():
    args = sys.argv[1:]
    if args and args[0] == "--child":
        variant, B = args[1], int(args[2]) if len(args) > 2 else 8192
        return child(variant, B, loads_only=3 if variant.endswith("_trace") else 0)
    out_path = os.path.join(ROOT, "profiles", "load_rate.json")
    if "--out" in args:
        i = args.index("--out")
        out_path = args[i + 1]
        del args[i:i + 2]
    B = int(args[0]) if args else 8192
    res = dict(protocol="ieee123, fbs, B x T = %d x %d; median of %d after %d warm-ups; load = gs_rollout_load of six arrays, copies = one hipMemcpy per array "
                        "from the same host memory, alternating in one process" % (B, T, REPEATS, WARMUP), variants={})
    for v in VARIANTS:
        res["variants"][v] = run(v, B)
    slow = [v for v in VARIANTS if res["variants"][v]["ratio"] > 1.5]
    if slow:
        res["trace"] = {v: trace(v, B) for v in slow[:2]}
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", out_path)


if __name__ == "__main__":
    main()
