#!/usr/bin/env python3
"""Constraint costs of a rollout on the device: gs_rollout_costs against a torch assembly of the same work on
the same zero-copy views, the kernel's own time and achieved bytes/s, and gs_rollout_evaluate_costs with three critics beside
gs_rollout_evaluate.  123-bus feeder, sweep solver, B = 8192, T = 64, a stochastic float32 policy rollout; every visit a fresh
process with warm-up and its own median of five (the protocol of tools/onpolicy_rate.py).
    costs / torch_costs      ms per call, device events (on torch's stream, which is made to wait for the handle's) around work that
                             ends in a synchronise.  torch_costs: amin / amax / comparisons over the strided column slices of
                             obs_seq[1:], the terminal rows put in place, the same three outputs [3, T, B].  The two legs ALTERNATE for
                             ROUNDS rounds; a leg's figure is the median of its rounds, every round is kept, and `spread` is the
                             largest (max - min) / median over the rounds of one leg -- what the protocol can resolve
    evaluate / evaluate_costs   gs_rollout_evaluate (one critic) and gs_rollout_evaluate_costs (three critics of the same shape), ms per
                             call, host clock around work that ends in a synchronise
    trace                    rocprofv3 --kernel-trace --stats of a run of its own (one rollout, five gs_rollout_costs): gs_k_costs'
                             two launches (told apart by their order), algorithmic bytes = prefix bytes of (T B + n_terminal) rows plus the outputs, over their time
    python tools/costs_rate.py [B] [--out profiles/costs_rate.json]     (on the GPU box)
    python tools/costs_rate.py --trace-only --out profiles/costs_rate.json   the trace alone, replacing that entry of the file
    python tools/costs_rate.py --child LEG [B]                           one leg in this process"""
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
STREAM_BYTES_PER_S = 6.0e12          # in-order streaming reads, MI355X


def _networks(fs, n_critics):
    import numpy as np
    rng = np.random.default_rng(1)
    out = []
    for last in [2 * fs.action_dim] + [1] * n_critics:
        dims = [fs.obs_dim, 256, 256, last]
        out.append(([rng.normal(0.0, 1.0 / np.sqrt(dims[l]), (dims[l + 1], dims[l])) for l in range(3)],
                    [rng.normal(0.0, 0.1, dims[l + 1]) for l in range(3)]))
    return out


def _torch_costs(torch, a, n, m, lim):
    (vlo, vhi), (flo, fhi), lt = lim.voltage, lim.frequency, lim.thermal
    W = 2 * n + 2 * m

    def parts(x):
        vm, ld, f = x[..., 0:2 * n:2], x[..., 2 * n + 1:W:2].abs(), x[..., W]
        margins = torch.stack([torch.minimum(vm.amin(-1) - vlo, vhi - vm.amax(-1)), torch.minimum(f - flo, fhi - f), lt - ld.amax(-1)])
        counts = torch.stack([((vm < vlo) | (vm > vhi)).sum(-1, dtype=torch.int32), ((f < flo) | (f > fhi)).to(torch.int32),
                              (ld > lt).sum(-1, dtype=torch.int32)])
        return margins, counts

    margins, counts = parts(a["obs_seq"][1:])
    tm, tc = parts(a["terminal_obs"])
    idx = a["terminal_index"].long()
    margins[:, idx[:, 0], idx[:, 1]] = tm
    counts[:, idx[:, 0], idx[:, 1]] = tc
    costs = torch.where(margins < 0, -margins, torch.zeros_like(margins))
    return margins, counts, costs


def child(leg, B):
    import time
    import numpy as np
    sys.path.insert(0, ROOT)
    import torch
    if leg in ("costs", "torch_costs") and not torch.cuda.is_available():
        print(json.dumps(dict(leg=leg, B=B, T=T, unavailable="torch sees no GPU in this process")), flush=True)
        return
    import grid_fed_rl_gym_amd as P
    fs = P.ieee123_like()
    env = P.BatchedGridEnvironment(fs, num_envs=B, solver="fbs", stochastic_loads=True, weather_variation=True)
    h = env.handle
    nets = _networks(fs, 3)
    env.set_policy(P.MLPPolicy(*nets[0], activation="relu", compute="float32"), stochastic=True)
    env.reset(seed=np.arange(B, dtype=np.uint64))
    h.rollout(T, "mlp", seed=7)
    h.synchronize()
    n_term = int(h.rollout_device_view().n_terminal)
    limits = P.ConstraintLimits.of(env)
    cfg = P._lib.cost_config(limits, "excess")
    res = dict(leg=leg, B=B, T=T, n_terminal=n_term)
    if leg in ("costs", "torch_costs"):
        stream = torch.cuda.current_stream().cuda_stream
        if leg == "costs":
            def run():
                h.rollout_costs(cfg)
                h.rollout_costs_view(stream)          # torch's stream waits for the handle's
        else:
            a = {k: torch.as_tensor(v, device="cuda") for k, v in h.rollout_device_arrays().items()}
            def run():
                return _torch_costs(torch, a, fs.n, fs.m, limits)
            # the same numbers as the device's (a sanity check of the leg, not a test)
            h.rollout_costs(cfg)
            dev = h.rollout_costs_arrays()
            tm, tc, tk = run()
            torch.cuda.synchronize()
            res["equal_to_device"] = bool(torch.equal(tm, torch.as_tensor(dev["margins"], device="cuda")) and
                                          torch.equal(tc, torch.as_tensor(dev["counts"], device="cuda")) and
                                          torch.equal(tk, torch.as_tensor(dev["costs"], device="cuda")))
        run(); run(); torch.cuda.synchronize()
        ms = []
        for rep in range(5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run()
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        res.update(ms_per_call=sorted(ms)[2], ms_per_call_min=min(ms), ms_per_call_max=max(ms))
    elif leg in ("evaluate", "evaluate_costs"):
        if leg == "evaluate":
            env.set_value(P.MLPValue(*nets[1], activation="relu"))
            def run():
                h.rollout_evaluate(0.99, 0.95, 3)
                h.synchronize()
        else:
            for c in range(3):
                env.set_cost_value(c, P.MLPValue(*nets[1 + c], activation="relu"))
            h.rollout_costs(cfg)
            def run():
                h.rollout_evaluate_costs(0.99, 0.95, 3)
                h.synchronize()
        run(); run()
        ms = []
        for rep in range(5):
            t0 = time.perf_counter()
            run()
            ms.append((time.perf_counter() - t0) * 1e3)
        res.update(ms_per_call=sorted(ms)[2], ms_per_call_min=min(ms), ms_per_call_max=max(ms), rows=(T + 1) * B)
    elif leg == "trace_child":
        for rep in range(5):
            h.rollout_costs(cfg)
        h.synchronize()
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


def algorithmic_bytes(B, n, m, n_terminal):
    """what gs_rollout_costs must move: the prefix of every row it evaluates plus a skipped flag per ordinary row, and per transition
    and channel a margin, a count and a cost"""
    prefix = (2 * n + 2 * m + 1) * 8
    return (T * B + n_terminal) * prefix + T * B + 3 * T * B * (8 + 4 + 8)


def trace(B, n, m):
    """gs_k_costs' dispatches from a rocprofv3 --kernel-trace --stats run of its own"""
    rocprof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    tmp = tempfile.mkdtemp(prefix="costs_trace_")
    try:
        r = subprocess.run([rocprof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--", sys.executable, os.path.abspath(__file__),
                            "--child", "trace_child", str(B)], capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            return dict(unavailable=f"rocprofv3 failed ({r.returncode}): {r.stderr.strip()[-300:]}")
        n_terminal = json.loads(r.stdout.strip().splitlines()[-1])["n_terminal"]
        seen = []
        for f in glob.glob(os.path.join(tmp, "**", "*kernel_trace.csv"), recursive=True):
            for row in csv.DictReader(open(f)):
                if row["Kernel_Name"].split("(")[0] == "gs_k_costs":
                    seen.append((int(row["Start_Timestamp"]), int(row["End_Timestamp"]) - int(row["Start_Timestamp"])))
        if not seen or len(seen) % 2:
            return dict(unavailable=f"{len(seen)} gs_k_costs dispatches in kernel_trace.csv, expected pairs")
        # gs_rollout_costs launches the kernel twice, in this order (both grids are capped, so the grid size does not tell them apart)
        seen.sort()
        per = {"obs_seq": [d for _, d in seen[0::2]], "terminal_list": [d for _, d in seen[1::2]]}
        med = lambda v: sorted(v)[len(v) // 2]
        out = dict(n_terminal=n_terminal, dispatches={k: dict(n=len(v), median_ns=med(v), min_ns=min(v), max_ns=max(v)) for k, v in per.items()})
        ns = sum(med(v) for v in per.values())
        by = algorithmic_bytes(B, n, m, n_terminal)
        out.update(kernel_us=ns / 1e3, algorithmic_bytes=by, bytes_per_s=by / (ns * 1e-9), share_of_streaming_rate=by / (ns * 1e-9) / STREAM_BYTES_PER_S)
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
    trace_only = "--trace-only" in args
    if trace_only:
        args.remove("--trace-only")
    B = int(args[0]) if args else 8192
    sys.path.insert(0, ROOT)
    import grid_fed_rl_gym_amd as P
    fs = P.ieee123_like()
    if trace_only:          # the profiler's run alone, filed into the summary --out already holds
        summary = json.load(open(out))
        summary["trace"] = trace(B, fs.n, fs.m)
        print(json.dumps(summary["trace"]), flush=True)
        with open(out, "w") as f:
            json.dump(summary, f, indent=1); f.write("\n")
        return
    rounds = {}
    for r in range(ROUNDS):
        for leg in ("torch_costs", "costs"):
            rounds.setdefault(leg, []).append(run(leg, B))
    res = {leg: run(leg, B) for leg in ("evaluate", "evaluate_costs")}
    mid = lambda v: sorted(v)[len(v) // 2]
    ms = {leg: mid([r["ms_per_call"] for r in rs]) for leg, rs in rounds.items()}
    per_round = {leg: [r["ms_per_call"] for r in rs] for leg, rs in rounds.items()}
    spread = max((max(v) - min(v)) / mid(v) for v in per_round.values())
    summary = dict(B=B, T=T, rounds_per_leg=ROUNDS, feeder="ieee123_like", solver="fbs", prefix_columns=2 * fs.n + 2 * fs.m + 1, obs_dim=fs.obs_dim,
                   ms_per_call=ms, rounds=per_round, spread=spread, device_over_torch=ms["costs"] / ms["torch_costs"],
                   device_no_slower_than_torch=bool(ms["costs"] <= ms["torch_costs"] * (1.0 + spread)),
                   torch_equal_to_device=all(r.get("equal_to_device") for r in rounds["torch_costs"]),
                   evaluate=res["evaluate"], evaluate_costs=res["evaluate_costs"],
                   evaluate_costs_over_evaluate=res["evaluate_costs"]["ms_per_call"] / res["evaluate"]["ms_per_call"], trace=trace(B, fs.n, fs.m))
    print(json.dumps(summary), flush=True)
    if out:
        with open(out, "w") as f:
            json.dump(summary, f, indent=1); f.write("\n")


if __name__ == "__main__":
    main()
