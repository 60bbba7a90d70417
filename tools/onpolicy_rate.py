#!/usr/bin/env python3
"""On-policy rollouts on the device: what recording the log-probabilities costs the rollout, what the value
kernel costs per row next to the policy kernel, and gs_rollout_evaluate against a torch assembly of the same work.
123-bus feeder, B = 8192, T = 64, sweep solver, networks 684 -> 256 -> 256 -> (2 A | 1) with relu, every leg in a fresh process of
its own, median of five (the protocol of tools/policy_rate.py).
    roll_f64 / roll_f32           gs_rollout(T, GS_POLICY_MLP) under the STOCHASTIC policy, log-probabilities recorded
    roll_f64_off / roll_f32_off   the same with gs_rollout_set_log_probs(h, 0)
    parent_f64 / parent_f32       the same rollout on another build of the library (--parent-lib: the parent commit's libgridstep.so)
                                  The three legs of a precision ALTERNATE in one session: parent, off, on, parent, off, on, ... for
                                  ROUNDS rounds, every visit a fresh process with its own median of five; a leg's figure is the median
                                  of its rounds, and every round's figure is kept (`rounds`), so drift over the session shows
    evaluate                      gs_rollout_evaluate after a float32 rollout (two value launches and gs_k_gae), ms per call
    torch_eval                    the same critic as a torch float32 module over the zero-copy obs_seq / terminal_obs views and a torch
                                  GAE loop over T on the views of rewards and flags, ms per call
    trace                         rocprofv3 --kernel-trace --stats of a run of its own (two float32 rollouts, five evaluations):
                                  ns per row of gs_k_value_mlp_f32's launch over obs_seq and of gs_k_policy_mlp_f32, gs_k_gae's time
    python tools/onpolicy_rate.py [B] [--parent-lib PATH] [--out profiles/onpolicy_rate.json]     (on the GPU box)
    python tools/onpolicy_rate.py --child LEG [B] [--parent-lib PATH]                               one leg in this process"""
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


def _networks(fs):
    import numpy as np
    rng = np.random.default_rng(1)
    out = []
    for last in (2 * fs.action_dim, 1):
        dims = [fs.obs_dim, 256, 256, last]
        out.append(([rng.normal(0.0, 1.0 / np.sqrt(dims[l]), (dims[l + 1], dims[l])) for l in range(3)],
                    [rng.normal(0.0, 0.1, dims[l + 1]) for l in range(3)]))
    return out


def child(leg, B, parent_lib):
    import time
    import numpy as np
    sys.path.insert(0, ROOT)
    if leg == "torch_eval":
        import torch
        if not torch.cuda.is_available():
            print(json.dumps(dict(leg=leg, B=B, T=T, unavailable="torch sees no GPU in this process")), flush=True)
            return
    from grid_fed_rl_gym_amd import _lib
    if leg.startswith("parent"):          # another build: bind what it exports
        import ctypes
        other = ctypes.CDLL(parent_lib)
        _lib.LIB_PATH = parent_lib
        _lib.SYMBOLS = [s for s in _lib.SYMBOLS if hasattr(other, s[0])]
    import grid_fed_rl_gym_amd as P
    fs = P.ieee123_like()
    env = P.BatchedGridEnvironment(fs, num_envs=B, solver="fbs", stochastic_loads=True, weather_variation=True)
    h = env.handle
    (pw, pb), (vw, vb) = _networks(fs)
    f32 = not leg.endswith("f64") and not leg.endswith("f64_off")
    env.set_policy(P.MLPPolicy(pw, pb, activation="relu", compute="float32" if f32 else "float64"), stochastic=True)
    env.reset(seed=np.arange(B, dtype=np.uint64))
    res = dict(leg=leg, B=B, T=T)
    if leg.startswith(("roll", "parent")):
        if leg.endswith("_off"):
            h.rollout_log_probs(False)
        def run():
            for _ in range(4):
                h.rollout(T, "mlp", seed=7)
            h.synchronize()
        run(); run()
        us = []
        for rep in range(5):
            t0 = time.perf_counter()
            run()
            us.append((time.perf_counter() - t0) / (4 * T) * 1e6)
        res.update(us_per_step=sorted(us)[2], us_per_step_min=min(us), us_per_step_max=max(us), env_steps_per_s=B / sorted(us)[2] * 1e6)
    elif leg in ("evaluate", "torch_eval", "trace_child"):
        env.set_value(P.MLPValue(vw, vb, activation="relu"))
        h.rollout(T, "mlp", seed=7)
        if leg == "trace_child":
            h.rollout(T, "mlp", seed=8)
        h.synchronize()
        if leg == "torch_eval":
            import torch
            net = torch.nn.Sequential(torch.nn.Linear(fs.obs_dim, 256), torch.nn.ReLU(), torch.nn.Linear(256, 256), torch.nn.ReLU(), torch.nn.Linear(256, 1))
            with torch.no_grad():
                for lin, w, b in zip([m for m in net if hasattr(m, "weight")], vw, vb):
                    lin.weight.copy_(torch.from_numpy(w)); lin.bias.copy_(torch.from_numpy(b))
            net = net.float().cuda()
            a = {k: torch.as_tensor(v, device="cuda") for k, v in h.rollout_device_arrays().items()}
            gamma, lam = 0.99, 0.95
            def run():
                with torch.no_grad():
                    values = net(a["obs_seq"].reshape(-1, fs.obs_dim).float()).double().reshape(T + 1, B)
                    tv = net(a["terminal_obs"].float()).double().reshape(-1)
                    term = torch.zeros(T, B, dtype=torch.float64, device="cuda")
                    idx = a["terminal_index"].long()
                    term[idx[:, 0], idx[:, 1]] = tv
                    done = a["terminals"] != 0
                    adv = torch.empty(T, B, dtype=torch.float64, device="cuda")
                    nxt = torch.zeros(B, dtype=torch.float64, device="cuda")
                    for t in range(T - 1, -1, -1):
                        vnext = torch.where(done[t], term[t], values[t + 1])
                        delta = a["rewards"][t] + gamma * vnext - values[t]
                        nxt = torch.where(done[t], delta, delta + gamma * lam * nxt)
                        adv[t] = nxt
                    ret = adv + values[:T]
                torch.cuda.synchronize()
                return ret
        else:
            def run():
                h.rollout_evaluate(0.99, 0.95, 3)
                h.synchronize()
        run(); run()
        ms = []
        for rep in range(5):
            t0 = time.perf_counter()
            run()
            ms.append((time.perf_counter() - t0) * 1e3)
        res.update(ms_per_call=sorted(ms)[2], ms_per_call_min=min(ms), ms_per_call_max=max(ms), n_terminal=int(h.rollout_device_view().n_terminal),
                   rows=(T + 1) * B)
    else:
        raise SystemExit(f"unknown leg {leg}")
    print(json.dumps(res), flush=True)
    env.close()


def run(leg, B, parent_lib):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", leg, str(B)] + (["--parent-lib", parent_lib] if parent_lib else [])
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        raise SystemExit(f"{leg} failed ({r.returncode}): {r.stderr.strip()[-600:]}")
    line = r.stdout.strip().splitlines()[-1]
    print(line, flush=True)
    return json.loads(line)


def trace(B):
    """ns per dispatch of the three kernels from a rocprofv3 --kernel-trace --stats run of its own"""
    rocprof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    tmp = tempfile.mkdtemp(prefix="onpolicy_trace_")
    try:
        r = subprocess.run([rocprof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--", sys.executable, os.path.abspath(__file__),
                            "--child", "trace_child", str(B)], capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            return dict(unavailable=f"rocprofv3 failed ({r.returncode}): {r.stderr.strip()[-300:]}")
        per = {}
        for f in glob.glob(os.path.join(tmp, "**", "*kernel_trace.csv"), recursive=True):
            for row in csv.DictReader(open(f)):
                name = row["Kernel_Name"].split("(")[0]
                if name in ("gs_k_value_mlp_f32", "gs_k_policy_mlp_f32", "gs_k_gae"):
                    per.setdefault((name, int(row.get("Grid_Size_X") or row.get("Grid_Size") or 0)), []).append(int(row["End_Timestamp"]) - int(row["Start_Timestamp"]))
        if not per:
            return dict(unavailable="no kernel_trace.csv with the three kernels")
        med = lambda v: sorted(v)[len(v) // 2]
        out = dict(dispatches={f"{k[0]}:{k[1]}": dict(n=len(v), median_ns=med(v), min_ns=min(v), max_ns=max(v)) for k, v in sorted(per.items())})
        value = max((k for k in per if k[0] == "gs_k_value_mlp_f32"), key=lambda k: k[1], default=None)      # the launch over obs_seq
        policy = max((k for k in per if k[0] == "gs_k_policy_mlp_f32"), key=lambda k: k[1], default=None)
        if value and policy:
            out["value_ns_per_row"] = med(per[value]) / ((T + 1) * B)
            out["policy_ns_per_row"] = med(per[policy]) / B
            out["value_over_policy_per_row"] = out["value_ns_per_row"] / out["policy_ns_per_row"]
        gae = [v for k, v in per.items() if k[0] == "gs_k_gae"]
        if gae:
            out["gae_us"] = med(gae[0]) / 1e3
        return out
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def main():
    args = sys.argv[1:]
    out = parent_lib = None
    for flag in ("--out", "--parent-lib"):
        if flag in args:
            k = args.index(flag)
            if flag == "--out":
                out = args[k + 1]
            else:
                parent_lib = os.path.abspath(args[k + 1])
            del args[k:k + 2]
    if args and args[0] == "--child":
        return child(args[1], int(args[2]) if len(args) > 2 else 8192, parent_lib)
    B = int(args[0]) if args else 8192
    rounds = {}
    for prec in ("f64", "f32"):
        legs = ([f"parent_{prec}"] if parent_lib else []) + [f"roll_{prec}_off", f"roll_{prec}"]
        for r in range(ROUNDS):
            for leg in legs:
                rounds.setdefault(leg, []).append(run(leg, B, parent_lib))
    res = {leg: run(leg, B, parent_lib) for leg in ("evaluate", "torch_eval")}
    mid = lambda v: sorted(v)[len(v) // 2]
    us = {m: mid([r["us_per_step"] for r in rs]) for m, rs in rounds.items()}
    rate = {m: B / u * 1e6 for m, u in us.items()}
    ratio = lambda a, b: rate[a] / rate[b] if rate.get(a) and rate.get(b) else None
    summary = dict(B=B, T=T, rounds_per_leg=ROUNDS, feeder="ieee123_like", solver="fbs", policy=[684, 256, 256, 16], critic=[684, 256, 256, 1],
                   activation="relu", env_steps_per_s=rate, us_per_step=us,
                   us_per_step_min={m: min(r["us_per_step_min"] for r in rs) for m, rs in rounds.items()},
                   us_per_step_max={m: max(r["us_per_step_max"] for r in rs) for m, rs in rounds.items()},
                   rounds={m: [r["us_per_step"] for r in rs] for m, rs in rounds.items()},
                   f64_off_over_parent=ratio("roll_f64_off", "parent_f64"), f32_off_over_parent=ratio("roll_f32_off", "parent_f32"),
                   f64_logp_over_off=ratio("roll_f64", "roll_f64_off"), f32_logp_over_off=ratio("roll_f32", "roll_f32_off"),
                   evaluate=res["evaluate"], torch_eval=res["torch_eval"], trace=trace(B))
    print(json.dumps(summary), flush=True)
    if out:
        with open(out, "w") as f:
            json.dump(summary, f, indent=1); f.write("\n")


if __name__ == "__main__":
    main()
