#!/usr/bin/env python3
"""What the device-resident dataset costs against the routes it replaces.  123-bus feeder, sweep solver,
B = 8192, T = 64 (N = 524 288 transitions, obs_seq[0 .. T-1] = 2.87 GB); every leg in a fresh process of its own that first collects
the same rollout, then times its call five times behind one untimed warm-up (host clock around work that ends in a synchronise):
    build        gs_dataset_build: statistics of observations, actions and rewards and the terminal map
    host         the route before: rollout_download() + GridDataset(...) -- two PCIe copies of the sequence into pageable arrays,
                 np.mean / np.std, two normalised copies (no warm-up: every call allocates its arrays afresh, as a user's does)
    torch_stats  torch.var_mean(obs, dim=0, correction=0) on the zero-copy view of the observations (what a user would write)
    d2d          a device-to-device copy of obs_seq[0 .. T-1]: the bandwidth yardstick (bytes read per second, as many written)
    sample       sample_batch(256), per call, the call returning when the batch is complete
    torch_batch  the same five arrays assembled with torch indexing on the device views, terminal scatter and normalisation
                 included (the map from transition to terminal row built once, outside the timing), one synchronise per call
    python tools/dataset_rate.py [B] [T] [--out profiles/dataset_rate.json]     (on the GPU box; one JSON line per leg)
    python tools/dataset_rate.py --child build [B] [T]                          one leg in this process
Every leg reports the median, the fastest and the slowest of its five timings.  Nothing here is asserted anywhere."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEGS = ("build", "torch_stats", "d2d", "sample", "torch_batch", "host")
BATCH, CALLS = 256, 200


def child(leg, B, T):
    import time
    import numpy as np
    sys.path.insert(0, ROOT)
    torch = None
    if leg.startswith("torch") or leg == "d2d":
        import torch
        if not torch.cuda.is_available():
            print(json.dumps(dict(leg=leg, B=B, T=T, unavailable="torch sees no GPU in this process")), flush=True)
            return
    import grid_fed_rl_gym_amd as P
    fs = P.ieee123_like()
    env = P.BatchedGridEnvironment(fs, num_envs=B, solver="fbs", stochastic_loads=True, weather_variation=True, episode_length=24)
    h = env.handle
    P.rollout_device(env, T, seed=1)
    h.synchronize()
    N, D, A = T * B, h.obs_dim, h.action_dim
    obs_bytes = N * D * 8
    extra = {}
    per = 1
    warm = 1
    if leg == "build":
        def run():
            h.dataset_build(); h.synchronize()
    elif leg == "host":
        warm = 0
        def run():
            d = h.rollout_download()
            flat = {k: d[k].reshape((N,) + d[k].shape[2:]) for k in ("observations", "actions", "rewards", "next_observations")}
            P.GridDataset(flat["observations"], flat["actions"], flat["rewards"], flat["next_observations"], d["terminals"].reshape(N) != 0)
    elif leg == "sample":
        ds = P.DeviceGridDataset(env)
        per = CALLS
        def run():
            for _ in range(CALLS):
                ds.sample_batch(BATCH, seed=3)
    else:
        v = {k: torch.as_tensor(x, device="cuda") for k, x in h.rollout_device_arrays().items() if x.shape[0] > 0}
        obs = v["obs_seq"][:T].reshape(N, D)
        if leg == "torch_stats":
            def run():
                torch.var_mean(obs, dim=0, correction=0); torch.cuda.synchronize()
        elif leg == "d2d":
            dst = torch.empty_like(obs)
            def run():
                dst.copy_(obs); torch.cuda.synchronize()
        else:
            per = CALLS
            seq = v["obs_seq"].reshape((T + 1) * B, D)
            act, rew, flags = v["actions"].reshape(N, A), v["rewards"].reshape(N), v["terminals"].reshape(N)
            tmap = torch.full((N,), -1, dtype=torch.int64, device="cuda")
            if "terminal_index" in v:
                ti = v["terminal_index"].to(torch.int64)
                tmap[ti[:, 0] * B + ti[:, 1]] = torch.arange(ti.shape[0], device="cuda")
            var, mean = torch.var_mean(obs, dim=0, correction=0)
            sd = var.sqrt() + 1e-6
            avar, amean = torch.var_mean(act, dim=0, correction=0)
            asd = avar.sqrt() + 1e-6
            rvar, rmean = torch.var_mean(rew, dim=0, correction=0)
            rsd = rvar.sqrt() + 1e-6
            def run():
                for _ in range(CALLS):
                    idx = torch.randint(0, N, (BATCH,), device="cuda")
                    o = (seq[idx] - mean) / sd
                    nxt = seq[idx + B]
                    k = tmap[idx]
                    m = k >= 0
                    if "terminal_obs" in v:
                        nxt[m] = v["terminal_obs"][k[m]]
                    batch = (o, (act[idx] - amean) / asd, (rew[idx] - rmean) / rsd, (nxt - mean) / sd, ((flags[idx] & 3) != 0).to(torch.float64))
                    torch.cuda.synchronize()
                return batch
    for _ in range(warm):
        run()
    ms = []
    for _ in range(5):
        t0 = time.perf_counter()
        run()
        ms.append((time.perf_counter() - t0) / per * 1e3)
    med = sorted(ms)[2]
    if leg in ("build", "torch_stats", "d2d"):
        extra["obs_bytes_read_per_s"] = obs_bytes / (med * 1e-3)
    print(json.dumps(dict(leg=leg, B=B, T=T, N=N, obs_dim=D, obs_bytes=obs_bytes, ms=med, ms_min=min(ms), ms_max=max(ms),
                          per="call of %d samples" % BATCH if per > 1 else "call", **extra)), flush=True)
    env.close()


def run(leg, B, T):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", leg, str(B), str(T)], capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        raise SystemExit(f"{leg} failed ({r.returncode}): {r.stderr.strip()[-600:]}")
    line = r.stdout.strip().splitlines()[-1]
    print(line, flush=True)
    return json.loads(line)


def main():
    args = sys.argv[1:]
    out = None
    if "--out" in args:
        k = args.index("--out"); out = args[k + 1]; del args[k:k + 2]
    if args and args[0] == "--child":
        return child(args[1], int(args[2]) if len(args) > 2 else 8192, int(args[3]) if len(args) > 3 else 64)
    B = int(args[0]) if args else 8192
    T = int(args[1]) if len(args) > 1 else 64
    res = {leg: run(leg, B, T) for leg in LEGS}
    ms = {leg: r.get("ms") for leg, r in res.items()}
    ratio = lambda a, b: ms[a] / ms[b] if ms.get(a) and ms.get(b) else None
    summary = dict(B=B, T=T, feeder="ieee123_like", solver="fbs", legs=res,
                   torch_stats_over_build=ratio("torch_stats", "build"), host_over_build=ratio("host", "build"),
                   build_share_of_d2d_read_rate=ratio("d2d", "build"), torch_batch_over_sample=ratio("torch_batch", "sample"))
    print(json.dumps(summary), flush=True)
    if out:
        with open(out, "w") as f:
            json.dump(summary, f, indent=1); f.write("\n")


if __name__ == "__main__":
    main()
