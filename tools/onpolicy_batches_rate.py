#!/usr/bin/env python3
"""On-policy minibatch epochs on the device: one epoch of OnPolicyBatches against the route it replaces, and the
gather kernel's own time beside the dataset's.  123-bus feeder, sweep solver, B = 8192, T = 64, minibatch 4096, float32, all fields,
cost critics on voltage and thermal; every visit a fresh process with warm-up and its own median of five (the protocol of
tools/episodes_rate.py).  PyTorch is the consumer of both legs.  The bar: batches <= 1.0 x torch.
    batches    ms per epoch of OnPolicyBatches.epoch with the consumer's stream, every field wrapped as a torch tensor, host clock
               around the epoch and a synchronise
    torch      ms per epoch of the same rollout the former way: a host permutation, DeviceGridDataset.sample_batch(indices=,
               normalize=False), and the torch lines of examples/device_lagrangian_ppo.py (normalisation, fancy indexing of the float64
               views, the Lagrangian combination, the minibatch normalisation), producing the same tensors
               The legs ALTERNATE for ROUNDS rounds; a leg's figure is the median of its rounds, every round is kept, and `spread`
               is the largest (max - min) / median over the rounds of one leg
    trace      rocprofv3 --kernel-trace --stats of a run of its own (no counters): gs_k_opb_gather_f32 and the dataset's
               gs_k_ds_gather_f32 at the same n, median ns per dispatch, bytes moved per dispatch and the rate against 6.0 TB/s
    python tools/onpolicy_batches_rate.py [B] [--out profiles/onpolicy_batches_rate.json]     (on the GPU box)
    python tools/onpolicy_batches_rate.py --child LEG [B]                                      one leg in this process"""
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
MINIBATCH = 4096
ROUNDS = 3
EPISODE_LENGTH = 24
LEGS = ("torch", "batches")
CHANNELS = {"voltage": 0, "thermal": 2}
LAMBDAS = {"voltage": 1.0, "thermal": 1.0}
KERNELS = ("gs_k_opb_gather_f32", "gs_k_ds_gather_f32", "gs_k_opb_index", "gs_k_opb_mbstats")
STREAM_TBS = 6.0


def _networks(fs):
    import numpy as np
    rng = np.random.default_rng(1)
    out = []
    for last in (2 * fs.action_dim, 1, 1, 1):
        dims = [fs.obs_dim, 256, 256, last]
        out.append(([rng.normal(0.0, 1.0 / np.sqrt(dims[l]), (dims[l + 1], dims[l])) for l in range(3)],
                    [rng.normal(0.0, 0.1, dims[l + 1]) for l in range(3)]))
    return out


def child(leg, B):
    import time
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import grid_fed_rl_gym_amd as P
    fs = P.ieee123_like()
    env = P.BatchedGridEnvironment(fs, num_envs=B, solver="fbs", stochastic_loads=True, weather_variation=True, episode_length=EPISODE_LENGTH)
    h = env.handle
    nets = _networks(fs)
    rng = np.random.default_rng(2)
    mean, std = rng.normal(0.0, 1.0, fs.obs_dim), rng.uniform(0.5, 2.0, fs.obs_dim)
    policy = P.MLPPolicy(*nets[0], activation="relu", compute="float32", obs_mean=mean, obs_std=std)
    env.set_policy(policy, stochastic=True)
    env.set_value(P.MLPValue(*nets[1], activation="relu", obs_mean=mean, obs_std=std))
    for k, name in enumerate(CHANNELS):
        env.set_cost_value(name, P.MLPValue(*nets[2 + k], activation="relu", obs_mean=mean, obs_std=std))
    env.reset(seed=np.arange(B, dtype=np.uint64))
    h.rollout(T, "mlp", seed=7)
    stream = torch.cuda.current_stream().cuda_stream
    on = P.evaluate_rollout(env, bootstrap=("terminated", "truncated"), stream=stream)
    P.rollout_costs(env, P.ConstraintLimits.of(env, voltage=(0.97, 1.03), thermal=0.5), stream=stream)
    con = P.evaluate_rollout_costs(env, bootstrap=("terminated", "truncated"), stream=stream)
    N = T * B
    view = lambda x: torch.as_tensor(x, device="cuda")

    batches = P.OnPolicyBatches(env, MINIBATCH, policy=policy, lambdas=LAMBDAS, adv_norm="minibatch", dtype=np.float32)
    batches.prepare()

    def epoch_batches(e):
        last = None
        for b in batches.epoch(e, stream=stream):
            last = {k: ([None if x is None else view(x) for x in v] if isinstance(v, list) else view(v)) for k, v in b.items()}
        torch.cuda.synchronize()
        return last

    old_logp, adv_all, ret_all = view(on.log_probs).reshape(N), view(on.advantages).reshape(N), view(on.returns).reshape(N)
    val_all = view(on.values)[:T].reshape(N)
    cadv = {name: view(con.advantages[c]).reshape(N) for name, c in CHANNELS.items()}
    cret = {name: view(con.returns[c]).reshape(N) for name, c in CHANNELS.items()}
    mean_t, inv_std_t = torch.as_tensor(mean, device="cuda"), torch.as_tensor(1.0 / std, device="cuda")
    ds = P.DeviceGridDataset(env, normalize=False)

    def epoch_torch(e):
        perm = np.random.default_rng(e).permutation(N)
        last = None
        for k in range(0, N, MINIBATCH):
            idx = perm[k:k + MINIBATCH]
            batch = ds.sample_batch(len(idx), indices=idx, stream=stream)
            obs_n = ((view(batch["observations"]) - mean_t) * inv_std_t).float()
            actions = view(batch["actions"]).float()
            sel = torch.as_tensor(idx, device="cuda")
            adv = adv_all[sel] - sum(LAMBDAS[name] * cadv[name][sel] for name in CHANNELS)
            adv = ((adv - adv.mean()) / (adv.std() + 1e-8)).float()
            last = dict(observations=obs_n, actions=actions, log_probs=old_logp[sel].float(), advantages=adv, returns=ret_all[sel].float(),
                        values=val_all[sel].float(), cost_advantages=[cadv[name][sel].float() for name in CHANNELS],
                        cost_returns=[cret[name][sel].float() for name in CHANNELS], indices=sel)
        torch.cuda.synchronize()
        return last

    res = dict(leg=leg, B=B, T=T, minibatch=MINIBATCH, obs_dim=fs.obs_dim)
    if leg == "trace_child":
        for e in range(3):
            epoch_batches(e)
        for k in range(8):
            ds.sample_batch(MINIBATCH, seed=k, dtype=np.float32)
        h.synchronize()
    elif leg in LEGS:
        run = epoch_batches if leg == "batches" else epoch_torch
        for e in range(2):
            run(e)
        ms = []
        for e in range(5):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(2 + e)
            ms.append((time.perf_counter() - t0) * 1e3)
        res.update(ms_per_epoch=sorted(ms)[2], ms_per_epoch_min=min(ms), ms_per_epoch_max=max(ms), minibatches=len(batches))
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
    """the gather kernels' dispatches from a rocprofv3 --kernel-trace --stats run of its own"""
    rocprof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    tmp = tempfile.mkdtemp(prefix="onpolicy_batches_trace_")
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
        if not seen["gs_k_opb_gather_f32"] or not seen["gs_k_ds_gather_f32"]:
            return dict(unavailable="no gs_k_opb_gather_f32 / gs_k_ds_gather_f32 dispatches in kernel_trace.csv")
        med = lambda v: sorted(v)[len(v) // 2]
        D = json.loads(r.stdout.strip().splitlines()[-1])["obs_dim"]
        # bytes per dispatch at n = MINIBATCH: float64 rows read, float32 rows written (the dataset gathers the next observation as well)
        moved = {"gs_k_opb_gather_f32": MINIBATCH * D * 12, "gs_k_ds_gather_f32": 2 * MINIBATCH * D * 12}
        out = dict(dispatches={k: dict(n=len(v), median_ns=med(v), min_ns=min(v), max_ns=max(v)) for k, v in seen.items() if v})
        for k, nbytes in moved.items():
            d = out["dispatches"][k]
            d["bytes"] = nbytes
            d["ns_per_mb"] = d["median_ns"] / (nbytes / 1e6)
            d["tb_per_s"] = nbytes / d["median_ns"] / 1e3
            d["of_streaming_rate"] = d["tb_per_s"] / STREAM_TBS
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
    per_round = {leg: [r["ms_per_epoch"] for r in rs] for leg, rs in rounds.items()}
    ms = {leg: mid(v) for leg, v in per_round.items()}
    summary = dict(B=B, T=T, minibatch=MINIBATCH, minibatches=rounds["batches"][0]["minibatches"], episode_length=EPISODE_LENGTH, rounds_per_leg=ROUNDS,
                   feeder="ieee123_like", solver="fbs", dtype="float32", ms_per_epoch=ms, rounds=per_round,
                   spread=max((max(v) - min(v)) / mid(v) for v in per_round.values()), batches_over_torch=ms["batches"] / ms["torch"],
                   trace=trace(B))
    print(json.dumps(summary), flush=True)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            json.dump(summary, f, indent=1); f.write("\n")


if __name__ == "__main__":
    main()
