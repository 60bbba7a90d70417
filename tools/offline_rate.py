#!/usr/bin/env python3
"""The learner's offline losses on the device: one epoch of OnPolicyBatches plus DeviceLearner.step under AWR and
the expectile loss against the same losses in torch, and the new kernels' own times.  The protocol of tools/learner_rate.py: 123-bus
feeder, sweep solver, B = 8192, T = 64, minibatch 4096, float32, policy 684 -> 256 -> 256 -> 16 plus the reward critic; every visit a
fresh process with warm-up and its own median of five.  The bar, stated before measuring: learner <= 1.0 x torch on the median of the
rounds.
    learner    ms per epoch of OnPolicyBatches.epoch with DeviceLearner(policy_loss="awr", value_loss="expectile").step on every
               minibatch (policy and value), host clock around the epoch and a synchronise
    torch      ms per epoch of the same batches into torch float32 autograd (the same two losses) and torch.optim.Adam, plus, at the
               end of the epoch, the round trip of the weights to the handle, which the learner leg does not need
               The legs ALTERNATE for ROUNDS rounds; a leg's figure is the median of its rounds, every round is kept, and `spread`
               is the largest (max - min) / median over the rounds of one leg
    trace      rocprofv3 --kernel-trace --stats of a run of its own (no counters): two epochs under the default losses, then two under
               AWR and the expectile loss, so that gs_k_train_head_awr / _expectile / gs_k_train_stats_awr stand beside gs_k_train_head
               and gs_k_train_stats in ONE trace.  (gs_k_train_head and gs_k_train_stats serve the policy and the critic of the
               default epochs alike, and gs_k_train_stats also the expectile critic: their policy dispatches are the slower half.)
The collection is a stochastic policy rollout, so that the trace's default epochs can run; the offline losses read no log-probability.
    python tools/offline_rate.py [B] [--out profiles/offline_rate.json]     (on the GPU box)
    python tools/offline_rate.py --child LEG [B]                             one leg in this process"""
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
LEGS = ("torch", "learner")
HIDDEN = [256, 256]
TEMPERATURE, WEIGHT_MAX, EXPECTILE = 1.0, 20.0, 0.7
KERNELS = ("gs_k_train_head", "gs_k_train_head_awr", "gs_k_train_head_expectile", "gs_k_train_stats", "gs_k_train_stats_awr", "gs_k_train_forward",
           "gs_k_train_bwd_data", "gs_k_train_grad", "gs_k_train_reduce", "gs_k_train_adam")


def _networks(fs):
    import numpy as np
    rng = np.random.default_rng(1)
    out = []
    for last in (2 * fs.action_dim, 1):
        dims = [fs.obs_dim] + HIDDEN + [last]
        out.append(([rng.normal(0.0, 1.0 / np.sqrt(dims[l]), (dims[l + 1], dims[l])) for l in range(3)],
                    [rng.normal(0.0, 0.1, dims[l + 1]) for l in range(3)]))
    return out


def _sequential(torch, ws, bs):
    mods = []
    for l, (w, b) in enumerate(zip(ws, bs)):
        lin = torch.nn.Linear(w.shape[1], w.shape[0])
        with torch.no_grad():
            lin.weight.copy_(torch.as_tensor(w, dtype=torch.float32)); lin.bias.copy_(torch.as_tensor(b, dtype=torch.float32))
        mods.append(lin)
        if l < len(ws) - 1:
            mods.append(torch.nn.ReLU())
    return torch.nn.Sequential(*mods)


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
    env.reset(seed=np.arange(B, dtype=np.uint64))
    h.rollout(T, "mlp", seed=7)
    stream = torch.cuda.current_stream().cuda_stream
    P.evaluate_rollout(env, bootstrap=("terminated", "truncated"), stream=stream)
    view = lambda x: torch.as_tensor(x, device="cuda")
    A = fs.action_dim
    batches = P.OnPolicyBatches(env, MINIBATCH, policy=policy, adv_norm="minibatch", dtype=np.float32)
    batches.prepare()

    offline = dict(policy_loss="awr", temperature=TEMPERATURE, weight_max=WEIGHT_MAX, value_loss="expectile", expectile=EXPECTILE)
    learner = None
    if leg == "learner":
        learner = P.DeviceLearner(env, nets=("policy", "value"), lr=3e-4, **offline)
    elif leg == "trace_child":
        learner = P.DeviceLearner(env, nets=("policy", "value"), lr=3e-4, clip=0.2)

    def epoch_learner(e):
        for b in batches.epoch(e):
            learner.step(b)
        h.synchronize()

    actor, critic = _sequential(torch, *nets[0]).cuda(), _sequential(torch, *nets[1]).cuda()
    opt = torch.optim.Adam(list(actor.parameters()) + list(critic.parameters()), lr=3e-4)

    def epoch_torch(e):
        for b in batches.epoch(e, stream=stream):
            obs_n, actions = view(b["observations"]), view(b["actions"])
            adv, ret = view(b["advantages"]), view(b["returns"])
            m, log_std = torch.chunk(actor(obs_n), 2, dim=-1)
            log_std = torch.clamp(log_std, -20.0, 2.0)
            x = torch.atanh(torch.clamp(actions, -1.0 + 1e-7, 1.0 - 1e-7))
            eps = (x - m) * torch.exp(-log_std)
            lp = (-0.5 * eps * eps - log_std - 0.5 * np.log(2.0 * np.pi) - torch.log(1.0 - actions * actions + 1e-6)).sum(dim=-1)
            weight = torch.clamp(torch.exp(adv / TEMPERATURE), max=WEIGHT_MAX)
            d = critic(obs_n).squeeze(-1) - ret
            value_loss = (torch.where(d < 0, EXPECTILE, 1.0 - EXPECTILE) * d * d).mean()
            loss = -(weight * lp).mean() + value_loss
            opt.zero_grad(); loss.backward(); opt.step()
            torch.cuda.current_stream().synchronize()          # the next batch reuses the handle's buffers
        # the weights back to the handle, for the next evaluation of the rollout
        env.set_policy(P.MLPPolicy.from_sequential(actor, obs_mean=mean, obs_std=std, compute="float32"), stochastic=True)
        env.set_value(P.MLPValue.from_sequential(critic, obs_mean=mean, obs_std=std))
        torch.cuda.synchronize()

    res = dict(leg=leg, B=B, T=T, minibatch=MINIBATCH, obs_dim=fs.obs_dim, action_dim=A)
    if leg == "trace_child":
        for e in range(2):
            epoch_learner(e)
        learner.set_loss("policy", "awr", temperature=TEMPERATURE, weight_max=WEIGHT_MAX)
        learner.set_loss("value", "expectile", expectile=EXPECTILE)
        for e in range(2, 4):
            epoch_learner(e)
        res.update(minibatches=len(batches))
    elif leg in LEGS:
        run = epoch_learner if leg == "learner" else epoch_torch
        for e in range(2):
            run(e)
        ms = []
        for e in range(5):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(2 + e)
            ms.append((time.perf_counter() - t0) * 1e3)
        res.update(ms_per_epoch=sorted(ms)[2], ms_per_epoch_min=min(ms), ms_per_epoch_max=max(ms), minibatches=len(batches))
        if learner is not None:
            res.update(stats=learner.stats("policy"), value_stats=learner.stats("value"))
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
    """the head and statistics kernels' dispatches from a rocprofv3 --kernel-trace --stats run of its own"""
    rocprof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    tmp = tempfile.mkdtemp(prefix="offline_trace_")
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
        if not seen["gs_k_train_head_awr"]:
            return dict(unavailable="no gs_k_train_head_awr dispatches in kernel_trace.csv")
        med = lambda v: sorted(v)[len(v) // 2]
        out = dict(dispatches={k: dict(n=len(v), median_ns=med(v), min_ns=min(v), max_ns=max(v)) for k, v in seen.items() if v})
        # gs_k_train_head and gs_k_train_stats also serve critics, which are much cheaper: their policy dispatches (the default epochs',
        # as many as the AWR kernel has) are the slowest ones
        n_policy = len(seen["gs_k_train_head_awr"])
        for k in ("gs_k_train_head", "gs_k_train_stats"):
            v = sorted(seen[k])
            out["dispatches"][k].update(policy_n=n_policy, policy_median_ns=med(v[-n_policy:]), critic_median_ns=med(v[:-n_policy]))
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
    summary = dict(B=B, T=T, minibatch=MINIBATCH, minibatches=rounds["learner"][0]["minibatches"], episode_length=EPISODE_LENGTH, rounds_per_leg=ROUNDS,
                   feeder="ieee123_like", solver="fbs", dtype="float32", temperature=TEMPERATURE, weight_max=WEIGHT_MAX, expectile=EXPECTILE,
                   ms_per_epoch=ms, rounds=per_round, spread=max((max(v) - min(v)) / mid(v) for v in per_round.values()),
                   learner_over_torch=ms["learner"] / ms["torch"],
                   stats={k: (None if x != x else x) for k, x in rounds["learner"][-1]["stats"].items()},      # (NaN is not JSON)
                   trace=trace(B))
    print(json.dumps(summary), flush=True)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            json.dump(summary, f, indent=1); f.write("\n")


if __name__ == "__main__":
    main()
