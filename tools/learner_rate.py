#!/usr/bin/env python3
"""The learner on the device: one epoch of OnPolicyBatches plus DeviceLearner.step against the route it
replaces, and the learner kernels' own times.  The protocol of tools/onpolicy_batches_rate.py: 123-bus feeder, sweep solver, B = 8192,
T = 64, minibatch 4096, float32, policy 684 -> 256 -> 256 -> 32 plus the reward critic; every visit a fresh process with warm-up and
its own median of five.  The bar, stated before measuring: learner <= 1.0 x torch on the median of the rounds.
    learner    ms per epoch of OnPolicyBatches.epoch with DeviceLearner.step on every minibatch (policy and value), host clock around
               the epoch and a synchronise
    torch      ms per epoch of the same batches into torch float32 autograd and torch.optim.Adam -- the loop of
               examples/device_ppo_epochs.py without cost critics -- plus, at the end of the epoch, the round trip of the weights to
               the handle (MLPPolicy.from_sequential, set_policy, set_value), which the learner leg does not need
               The legs ALTERNATE for ROUNDS rounds; a leg's figure is the median of its rounds, every round is kept, and `spread`
               is the largest (max - min) / median over the rounds of one leg
    trace      rocprofv3 --kernel-trace --stats of a run of its own (no counters): the gs_k_train_* kernels per dispatch, and the
               rate of the three matrix kernels on the policy's step against the 79 TFLOP/s gs_k_value_mlp_f32 reaches
    python tools/learner_rate.py [B] [--out profiles/learner_rate.json]     (on the GPU box)
    python tools/learner_rate.py --child LEG [B]                             one leg in this process"""
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
KERNELS = ("gs_k_train_forward", "gs_k_train_head", "gs_k_train_bwd_data", "gs_k_train_grad", "gs_k_train_reduce", "gs_k_train_stats",
           "gs_k_train_adam", "gs_k_opb_gather_f32", "gs_k_opb_index")
VALUE_KERNEL_TFLOPS = 79.0


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

    learner = P.DeviceLearner(env, nets=("policy", "value"), lr=3e-4, clip=0.2) if leg in ("learner", "trace_child") else None

    def epoch_learner(e):
        for b in batches.epoch(e):
            learner.step(b)
        h.synchronize()

    actor, critic = _sequential(torch, *nets[0]).cuda(), _sequential(torch, *nets[1]).cuda()
    opt = torch.optim.Adam(list(actor.parameters()) + list(critic.parameters()), lr=3e-4)

    def epoch_torch(e):
        for b in batches.epoch(e, stream=stream):
            obs_n, actions = view(b["observations"]), view(b["actions"])
            lp_old, adv, ret = view(b["log_probs"]), view(b["advantages"]), view(b["returns"])
            m, log_std = torch.chunk(actor(obs_n), 2, dim=-1)
            log_std = torch.clamp(log_std, -20.0, 2.0)
            x = torch.atanh(torch.clamp(actions, -1.0 + 1e-7, 1.0 - 1e-7))
            eps = (x - m) * torch.exp(-log_std)
            lp = (-0.5 * eps * eps - log_std - 0.5 * np.log(2.0 * np.pi) - torch.log(1.0 - actions * actions + 1e-6)).sum(dim=-1)
            ratio = torch.exp(lp - lp_old)
            surrogate = torch.minimum(ratio * adv, torch.clamp(ratio, 0.8, 1.2) * adv).mean()
            value_loss = (critic(obs_n).squeeze(-1) - ret).pow(2).mean()
            loss = -surrogate + value_loss
            opt.zero_grad(); loss.backward(); opt.step()
            torch.cuda.current_stream().synchronize()          # the next batch reuses the handle's buffers
        # the weights back to the handle, for the next rollout
        env.set_policy(P.MLPPolicy.from_sequential(actor, obs_mean=mean, obs_std=std, compute="float32"), stochastic=True)
        env.set_value(P.MLPValue.from_sequential(critic, obs_mean=mean, obs_std=std))
        torch.cuda.synchronize()

    res = dict(leg=leg, B=B, T=T, minibatch=MINIBATCH, obs_dim=fs.obs_dim, action_dim=A)
    if leg == "trace_child":
        for e in range(2):
            epoch_learner(e)
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
            res.update(stats=learner.stats("policy"))
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
    """the learner kernels' dispatches from a rocprofv3 --kernel-trace --stats run of its own"""
    rocprof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    tmp = tempfile.mkdtemp(prefix="learner_trace_")
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
        if not seen["gs_k_train_forward"]:
            return dict(unavailable="no gs_k_train_forward dispatches in kernel_trace.csv")
        med = lambda v: sorted(v)[len(v) // 2]
        info = json.loads(r.stdout.strip().splitlines()[-1])
        out = dict(dispatches={k: dict(n=len(v), median_ns=med(v), min_ns=min(v), max_ns=max(v)) for k, v in seen.items() if v})
        # the policy's dispatches are the slower half of a matrix kernel's (policy and value alternate): flops of the policy's step
        dims = [info["obs_dim"]] + HIDDEN + [2 * info["action_dim"]]
        macs = [dims[l] * dims[l + 1] for l in range(3)]
        flops = {"gs_k_train_forward": 2 * MINIBATCH * sum(macs), "gs_k_train_bwd_data": 2 * MINIBATCH * sum(macs[1:]),
                 "gs_k_train_grad": 2 * MINIBATCH * sum(macs)}
        for k, f in flops.items():
            v = sorted(seen[k])
            policy_ns = med(v[len(v) // 2:])
            out["dispatches"][k].update(policy_median_ns=policy_ns, policy_flops=f, policy_tflops=f / policy_ns / 1e3,
                                        of_value_kernel=f / policy_ns / 1e3 / VALUE_KERNEL_TFLOPS)
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
                   feeder="ieee123_like", solver="fbs", dtype="float32", ms_per_epoch=ms, rounds=per_round,
                   spread=max((max(v) - min(v)) / mid(v) for v in per_round.values()), learner_over_torch=ms["learner"] / ms["torch"],
                   trace=trace(B))
    print(json.dumps(summary), flush=True)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            json.dump(summary, f, indent=1); f.write("\n")


if __name__ == "__main__":
    main()
