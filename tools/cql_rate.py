#!/usr/bin/env python3
"""The conservative critic step on the device: one epoch of CQL -- evaluate_rollout_q_next (the policy over the
rollout's next states, the target twins on its actions, the Bellman target), then per minibatch DeviceLearner.step on Q1 and Q2
(gs_learner_step_conservative: the regression plus conservative_weight x the logsumexp penalty over 3 n rows) and the policy
(gs_learner_step_pathwise) plus update_targets -- against the same epoch in torch.  The protocol of tools/q_next_rate.py: 123-bus
feeder, sweep solver, B = 8192, T = 64, minibatch 4096, float32, nets 692 -> 256 -> 256 -> 1 (Q) and 684 -> 256 -> 256 -> 16 (policy);
every visit a fresh process, under a time limit of its own, with two warm-up epochs and its own median of five.  The expectation,
stated before measuring: device <= 1.0 x torch in EVERY round.
    device     ms per epoch as above, host clock around the epoch and a synchronise
    torch      ms per epoch: the same batches (observations, actions, indices from the device) into torch float32 autograd of the
               reference's CQL.update (offline.py:138-249): next actions by rsample and the target twins under no_grad, per twin the
               mse plus conservative_weight x (logsumexp over the batch of Q on uniform, policy and data actions - mean Q on data),
               the actor through the twins, torch.optim.Adam, the soft update of torch target towers; plus, at the end of the epoch,
               the round trip of the weights to the handle (set_policy, set_q twice), which the device leg does not need.
               The legs ALTERNATE for ROUNDS rounds; every round is kept.
    td3bc      beside the bar: device ms per epoch over the TD3 + BC epoch recorded in profiles/q_next_rate.json (the twins' passes run
               over 3 n rows here, so somewhat under 3 x on the Q part is expected; an observation, not a bar)
    trace      rocprofv3 --kernel-trace --stats of a run of its own (no counters), two device epochs: the kernels of an epoch, and
               gs_k_cql_lse (ONE workgroup) beside the per-minibatch gs_k_train_reduce
    python tools/cql_rate.py [B] [--out profiles/cql_rate.json]     (on the GPU box)
    python tools/cql_rate.py --child LEG [B]                         one leg in this process"""
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
LEGS = ("torch", "device")
HIDDEN = [256, 256]
ALPHA, CW, TAU, GAMMA = 0.2, 5.0, 0.005, 0.99
LEG_SECONDS = 300      # a visit's own time limit
KERNELS = ("gs_k_policy_rows_f32", "gs_k_value_mlp_f32", "gs_k_q_mlp_f32", "gs_k_q_mlp_rows_f32", "gs_k_q_next_td", "gs_k_q_gather", "gs_k_pw_sample",
           "gs_k_pw_head", "gs_k_cql_rows", "gs_k_cql_lse", "gs_k_cql_head", "gs_k_cql_stats", "gs_k_train_forward", "gs_k_train_bwd_data", "gs_k_train_grad", "gs_k_train_reduce", "gs_k_train_adam", "gs_k_q_polyak")


def _layers(dims, rng, last_scale=1.0):
    import numpy as np
    ws = [rng.normal(0.0, 1.0 / np.sqrt(dims[l]), (dims[l + 1], dims[l])) for l in range(len(dims) - 1)]
    ws[-1] *= last_scale
    return ws, [rng.normal(0.0, 0.1, dims[l + 1]) for l in range(len(dims) - 1)]


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
    import copy
    import time
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import grid_fed_rl_gym_amd as P
    fs = P.ieee123_like()
    D, A = fs.obs_dim, fs.action_dim
    env = P.BatchedGridEnvironment(fs, num_envs=B, solver="fbs", stochastic_loads=True, weather_variation=True, episode_length=EPISODE_LENGTH)
    h = env.handle
    rng = np.random.default_rng(1)
    pol_l, val_l = _layers([D] + HIDDEN + [2 * A], rng, 0.3), _layers([D] + HIDDEN + [1], rng)
    q_l = [_layers([D + A] + HIDDEN + [1], rng) for _ in range(2)]
    mean, std = rng.normal(0.0, 1.0, D), rng.uniform(0.5, 2.0, D)
    policy = P.MLPPolicy(*pol_l, activation="relu", compute="float32", obs_mean=mean, obs_std=std)
    env.set_policy(policy, stochastic=True)
    env.set_value(P.MLPValue(*val_l, activation="relu", obs_mean=mean, obs_std=std))      # (gs_onpolicy_prepare's; and the trace's yardstick)
    for w in range(2):
        env.set_q(w, P.MLPQ(*q_l[w], D, activation="relu", obs_mean=mean, obs_std=std))
    env.reset(seed=np.arange(B, dtype=np.uint64))
    h.rollout(T, "random", seed=7)
    stream = torch.cuda.current_stream().cuda_stream
    view = lambda x: torch.as_tensor(x, device="cuda")
    bootstrap = ()          # the reference's (1 - terminals)
    P.evaluate_rollout(env, gamma=GAMMA)
    batches = P.OnPolicyBatches(env, MINIBATCH, policy=policy, adv_norm="none", dtype=np.float32, fields=["observations", "actions", "indices"])
    batches.prepare()       # (once: the fields served here do not change with the evaluations)

    learner = None
    if leg in ("device", "trace_child"):
        learner = P.DeviceLearner(env, nets=("q1", "q2", "policy"), lr=3e-4, policy_loss="pathwise", alpha=ALPHA, pathwise_seed=7,
                                  q_target="policy", conservative_weight=CW, conservative_seed=13)

    def epoch_device(e):
        P.evaluate_rollout_q_next(env, gamma=GAMMA, alpha=ALPHA, bootstrap=bootstrap, seed=11, draw=e)
        for b in batches.epoch(e):
            learner.step(b)
            learner.update_targets(TAU)
        h.synchronize()

    actor = _sequential(torch, *pol_l).cuda()
    towers = [_sequential(torch, *q_l[w]).cuda() for w in range(2)]
    targets = [copy.deepcopy(t) for t in towers]
    opt = torch.optim.Adam([p for m in [actor] + towers for p in m.parameters()], lr=3e-4)
    t_mean, t_inv = torch.as_tensor(mean, device="cuda"), torch.as_tensor(1.0 / std, device="cuda")

    def sample(obs_n):
        m, log_std = torch.chunk(actor(obs_n), 2, dim=-1)
        log_std = torch.clamp(log_std, -20.0, 2.0)
        eps = torch.randn_like(m)
        a = torch.tanh(m + torch.exp(log_std) * eps)
        lp = (-0.5 * eps * eps - log_std - 0.5 * np.log(2.0 * np.pi) - torch.log(1.0 - a * a + 1e-6)).sum(dim=-1)
        return a, lp

    def epoch_torch(e):
        dev = h.rollout_device_arrays()
        obs_seq, rew, done = view(dev["obs_seq"]), view(dev["rewards"]).reshape(-1), view(dev["terminals"]).reshape(-1)
        nxt = obs_seq[1:].reshape(-1, D)
        for b in batches.epoch(e, stream=stream):
            obs_n, actions, idx = view(b["observations"]), view(b["actions"]), view(b["indices"]).long()
            with torch.no_grad():          # offline.py:173-178
                next_n = ((nxt[idx] - t_mean) * t_inv).float()
                na, nlp = sample(next_n)
                ns = torch.cat([next_n, na], dim=-1)
                tq = torch.min(targets[0](ns), targets[1](ns)).squeeze(-1) - ALPHA * nlp
                y = rew[idx].float() + GAMMA * (1.0 - (done[idx] != 0).float()) * tq
            sa = torch.cat([obs_n, actions], dim=-1)
            with torch.no_grad():          # the candidates are constants of the critic's step (offline.py:209-215)
                ra = torch.empty_like(actions).uniform_(-1.0, 1.0)
                ca, _ = sample(obs_n)
            q_loss = 0.0
            for t in towers:               # offline.py:181-196, 217-228
                q_data = t(sa)
                cat = torch.cat([t(torch.cat([obs_n, ra], dim=-1)), t(torch.cat([obs_n, ca], dim=-1)), q_data], dim=0)
                q_loss = q_loss + torch.nn.functional.mse_loss(q_data.squeeze(-1), y) + CW * (torch.logsumexp(cat, dim=0).squeeze() - q_data.mean())
            a, lp = sample(obs_n)
            for t in towers:
                t.requires_grad_(False)            # the actor's loss moves the policy alone
            pa = torch.cat([obs_n, a], dim=-1)
            q_pi = torch.min(towers[0](pa), towers[1](pa)).squeeze(-1)
            for t in towers:
                t.requires_grad_(True)
            actor_loss = (ALPHA * lp - q_pi).mean()
            loss = actor_loss + q_loss
            opt.zero_grad(); loss.backward(); opt.step()
            with torch.no_grad():
                for t, tt in zip(towers, targets):
                    for p, tp in zip(t.parameters(), tt.parameters()):
                        tp.mul_(1.0 - TAU).add_(p, alpha=TAU)
            torch.cuda.current_stream().synchronize()          # the next batch reuses the handle's buffers
        # the weights back to the handle, for the next rollout or evaluation
        env.set_policy(P.MLPPolicy.from_sequential(actor, obs_mean=mean, obs_std=std, compute="float32"), stochastic=True)
        for w in range(2):
            env.set_q(w, P.MLPQ.from_sequential(towers[w], obs_mean=mean, obs_std=std))
        torch.cuda.synchronize()

    res = dict(leg=leg, B=B, T=T, minibatch=MINIBATCH, obs_dim=D, action_dim=A)
    if leg == "trace_child":
        P.evaluate_rollout(env, gamma=GAMMA)
        for e in range(2):
            epoch_device(e)
        res.update(minibatches=len(batches), rows=B * T)
    elif leg in LEGS:
        run = epoch_device if leg == "device" else epoch_torch
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
            res.update(stats={net: {k: (None if x != x else x) for k, x in learner.stats(net).items()} for net in learner.nets})
    else:
        raise SystemExit(f"unknown leg {leg}")
    print(json.dumps(res), flush=True)
    env.close()


def run(leg, B):
    r = subprocess.run(["timeout", "-k", "10", str(LEG_SECONDS), sys.executable, os.path.abspath(__file__), "--child", leg, str(B)], capture_output=True, text=True)
    if r.returncode != 0:
        raise SystemExit(f"{leg} failed ({r.returncode}): {r.stderr.strip()[-600:]}")
    line = r.stdout.strip().splitlines()[-1]
    print(line, flush=True)
    return json.loads(line)


def trace(B):
    """the kernels' dispatches from a rocprofv3 --kernel-trace --stats run of its own"""
    rocprof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    tmp = tempfile.mkdtemp(prefix="cql_trace_")
    try:
        r = subprocess.run(["timeout", "-k", "10", str(LEG_SECONDS), rocprof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--", sys.executable,
                            os.path.abspath(__file__), "--child", "trace_child", str(B)], capture_output=True, text=True)
        if r.returncode != 0:
            return dict(unavailable=f"rocprofv3 failed ({r.returncode}): {r.stderr.strip()[-300:]}")
        seen = {k: [] for k in KERNELS}
        for f in glob.glob(os.path.join(tmp, "**", "*kernel_trace.csv"), recursive=True):
            for row in csv.DictReader(open(f)):
                name = row["Kernel_Name"].split("(")[0]
                if name in seen:
                    seen[name].append(int(row["End_Timestamp"]) - int(row["Start_Timestamp"]))
        if not seen["gs_k_cql_lse"]:
            return dict(unavailable="no gs_k_cql_lse dispatches in kernel_trace.csv")
        med = lambda v: sorted(v)[len(v) // 2]
        out = dict(dispatches={k: dict(n=len(v), median_ns=med(v), min_ns=min(v), max_ns=max(v)) for k, v in seen.items() if v})
        out["sum_ns"] = {k: sum(v) for k, v in seen.items() if v}
        # the single workgroup of the logsumexp beside the gradient reduction of the same minibatch
        if seen["gs_k_train_reduce"]:
            out["cql_lse_over_train_reduce"] = med(seen["gs_k_cql_lse"]) / med(seen["gs_k_train_reduce"])
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
    summary = dict(B=B, T=T, minibatch=MINIBATCH, minibatches=rounds["device"][0]["minibatches"], episode_length=EPISODE_LENGTH, rounds_per_leg=ROUNDS,
                   feeder="ieee123_like", solver="fbs", dtype="float32", alpha=ALPHA, conservative_weight=CW, tau=TAU,
                   ms_per_epoch=ms, rounds=per_round, spread=max((max(v) - min(v)) / mid(v) for v in per_round.values()),
                   device_over_torch=ms["device"] / ms["torch"],
                   device_over_torch_per_round=[a / b for a, b in zip(per_round["device"], per_round["torch"])],
                   stats=rounds["device"][-1]["stats"])
    td3bc = os.path.join(ROOT, "profiles", "q_next_rate.json")
    if os.path.exists(td3bc):
        with open(td3bc) as f:
            summary["device_over_td3bc_epoch"] = ms["device"] / json.load(f)["ms_per_epoch"]["device"]
    summary["trace"] = trace(B)
    print(json.dumps(summary), flush=True)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            json.dump(summary, f, indent=1); f.write("\n")


if __name__ == "__main__":
    main()
