#!/usr/bin/env python3
"""Parameter anchors: what the terms cost a learner's epoch, that switched off they cost nothing, and what a
consolidation costs.  The protocol of tools/learner_rate.py: 123-bus feeder, sweep solver, B = 8192, T = 64, 128 minibatches of 4096,
float32, policy 684 -> 256 -> 256 -> 32 plus the reward critic; every visit a fresh process with two warm-up epochs and its own median
of five; the legs ALTERNATE for ROUNDS rounds, a leg's figure is the median of its rounds, every round is kept.
    off          ms per epoch of OnPolicyBatches.epoch with DeviceLearner.step on every minibatch (policy and value), both coefficients 0
    on           the same epoch with prox_mu and ewc_lambda on for both networks (anchored and consolidated before the clock starts)
    consolidate  ms per DeviceLearner.consolidate of both networks over that epoch's minibatches
    parent       the `off` leg in a built checkout of the parent commit (--parent ROOT): the same file, that tree's package
The only bar, stated before measuring: off / parent - 1 must lie within the parent leg's own round-to-round spread, (max - min) /
median over its rounds.  on / off and consolidate / off are reported, not judged.
    python tools/anchor_rate.py [B] [--parent ROOT] [--out profiles/anchor_rate.json]     (on the GPU box)
    python tools/anchor_rate.py --child LEG [B] [--root ROOT]                              one leg in this process"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = 64
MINIBATCH = 4096
ROUNDS = 3
EPISODE_LENGTH = 24
HIDDEN = [256, 256]
PROX_MU, EWC_LAMBDA = 0.01, 100.0


def _networks(fs):
    import numpy as np
    rng = np.random.default_rng(1)
    out = []
    for last in (2 * fs.action_dim, 1):
        dims = [fs.obs_dim] + HIDDEN + [last]
        out.append(([rng.normal(0.0, 1.0 / np.sqrt(dims[l]), (dims[l + 1], dims[l])) for l in range(3)],
                    [rng.normal(0.0, 0.1, dims[l + 1]) for l in range(3)]))
    return out


def child(leg, B, root):
    import time
    import numpy as np
    sys.path.insert(0, root)
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
    P.evaluate_rollout(env, bootstrap=("terminated", "truncated"))
    batches = P.OnPolicyBatches(env, MINIBATCH, policy=policy, adv_norm="minibatch", dtype=np.float32)
    batches.prepare()
    names = ("policy", "value")
    learner = P.DeviceLearner(env, nets=names, lr=3e-4, clip=0.2)
    if leg == "on":
        for net in names:
            learner.anchor_here(net)
            learner.consolidate(net, batches.epoch(0))

    def epoch_step(e):
        for b in batches.epoch(e):
            learner.step(b)
        h.synchronize()

    def epoch_consolidate(e):
        for net in names:
            learner.consolidate(net, batches.epoch(e))
        h.synchronize()

    run = epoch_consolidate if leg == "consolidate" else epoch_step
    for e in range(2):
        run(e)
    if leg == "on":                                                    # (after two free epochs: w differs from both centres)
        for net in names:
            learner.set_anchor(net, prox_mu=PROX_MU, ewc_lambda=EWC_LAMBDA)
        run(2)
    ms = []
    for e in range(5):
        h.synchronize()
        t0 = time.perf_counter()
        run(3 + e)
        ms.append((time.perf_counter() - t0) * 1e3)
    res = dict(leg=leg, B=B, T=T, minibatch=MINIBATCH, minibatches=len(batches), ms_per_epoch=sorted(ms)[2], ms_per_epoch_min=min(ms),
               ms_per_epoch_max=max(ms))
    if leg == "on":
        res.update(anchor_stats={net: learner.anchor_stats(net) for net in names})
    print(json.dumps(res), flush=True)
    env.close()


def run(leg, B, root):
    what = "off" if leg == "parent" else leg
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", what, str(B), "--root", root], capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        raise SystemExit(f"{leg} failed ({r.returncode}): {r.stderr.strip()[-600:]}")
    line = r.stdout.strip().splitlines()[-1]
    print(leg, line, flush=True)
    return json.loads(line)


def _option(args, name):
    if name not in args:
        return None
    k = args.index(name)
    value = args[k + 1]
    del args[k:k + 2]
    return value


def main():
    args = sys.argv[1:]
    out, parent, root = _option(args, "--out"), _option(args, "--parent"), _option(args, "--root")
    if args and args[0] == "--child":
        return child(args[1], int(args[2]) if len(args) > 2 else 8192, root or ROOT)
    B = int(args[0]) if args else 8192
    legs = ("off", "on", "consolidate") + (("parent",) if parent else ())
    rounds = {}
    for r in range(ROUNDS):
        for leg in legs:
            rounds.setdefault(leg, []).append(run(leg, B, os.path.abspath(parent) if leg == "parent" else ROOT))
    mid = lambda v: sorted(v)[len(v) // 2]
    per_round = {leg: [r["ms_per_epoch"] for r in rs] for leg, rs in rounds.items()}
    ms = {leg: mid(v) for leg, v in per_round.items()}
    spread = {leg: (max(v) - min(v)) / mid(v) for leg, v in per_round.items()}
    summary = dict(B=B, T=T, minibatch=MINIBATCH, minibatches=rounds["off"][0]["minibatches"], episode_length=EPISODE_LENGTH, rounds_per_leg=ROUNDS,
                   feeder="ieee123_like", solver="fbs", dtype="float32", prox_mu=PROX_MU, ewc_lambda=EWC_LAMBDA, ms_per_epoch=ms, rounds=per_round,
                   spread=spread, on_over_off=ms["on"] / ms["off"], consolidate_over_off=ms["consolidate"] / ms["off"])
    if parent:
        summary.update(off_over_parent=ms["off"] / ms["parent"], bar="|off / parent - 1| <= the parent leg's spread",
                       within_bar=abs(ms["off"] / ms["parent"] - 1.0) <= spread["parent"])
    else:
        summary.update(off_over_parent=None, bar="not measured: no --parent checkout given")
    print(json.dumps(summary), flush=True)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            json.dump(summary, f, indent=1); f.write("\n")


if __name__ == "__main__":
    main()
