#!/usr/bin/env python3
"""Closed-loop rollout rate: the MLP policy evaluated on the device inside gs_rollout against the host-driven loop it replaces.
123-bus feeder, B = 8192, sweep solver, network obs_dim -> 256 -> 256 -> 2 A with relu, each configuration in a fresh process of
its own, median of five:
    mlp        gs_rollout(T = 64, GS_POLICY_MLP): one policy kernel and one step per env step, nothing on the host in between
    mlp_f32    the same with the policy installed as compute="float32" (GS_COMPUTE_F32: gs_k_policy_mlp_f32)
    random     gs_rollout(T = 64, GS_POLICY_RANDOM): the fused rollout without a policy (what the environment alone sustains)
    host_f64   the loop of examples/device_policy_loop.py with the same network as a torch float64 module: per step one
               gs_step_device_ptr, one gs_step_device_view and the module's launches, driven from Python
    host_f32   the same with a float32 module (observations cast down, actions cast up)
    python tools/policy_rate.py [B] [--out profiles/policy_rollout_rate_f32.json] (on the GPU box; one JSON line per configuration)
    python tools/policy_rate.py --child mlp [B]                                   one configuration in this process (for a profiler)
Every configuration reports the median, the fastest and the slowest of its five timings.  profiles/policy_rollout_rate.json is the
record of the four configurations before mlp_f32 existed.
The host loops do not reset finished instances (the example does not); the rollouts do, in place."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = 64


def child(mode, B):
    import time
    import numpy as np
    sys.path.insert(0, ROOT)
    if mode.startswith("host"):          # (the consumer's runtime first, as tests/test_gpu_device_consumer.py brings it up)
        import torch
        if not torch.cuda.is_available():
            print(json.dumps(dict(mode=mode, B=B, T=T, unavailable="torch sees no GPU in this process")), flush=True)
            return
    import grid_fed_rl_gym_amd as P
    fs = P.ieee123_like()
    env = P.BatchedGridEnvironment(fs, num_envs=B, solver="fbs", stochastic_loads=True, weather_variation=True)
    h = env.handle
    rng = np.random.default_rng(1)
    dims = [fs.obs_dim, 256, 256, 2 * fs.action_dim]
    ws = [rng.normal(0.0, 1.0 / np.sqrt(dims[l]), (dims[l + 1], dims[l])) for l in range(3)]
    bs = [rng.normal(0.0, 0.1, dims[l + 1]) for l in range(3)]
    obs0, _ = env.reset(seed=np.arange(B, dtype=np.uint64))
    if mode in ("mlp", "mlp_f32", "random"):
        if mode != "random":
            env.set_policy(P.MLPPolicy(ws, bs, activation="relu", head="gaussian_tanh", compute="float32" if mode == "mlp_f32" else "float64"))
        def run(k):
            for _ in range(k // T):
                h.rollout(T, "random" if mode == "random" else "mlp", seed=7)
        sync = h.synchronize
        steps, warm = 4 * T, 2 * T
    else:
        import torch
        dt = torch.float64 if mode == "host_f64" else torch.float32
        net = torch.nn.Sequential(torch.nn.Linear(dims[0], dims[1]), torch.nn.ReLU(), torch.nn.Linear(dims[1], dims[2]), torch.nn.ReLU(),
                                  torch.nn.Linear(dims[2], dims[3])).to(dt)
        with torch.no_grad():
            for lin, w, b in zip([m for m in net if hasattr(m, "weight")], ws, bs):
                lin.weight.copy_(torch.from_numpy(w)); lin.bias.copy_(torch.from_numpy(b))
        net = net.cuda()
        stream = torch.cuda.current_stream().cuda_stream
        state = {"obs": torch.as_tensor(obs0, device="cuda")}
        A = fs.action_dim
        def run(k):
            obs = state["obs"]
            with torch.no_grad():
                for _ in range(k):
                    out = net(obs if dt == torch.float64 else obs.float())
                    actions = torch.tanh(out[:, :A]).to(torch.float64).contiguous()
                    obs_d, rew_d, term_d, trunc_d = env.step_device(actions, stream=stream)
                    obs = torch.as_tensor(obs_d, device="cuda")
            state["obs"] = obs
        def sync():
            torch.cuda.synchronize(); h.synchronize()
        steps, warm = 4 * T, 2 * T
    run(warm); sync()
    us = []
    for rep in range(5):
        t0 = time.perf_counter()
        run(steps); sync()
        us.append((time.perf_counter() - t0) / steps * 1e6)
    med = sorted(us)[2]
    print(json.dumps(dict(mode=mode, B=B, T=T, kernel=h.describe()["kernel"], us_per_step=med, us_per_step_min=min(us),
                          us_per_step_max=max(us), env_steps_per_s=B / med * 1e6, env_steps_per_s_min=B / max(us) * 1e6,
                          env_steps_per_s_max=B / min(us) * 1e6)), flush=True)
    env.close()


def run(mode, B):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", mode, str(B)], capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        raise SystemExit(f"{mode} failed ({r.returncode}): {r.stderr.strip()[-600:]}")
    line = r.stdout.strip().splitlines()[-1]
    print(line, flush=True)
    return json.loads(line)


def main():
    args = sys.argv[1:]
    out = None
    if "--out" in args:
        k = args.index("--out"); out = args[k + 1]; del args[k:k + 2]
    if args and args[0] == "--child":
        return child(args[1], int(args[2]) if len(args) > 2 else 8192)
    B = int(args[0]) if args else 8192
    res = {mode: run(mode, B) for mode in ("mlp", "mlp_f32", "random", "host_f64", "host_f32")}
    rate = {m: r.get("env_steps_per_s") for m, r in res.items()}
    ratio = lambda a, b: rate[a] / rate[b] if rate[a] and rate[b] else None
    summary = dict(B=B, T=T, feeder="ieee123_like", solver="fbs", network=[684, 256, 256, 16], activation="relu", env_steps_per_s=rate,
                   env_steps_per_s_min={m: r.get("env_steps_per_s_min") for m, r in res.items()},
                   env_steps_per_s_max={m: r.get("env_steps_per_s_max") for m, r in res.items()},
                   us_per_step={m: r.get("us_per_step") for m, r in res.items()},
                   us_per_step_min={m: r.get("us_per_step_min") for m, r in res.items()},
                   us_per_step_max={m: r.get("us_per_step_max") for m, r in res.items()},
                   unavailable={m: r["unavailable"] for m, r in res.items() if "unavailable" in r},
                   mlp_over_host_f64=ratio("mlp", "host_f64"), mlp_over_host_f32=ratio("mlp", "host_f32"),
                   mlp_over_random=ratio("mlp", "random"), mlp_f32_over_host_f32=ratio("mlp_f32", "host_f32"),
                   mlp_f32_over_mlp=ratio("mlp_f32", "mlp"),
                   mlp_f32_slowest_over_host_f32_fastest=(res["mlp_f32"]["env_steps_per_s_min"] / res["host_f32"]["env_steps_per_s_max"]
                                                          if "env_steps_per_s_min" in res["mlp_f32"] and "env_steps_per_s_max" in res["host_f32"] else None))
    print(json.dumps(summary), flush=True)
    if out:
        with open(out, "w") as f:
            json.dump(summary, f, indent=1); f.write("\n")


if __name__ == "__main__":
    main()
