#!/usr/bin/env python3
"""Sustained rate of the per-instance-impedance step against the shared handle: 2000 steps back to back (no synchronisation in
between), median of five, each configuration in a fresh process of its own.  123-bus feeder, B = 8192, both solvers:
    shared        the handle's one set of line impedances
    no_flat       (Newton-Raphson) the shared handle under GS_NR_NO_FLAT=1: iteration 0 eliminated like the per-instance handle does
    per_instance  +-10 % per-instance impedances (randomized_line_impedances)
    python tools/pz_rate.py            (on the GPU box; prints one JSON line per configuration and the ratios)
    python tools/pz_rate.py --loads    per-instance load powers (randomized_load_powers, one U(0.5, 1.5) multiplier per instance) on the same
                                       protocol: shared | loads | per_instance (line impedances) | both, for both solvers"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = r'''
import json, sys, time, numpy as np
sys.path.insert(0, %r)
import grid_fed_rl_gym_amd as P
solver, mode, B = sys.argv[1], sys.argv[2], int(sys.argv[3])
fs = P.ieee123_like()
kw = {}
if mode in ("per_instance", "both"): kw["line_impedances"] = P.randomized_line_impedances(fs, B, rel=0.1, seed=0)
if mode in ("loads", "both"): kw["load_powers"] = P.randomized_load_powers(fs, B, low=0.5, high=1.5, seed=0)
env = P.BatchedGridEnvironment(fs, num_envs=B, solver=solver, stochastic_loads=True, weather_variation=True, **kw)
h = env.handle
acts = np.random.default_rng(5678).uniform(-1, 1, (8, B, fs.action_dim)); h.upload_actions(acts)
env.reset(seed=np.arange(B, dtype=np.uint64))
for k in range(500): h.step_device(k %% 8)
h.synchronize()
us = []
for rep in range(5):
    t0 = time.perf_counter()
    for k in range(2000): h.step_device(k %% 8)
    h.synchronize()
    us.append((time.perf_counter() - t0) / 2000 * 1e6)
med = sorted(us)[2]
print(json.dumps(dict(solver=solver, mode=mode, B=B, kernel=h.describe()["kernel"], us_per_step=med, env_steps_per_s=B / med * 1e6)))
env.close()
''' % ROOT


def run(solver, mode, B):
    env = dict(os.environ)
    if mode == "no_flat":
        env["GS_NR_NO_FLAT"] = "1"
    r = subprocess.run([sys.executable, "-c", CHILD, solver, mode, str(B)], capture_output=True, text=True, env=env, timeout=900)
    if r.returncode != 0:
        raise SystemExit(f"{solver}/{mode} failed ({r.returncode}): {r.stderr.strip()[-600:]}")
    line = r.stdout.strip().splitlines()[-1]
    print(line, flush=True)
    return json.loads(line)


def main_loads(B):
    res = {}
    for solver in ("fbs", "nr"):
        for mode in ("shared", "loads", "per_instance", "both"):
            res[(solver, mode)] = run(solver, mode, B)["env_steps_per_s"]
    print(json.dumps(dict(fbs_loads_over_shared=res[("fbs", "loads")] / res[("fbs", "shared")],
                          nr_loads_over_shared=res[("nr", "loads")] / res[("nr", "shared")],
                          fbs_both_over_per_instance=res[("fbs", "both")] / res[("fbs", "per_instance")],
                          nr_both_over_per_instance=res[("nr", "both")] / res[("nr", "per_instance")])), flush=True)


def main():
    args = [a for a in sys.argv[1:] if a != "--loads"]
    B = int(args[0]) if args else 8192
    if "--loads" in sys.argv[1:]:
        return main_loads(B)
    res = {}
    for solver, modes in (("fbs", ("shared", "per_instance")), ("nr", ("shared", "no_flat", "per_instance"))):
        for mode in modes:
            res[(solver, mode)] = run(solver, mode, B)["env_steps_per_s"]
    print(json.dumps(dict(fbs_per_instance_over_shared=res[("fbs", "per_instance")] / res[("fbs", "shared")],
                          nr_per_instance_over_shared=res[("nr", "per_instance")] / res[("nr", "shared")],
                          nr_per_instance_over_no_flat=res[("nr", "per_instance")] / res[("nr", "no_flat")])), flush=True)


if __name__ == "__main__":
    main()
