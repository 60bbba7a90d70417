"""Shared test plumbing: golden loading and FeederSpec <-> oracle EnvSpec conversion."""
import glob
import os

import numpy as np

from oracle import oracle_np as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def golden(name):
    return np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)


def golden_names(prefix):
    return sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, prefix + "*.npz")))


def net_of(d):
    """(n, frm, to, r, x, rating, bus_type, v_set) from a fixture."""
    return (len(d["bus_type"]), d["frm"], d["to"], d["r"], d["x"], d["rating"], d["bus_type"], d["v_set"])


def oracle_spec(fs, **cfg):
    """oracle EnvSpec from a product FeederSpec (tests own this mapping; the product never imports oracle/)."""
    return O.EnvSpec(n=fs.n, frm=fs.frm, to=fs.to, r=fs.r, x=fs.x, rating=fs.rating, bus_type=fs.bus_type,
                     v_set=fs.v_set, load_bus=fs.load_bus, load_base=fs.load_base, load_pf=fs.load_pf,
                     gen_bus=fs.gen_bus, gen_kind=fs.gen_kind, gen_cap=fs.gen_cap, gen_p0=fs.gen_p0,
                     gen_p1=fs.gen_p1, gen_p2=fs.gen_p2, bat_bus=fs.bat_bus, bat_cap=fs.bat_cap,
                     bat_rating=fs.bat_rating, bat_eff=fs.bat_eff, bat_soc0=np.full(fs.n_bats, 0.5), **cfg)


# ---- feeder builders for the step members' limits (tree depth, fan-out, devices per bus, bus numbering) ----

def tree(name, parent, seed=0, drop=0.06, gens=True):
    """Radial feeder from parent[i] (bus i's parent, -1 for the slack at bus 0; parents come first): every line draws its
    impedance around (0.01, 0.02) pu, every bus below the slack a 10-200 kW load, and a solar unit, a wind unit and a
    battery sit at the deepest bus, a wind unit and a battery half way down (gens=False: the deepest bus's battery alone,
    which leaves the sweep's LDS room for the longest chains).  The loads are then scaled so that the linear
    (DistFlow) voltage drop to the worst bus is `drop` pu at nominal load: deep chains stay above ~0.9 pu under any action."""
    from grid_fed_rl_gym_amd.feeders import GEN_SOLAR, GEN_WIND, FeederSpec
    parent = np.asarray(parent, dtype=np.int64)
    n = len(parent)
    assert parent[0] < 0 and all(0 <= parent[i] < i for i in range(1, n))
    rng = np.random.default_rng(seed)
    r = 0.01 * rng.uniform(0.5, 1.5, n - 1); x = 0.02 * rng.uniform(0.5, 1.5, n - 1)
    load = rng.uniform(10e3, 200e3, n - 1); pf = rng.uniform(0.9, 0.98, n - 1)
    depth = np.zeros(n, dtype=np.int64)
    for i in range(1, n):
        depth[i] = depth[parent[i]] + 1
    deep = int(np.argmax(depth)); mid = deep
    while depth[mid] > depth[deep] // 2:
        mid = int(parent[mid])
    mid = max(mid, 1)
    # DistFlow: drop(i) = sum over the lines above i of r * P_below + x * Q_below
    p_below = np.zeros(n); q_below = np.zeros(n)
    p_below[1:] = load; q_below[1:] = load * np.tan(np.arccos(pf))
    for i in range(n - 1, 0, -1):
        p_below[parent[i]] += p_below[i]; q_below[parent[i]] += q_below[i]
    drop_at = np.zeros(n)
    for i in range(1, n):
        drop_at[i] = drop_at[parent[i]] + (r[i - 1] * p_below[i] + x[i - 1] * q_below[i]) / 10e6
    scale = drop / drop_at.max()
    load *= scale
    total = float(load.sum())
    keep_g = slice(None) if gens else slice(0, 0)
    keep_b = slice(None) if gens else slice(0, 1)
    return FeederSpec(
        name=name, bus_ids=list(range(1, n + 1)), bus_type=np.array([2] + [0] * (n - 1), dtype=np.uint8), v_set=np.ones(n),
        frm=parent[1:].astype(np.int32), to=np.arange(1, n, dtype=np.int32), r=r, x=x, rating=np.full(n - 1, 5e6),
        load_bus=np.arange(1, n, dtype=np.int32), load_base=load, load_pf=pf,
        gen_bus=np.array([deep, deep, mid], dtype=np.int32)[keep_g], gen_kind=np.array([GEN_SOLAR, GEN_WIND, GEN_WIND], dtype=np.int32)[keep_g],
        gen_cap=(np.array([0.1, 0.1, 0.05]) * total)[keep_g], gen_p0=np.array([0.2, 3.0, 3.0])[keep_g],
        gen_p1=np.array([0.1 * total / 200.0, 12.0, 12.0])[keep_g], gen_p2=np.array([0.0, 25.0, 25.0])[keep_g],
        bat_bus=np.array([deep, mid], dtype=np.int32)[keep_b], bat_cap=(np.array([0.2, 0.1]) * total)[keep_b],
        bat_rating=(np.array([0.1, 0.05]) * total)[keep_b], bat_eff=np.array([0.92, 0.95])[keep_b])


def chain(n, seed=0, gens=True):
    """n buses in a line: the slack, then depth n - 1."""
    return tree(f"chain{n}", [-1] + list(range(n - 1)), seed=seed, gens=gens)


def star(k, seed=0):
    """The slack, one bus below it, and k children under that bus."""
    return tree(f"star{k}", [-1, 0] + [1] * k, seed=seed)


def broom(depth, fan, seed=0):
    """A chain of `depth` buses below the slack whose last bus has `fan` leaves."""
    return tree(f"broom{depth}x{fan}", [-1] + list(range(depth)) + [depth] * fan, seed=seed)


def relabel(spec, perm, flip):
    """The same feeder with bus i renamed perm[i] and the lines where flip is true reversed (to -> frm)."""
    import dataclasses
    perm = np.asarray(perm, dtype=np.int32); inv = np.argsort(perm)
    flip = np.asarray(flip, dtype=bool)
    frm, to = perm[spec.frm], perm[spec.to]
    return dataclasses.replace(
        spec, name=spec.name + "_relabelled", bus_ids=[spec.bus_ids[i] for i in inv], bus_type=spec.bus_type[inv].copy(),
        v_set=spec.v_set[inv].copy(), frm=np.where(flip, to, frm).astype(np.int32), to=np.where(flip, frm, to).astype(np.int32),
        load_bus=perm[spec.load_bus], gen_bus=perm[spec.gen_bus], bat_bus=perm[spec.bat_bus])


def stack_devices(spec, buses, loads=2, gens=2, bats=2):
    """Fills `buses` up to `loads` loads, `gens` generators and `bats` batteries each.  The new devices copy the feeder's first
    load / generators / battery (a 50 kW load, a solar and a wind unit, a battery where it has none) at 0.5, 0.75 or 1 times
    their size, so that two devices at one bus differ; appended devices get the highest indices."""
    import dataclasses
    f = dataclasses.replace(spec)
    cat = np.concatenate
    ld = (spec.load_base[0], spec.load_pf[0]) if spec.n_loads else (50e3, 0.95)
    gd = [(spec.gen_kind[g], spec.gen_cap[g], spec.gen_p0[g], spec.gen_p1[g], spec.gen_p2[g]) for g in range(min(2, spec.n_gens))] or \
        [(0, 100e3, 0.2, 100e3 / 200.0, 0.0), (1, 100e3, 3.0, 12.0, 25.0)]
    bd = (spec.bat_cap[0], spec.bat_rating[0]) if spec.n_bats else (200e3, 100e3)
    for k, b in enumerate(buses):
        s = 0.5 + 0.25 * (k % 3)
        for _ in range(loads - int(np.sum(f.load_bus == b))):
            f.load_bus = cat([f.load_bus, [b]]); f.load_base = cat([f.load_base, [s * ld[0]]]); f.load_pf = cat([f.load_pf, [0.93]])
        for q in range(gens - int(np.sum(f.gen_bus == b))):
            kind, cap, p0, p1, p2 = gd[q % len(gd)]
            f.gen_bus = cat([f.gen_bus, [b]]); f.gen_kind = cat([f.gen_kind, [kind]]); f.gen_cap = cat([f.gen_cap, [s * cap]])
            f.gen_p0 = cat([f.gen_p0, [p0]]); f.gen_p1 = cat([f.gen_p1, [s * p1 if kind == 0 else p1]]); f.gen_p2 = cat([f.gen_p2, [p2]])
        for _ in range(bats - int(np.sum(f.bat_bus == b))):
            f.bat_bus = cat([f.bat_bus, [b]]); f.bat_cap = cat([f.bat_cap, [s * bd[0]]]); f.bat_rating = cat([f.bat_rating, [s * bd[1]]])
            f.bat_eff = cat([f.bat_eff, [0.9]])
    for k in ("load_bus", "gen_bus", "gen_kind", "bat_bus"):
        setattr(f, k, np.asarray(getattr(f, k), dtype=np.int32))
    for k in ("load_base", "load_pf", "gen_cap", "gen_p0", "gen_p1", "gen_p2", "bat_cap", "bat_rating", "bat_eff"):
        setattr(f, k, np.asarray(getattr(f, k), dtype=np.float64))
    f.name = spec.name + "_stacked"
    return f


def oracle_collect(fs, cfg, actions, seeds, first_instance, policy_seed=None, instance_feeder=None):
    """collect_random_data (algorithms/base.py:268-298) per instance with the oracle: reset, then T steps; where the
    reference calls env.reset() after a finished transition the instance's seed moves one step along its chain.
    instance_feeder(b): the feeder instance b solves (its own line impedances and load powers) where the instances differ.
    "final" holds every instance's (spec, state) where the loop left it, "converged" and "min_voltage" [T, B] what the load flows
    reported."""
    T = actions.shape[0] if actions is not None else cfg.pop("T")
    B = len(seeds)
    out = dict(observations=np.empty((T, B, fs.obs_dim)), actions=np.empty((T, B, fs.action_dim)), rewards=np.empty((T, B)),
               next_observations=np.empty((T, B, fs.obs_dim)), terminals=np.zeros((T, B), dtype=bool), final=[], converged=np.zeros((T, B), dtype=bool),
               min_voltage=np.empty((T, B)))
    spec = oracle_spec(fs, **cfg)
    for b in range(B):
        if instance_feeder is not None:
            spec = oracle_spec(instance_feeder(b), **cfg)
        seed = int(seeds[b])
        obs, st = O.env_reset(spec, seed=seed, instance=first_instance + b)
        for t in range(T):
            a = actions[t, b] if actions is not None else O.rollout_random_actions(policy_seed, first_instance + b, t, fs.action_dim)
            nxt, r, te, tr, inf = O.env_step(spec, st, a)
            out["converged"][t, b] = inf["power_flow_converged"]; out["min_voltage"][t, b] = inf["min_voltage"]
            out["observations"][t, b] = obs; out["actions"][t, b] = a; out["rewards"][t, b] = r
            out["next_observations"][t, b] = nxt; out["terminals"][t, b] = te or tr
            if te or tr:
                seed = O.next_episode_seed(seed, first_instance + b)
                obs, st = O.env_reset(spec, seed=seed, instance=first_instance + b)
            else:
                obs = nxt
        out["final"].append((spec, st))
    return out
