"""GPU: per-instance line impedances on the second-generation radial step members -- every instance against the NumPy oracle on
its own line data, bit-identity with the shared handle at nominal values, masked updates, rollouts, the linear fallback, loopback
shards and the calls a per-instance handle refuses."""
import copy
import os

import numpy as np
import pytest

import grid_fed_rl_gym_amd as P
from grid_fed_rl_gym_amd import _lib
from oracle import fallback_np as FB
from oracle import oracle_np as O
from tests.helpers import oracle_spec

pytestmark = pytest.mark.gpu

FEEDERS = {"ieee13": lambda: P.ieee13_like("epsilon"), "ieee123": P.ieee123_like, "wide": lambda: P.random_meshed(200, 0, seed=5)}
MEMBERS = [("ieee13", "fbs", "fbs_flow2s"), ("ieee13", "nr", "nr_flow2s"), ("ieee123", "fbs", "fbs_flow2h"),
           ("ieee123", "nr", "nr_flow2"), ("wide", "fbs", "fbs_flow2x")]
TOL = 1e-9


def _kw(fs, solver):
    return dict(solver=solver, stochastic_loads=True, weather_variation=True, jacobian="exact", tolerance=TOL,
                max_iterations=100 if solver == "fbs" else 50, power_base=fs.base_power_va)


def _spec(fs, solver, r=None, x=None):
    f = copy.copy(fs)
    if r is not None:
        f.r, f.x = np.array(r, dtype=np.float64), np.array(x, dtype=np.float64)
    return oracle_spec(f, stochastic_loads=True, weather_variation=True, power_base=fs.base_power_va, solver=solver, tolerance=TOL,
                       max_iterations=100 if solver == "fbs" else 50, jacobian_mode="exact", zero_z="open")


def _oracle_steps(fs, solver, r, x, seeds, actions, instances):
    """per instance b of `instances`: the oracle's (obs, reward, terminated, truncated, info) of every step"""
    out = {}
    for b in instances:
        spec = _spec(fs, solver, r[b], x[b])
        _, st = O.env_reset(spec, seed=int(seeds[b]), instance=int(b))
        out[b] = [O.env_step(spec, st, a[b]) for a in actions]
    return out


def _check_against_oracle(got, ref, instances):
    for b in instances:
        for k, (o, rw, te, tr, inf) in enumerate(ref[b]):
            g_obs, g_rew, g_te, g_tr, g_inf = got[k]
            rel = np.max(np.abs(o - g_obs[b]) / np.maximum(1.0, np.abs(o)))
            assert rel < 1e-8, (b, k, rel)
            assert abs(rw - g_rew[b]) <= 1e-8 * max(1.0, abs(rw)), (b, k, rw, g_rew[b])
            assert bool(te) == bool(g_te[b]) and bool(tr) == bool(g_tr[b]), (b, k)
            assert bool(inf["power_flow_converged"]) == bool(g_inf["power_flow_converged"][b]), (b, k)
            assert int(inf["iterations"]) == int(g_inf["iterations"][b]), (b, k, inf["iterations"], g_inf["iterations"][b])
            assert abs(inf["total_losses"] - g_inf["total_losses"][b]) <= 1e-8 * max(1.0, abs(inf["total_losses"])), (b, k)


def _run(env, seeds, actions):
    env.reset(seed=seeds)
    return [tuple(copy.deepcopy(v) for v in env.step(a)) for a in actions]


@pytest.mark.parametrize("feeder,solver,member", MEMBERS)
def test_every_instance_matches_the_oracle_on_its_own_lines(feeder, solver, member):
    fs = FEEDERS[feeder]()
    B = 37
    r, x = P.randomized_line_impedances(fs, B, rel=0.1, seed=11)
    env = P.BatchedGridEnvironment(fs, num_envs=B, line_impedances=(r, x), **_kw(fs, solver))
    d = env.handle.describe()
    assert d["kernel"] == member and d["per_instance_z"] == 1 and d["nr_flat_start_table"] == 0
    rng = np.random.default_rng(5)
    seeds = np.arange(B, dtype=np.uint64) + 3
    actions = [rng.uniform(-1, 1, (B, env.action_dim)) for _ in range(3)]
    got = _run(env, seeds, actions)
    gr, gx = env.line_impedances
    assert np.array_equal(gr, r) and np.array_equal(gx, x)
    env.close()
    _check_against_oracle(got, _oracle_steps(fs, solver, r, x, seeds, actions, range(B)), range(B))


@pytest.mark.parametrize("feeder,solver", [("ieee123", "fbs"), ("ieee13", "nr")])
def test_wide_spread_gives_each_instance_its_own_iteration_count(feeder, solver):
    fs = FEEDERS[feeder]()
    B = 66
    rng = np.random.default_rng(17)
    r = fs.r[None, :] * rng.uniform(0.5, 2.0, (B, fs.m)); x = fs.x[None, :] * rng.uniform(0.5, 2.0, (B, fs.m))
    zero = ~(np.hypot(fs.r, fs.x) > 1e-12)
    r[:, zero] = fs.r[zero]; x[:, zero] = fs.x[zero]
    env = P.BatchedGridEnvironment(fs, num_envs=B, line_impedances=(r, x), **_kw(fs, solver))
    seeds = np.arange(B, dtype=np.uint64) + 1
    actions = [rng.uniform(-1, 1, (B, env.action_dim)) for _ in range(2)]
    got = _run(env, seeds, actions)
    env.close()
    ref = _oracle_steps(fs, solver, r, x, seeds, actions, range(B))
    _check_against_oracle(got, ref, range(B))
    assert len({int(ref[b][0][4]["iterations"]) for b in range(B)}) > 1


def _same(u, v):
    if isinstance(u, dict):
        return u.keys() == v.keys() and all(_same(u[q], v[q]) for q in u)
    if isinstance(u, (list, tuple)):
        return len(u) == len(v) and all(_same(p, q) for p, q in zip(u, v))
    return np.array_equal(np.asarray(u), np.asarray(v))


def _equal_runs(a, b):
    for (o1, r1, t1, u1, i1), (o2, r2, t2, u2, i2) in zip(a, b):
        assert np.array_equal(o1, o2) and np.array_equal(r1, r2) and np.array_equal(t1, t2) and np.array_equal(u1, u2)
        for q in i1:
            assert _same(i1[q], i2[q]), q


@pytest.mark.parametrize("feeder,solver", [("ieee123", "fbs"), ("ieee13", "fbs"), ("ieee123", "nr"), ("ieee13", "nr")])
def test_nominal_instances_are_bit_identical_to_the_shared_handle(feeder, solver, monkeypatch):
    fs = FEEDERS[feeder]()
    B = 37
    r = np.tile(fs.r, (B, 1)); x = np.tile(fs.x, (B, 1))
    rng = np.random.default_rng(2)
    seeds = np.arange(B, dtype=np.uint64) + 9
    actions = [rng.uniform(-1, 1, (B, fs.n_bats + fs.n_gens)) for _ in range(3)]
    pz = P.BatchedGridEnvironment(fs, num_envs=B, line_impedances=(r, x), **_kw(fs, solver))
    got = _run(pz, seeds, actions)
    pz.close()
    if solver == "nr":      # the per-instance handle eliminates iteration 0 itself, as a shared handle does under GS_NR_NO_FLAT
        monkeypatch.setenv("GS_NR_NO_FLAT", "1")
    shared = P.BatchedGridEnvironment(fs, num_envs=B, **_kw(fs, solver))
    assert shared.handle.describe()["per_instance_z"] == 0
    ref = _run(shared, seeds, actions)
    shared.close()
    _equal_runs(got, ref)


def test_masked_updates_persist_and_rollouts_match_the_step_loop():
    fs = P.ieee123_like(); solver = "fbs"
    B = 66
    r0, x0 = P.randomized_line_impedances(fs, B, rel=0.1, seed=1)
    r1, x1 = P.randomized_line_impedances(fs, B, rel=0.1, seed=2)
    mask = np.zeros(B, dtype=bool); mask[::3] = True
    rng = np.random.default_rng(3)
    seeds = np.arange(B, dtype=np.uint64) + 5
    actions = [rng.uniform(-1, 1, (B, fs.n_bats + fs.n_gens)) for _ in range(4)]
    kw = _kw(fs, solver)

    a = P.BatchedGridEnvironment(fs, num_envs=B, line_impedances=(r0, x0), **kw)
    a.reset(seed=seeds)
    first = [a.step(actions[0])]
    a.set_line_impedances(r1, x1, mask=mask)
    er, ex = np.where(mask[:, None], r1, r0), np.where(mask[:, None], x1, x0)
    gr, gx = a.line_impedances
    assert np.array_equal(gr, er) and np.array_equal(gx, ex)
    later = [tuple(copy.deepcopy(v) for v in a.step(act)) for act in actions[1:]]
    # unmasked instances: bit-identical to a run without the update
    b = P.BatchedGridEnvironment(fs, num_envs=B, line_impedances=(r0, x0), **kw)
    ref_b = _run(b, seeds, actions)
    for k, got in enumerate(later):
        for i in np.flatnonzero(~mask):
            assert np.array_equal(got[0][i], ref_b[k + 1][0][i]) and got[1][i] == ref_b[k + 1][1][i], (k, i)
    # masked instances: the oracle with their new values from step 1 on
    for bi in np.flatnonzero(mask)[:8]:
        spec0, spec1 = _spec(fs, solver, r0[bi], x0[bi]), _spec(fs, solver, r1[bi], x1[bi])
        _, st = O.env_reset(spec0, seed=int(seeds[bi]), instance=int(bi))
        O.env_step(spec0, st, actions[0][bi])
        for k in range(1, 4):
            o, rw, te, tr, inf = O.env_step(spec1, st, actions[k][bi])
            assert np.max(np.abs(o - later[k - 1][0][bi]) / np.maximum(1.0, np.abs(o))) < 1e-8, (bi, k)
            assert int(inf["iterations"]) == int(later[k - 1][4]["iterations"][bi])
    # reset and set_state leave the values alone
    st = a.get_state()
    a.reset(seed=seeds)
    a.set_state(st)
    gr, gx = a.line_impedances
    assert np.array_equal(gr, er) and np.array_equal(gx, ex)
    # a device rollout on the per-instance handle equals the step-by-step loop (episodes of 6 steps: compared up to the first
    # in-place reset), and -- at nominal values -- the shared handle's rollout bit for bit through the in-place resets (T = 16)
    T = 16
    acts = rng.uniform(-1, 1, (T, B, fs.n_bats + fs.n_gens))
    c = P.BatchedGridEnvironment(fs, num_envs=B, line_impedances=(er, ex), episode_length=6, **kw)
    c.reset(seed=seeds)
    c.handle.rollout(T, "uploaded", actions=acts)
    ro = c.handle.rollout_download(("observations", "rewards", "next_observations", "terminals"))
    d = P.BatchedGridEnvironment(fs, num_envs=B, line_impedances=(er, ex), episode_length=6, **kw)
    obs, _ = d.reset(seed=seeds)
    for t in range(5):
        assert np.array_equal(ro["observations"][t], obs), t
        o2, rw, te, tr, _ = d.step(acts[t])
        assert np.array_equal(ro["rewards"][t], rw) and np.array_equal(ro["next_observations"][t], o2), t
        obs = np.array(o2, copy=True)
    outs = []
    for li in ((np.tile(fs.r, (B, 1)), np.tile(fs.x, (B, 1))), None):
        e = P.BatchedGridEnvironment(fs, num_envs=B, line_impedances=li, episode_length=6, **kw)
        e.reset(seed=seeds)
        e.handle.rollout(T, "uploaded", actions=acts)
        outs.append(e.handle.rollout_download(("observations", "rewards", "next_observations", "terminals")))
        e.close()
    assert outs[0]["n_terminal"] > 0
    for q in ("observations", "rewards", "next_observations", "terminals"):
        assert np.array_equal(outs[0][q], outs[1][q]), q
    for e in (a, b, c, d):
        e.close()


def test_linear_fallback_reads_each_instances_reactances():
    fs = P.ieee13_like("epsilon")
    B = 9
    r, x = P.randomized_line_impedances(fs, B, rel=0.3, seed=4)
    env = P.BatchedGridEnvironment(fs, num_envs=B, line_impedances=(r, x), **_kw(fs, "nr"))
    env.reset(seed=np.arange(B, dtype=np.uint64))
    rng = np.random.default_rng(6)
    n = fs.n
    loads = rng.uniform(0.0, 2e5, (B, n)); gens = rng.uniform(0.0, 1e5, (B, n))
    applied = env.handle.fallback_linear(load_w=loads, gen_w=gens, mask=np.ones(B, dtype=np.uint8))
    assert applied.all()
    sol = env.last_solution()
    is_slack = fs.bus_type == 2
    for b in range(B):
        tl = 0.0; tg = 0.0
        for i in range(n): tl += loads[b, i]; tg += gens[b, i]
        lin = FB.linear_approximation(is_slack, loads[b], gens[b], tl, tg, fs.frm, fs.to, x[b], fs.rating)
        assert np.array_equal(sol["bus_angles"][b], lin["bus_angles"]), b
        assert np.array_equal(sol["bus_voltages"][b], lin["bus_voltages"]), b
    env.close()


def test_loopback_shards_equal_one_environment():
    fs = P.ieee13_like("epsilon"); solver = "fbs"
    B = 2 * 40
    r, x = P.randomized_line_impedances(fs, B, rel=0.1, seed=9)
    kw = _kw(fs, solver)
    lb = P.LoopbackShards(fs, B, 2, line_impedances=(r, x), **kw)
    one = P.ShardedGridEnvironment(fs, B, 0, 1, line_impedances=(r, x), **kw)
    lb.reset(seed=4); one.reset(seed=4)
    rng = np.random.default_rng(1)
    for _ in range(3):
        a = rng.uniform(-1, 1, (B, fs.n_bats + fs.n_gens))
        parts = lb.step(a)
        whole = one.step(a)
        assert np.array_equal(np.concatenate([p[0] for p in parts]), whole[0])
        assert np.array_equal(np.concatenate([p[1] for p in parts]), whole[1])
        assert np.array_equal(np.concatenate([p[4]["iterations"] for p in parts]), whole[4]["iterations"])
    lb.close(); one.env.close()


def test_refused_calls_leave_later_steps_alone():
    fs = P.ieee13_like("epsilon")
    B = 16
    r, x = P.randomized_line_impedances(fs, B, rel=0.1, seed=2)
    rng = np.random.default_rng(8)
    seeds = np.arange(B, dtype=np.uint64)
    actions = [rng.uniform(-1, 1, (B, fs.n_bats + fs.n_gens)) for _ in range(2)]
    env = P.BatchedGridEnvironment(fs, num_envs=B, line_impedances=(r, x), **_kw(fs, "fbs"))
    ref = _run(env, seeds, actions)
    env.reset(seed=seeds)
    with pytest.raises(P.PowerFlowError, match=r"-5.*per-instance line impedances"):
        env.handle.solve(np.zeros((B, fs.n)))
    got = [tuple(copy.deepcopy(v) for v in env.step(a)) for a in actions]
    _equal_runs(got, ref)
    env.close()
    shared = P.BatchedGridEnvironment(fs, num_envs=B, **_kw(fs, "fbs"))
    ref = _run(shared, seeds, actions)
    shared.reset(seed=seeds)
    with pytest.raises(P.PowerFlowError, match=r"-5.*without per-instance"):
        shared.set_line_impedances(r, x)
    got = [tuple(copy.deepcopy(v) for v in shared.step(a)) for a in actions]
    _equal_runs(got, ref)
    shared.close()


def test_full_size_123_bus_8192_instances():
    fs = P.ieee123_like(); solver = "fbs"
    B = 8192
    r, x = P.randomized_line_impedances(fs, B, rel=0.1, seed=21)
    env = P.BatchedGridEnvironment(fs, num_envs=B, line_impedances=(r, x), **_kw(fs, solver))
    assert env.handle.describe()["kernel"] == "fbs_flow2h"
    rng = np.random.default_rng(4)
    seeds = np.arange(B, dtype=np.uint64) + 2
    actions = [rng.uniform(-1, 1, (B, env.action_dim))]
    got = _run(env, seeds, actions)
    env.close()
    assert got[0][4]["power_flow_converged"].all()
    picks = np.linspace(0, B - 1, 16).astype(int)
    _check_against_oracle(got, _oracle_steps(fs, solver, r, x, seeds, actions, picks), picks)


@pytest.mark.parametrize("solver", ["fbs", "nr"])
def test_full_size_nominal_instances_are_bit_identical_to_the_shared_handle(solver, monkeypatch):
    """Every one of 8192 instances, not a sample: gs_create zeroes and uploads the per-instance entries and derives them
    (gs_k_line_params) on the handle's stream, and an entry lost to an unordered copy or memset shows in some instances only."""
    fs = P.ieee123_like()
    B = 8192
    r = np.tile(fs.r, (B, 1)); x = np.tile(fs.x, (B, 1))
    rng = np.random.default_rng(6)
    seeds = np.arange(B, dtype=np.uint64) + 4
    actions = [rng.uniform(-1, 1, (B, fs.n_bats + fs.n_gens)) for _ in range(2)]
    pz = P.BatchedGridEnvironment(fs, num_envs=B, line_impedances=(r, x), **_kw(fs, solver))
    got = _run(pz, seeds, actions)
    pz.close()
    if solver == "nr":
        monkeypatch.setenv("GS_NR_NO_FLAT", "1")
    shared = P.BatchedGridEnvironment(fs, num_envs=B, **_kw(fs, solver))
    ref = _run(shared, seeds, actions)
    shared.close()
    assert got[0][4]["power_flow_converged"].all()
    _equal_runs(got, ref)
