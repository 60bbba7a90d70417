"""GPU: the epilogue of the second-generation step kernels (kernels_flow2.hip, f2_step behind the solver's last barrier) at the
line counts where its line phase changes shape, and wave 0's tail in both of its forms.  A member takes (64 / iw) * nw lines per
pass of the line phase, fbs_flow2h 32; the tail of the sweep members fbs_flow2h / fbs_flow2x (forms without the checks) reads
its generator / battery operands four at a time and spreads their observation columns over the sub-groups, every other kernel
keeps the plain loops:

* 1 line (the smallest feeder), 31 / 32 / 33 lines: the last pass empty, full, and a single line;
* a 140-bus feeder on the wide member fbs_flow2x: five passes;
* the 13-bus feeder through fbs_flow2s and nr_flow2s;
* the 33-line feeder with eleven generators and ten batteries (three batches of the tail's operands), sweeps and Newton-Raphson;
* the per-instance line impedance (_pz) and load power (_pl) forms and the fused checks (gs_k_stepc_*) on the 33-line feeder;
* a 12-step rollout with actions drawn on the device across two episode boundaries on the 33-line feeder: the reward / done
  arrays wave 0's tail writes, against the oracle's collection loop.

Every case: B = 70 (one 64-instance slab group and a partial one), 3 steps against the NumPy environment oracle at the bars of
tests/test_gpu_env.py (every third instance and the whole partial group), every instance converged, and bit for bit the same
handle built with GS_EAGER_ROWS=1 (the step then also writes the row pairs the line and bus phases produce)."""
import copy

import numpy as np
import pytest

import grid_fed_rl_gym_amd as P
from grid_fed_rl_gym_amd.safety import PostStepChecks
from tests import step_matrix as M
from tests.helpers import oracle_collect, stack_devices, tree

pytestmark = pytest.mark.gpu

B, T = 70, 3
CHECKED = sorted(set(range(0, B, 3)) | set(range(64, B)))      # the oracle's share: every third instance, and the partial slab group


def radial(m, seed, gens=True):
    """Random radial feeder with m lines: bus i hangs below a bus drawn from the ones before it (tests.helpers.tree; gens=False:
    one battery and no generator -- with two buses the full set would put three generators at the one bus below the slack, and
    the second-generation members take two devices of a kind per bus)."""
    rng = np.random.default_rng(seed)
    return tree(f"radial{m}", [-1] + [int(rng.integers(0, i)) for i in range(1, m + 1)], seed=seed, gens=gens)


FEEDERS = {
    "radial1": lambda: radial(1, 3, gens=False), "radial31": lambda: radial(31, 3), "radial32": lambda: radial(32, 3), "radial33": lambda: radial(33, 3),
    "radial139": lambda: radial(139, 3), "ieee13": lambda: P.ieee13_like("epsilon"),
    # two generators and two batteries at each of four more buses: more than two batches of the tail's operands
    "radial33_stacked": lambda: stack_devices(radial(33, 3), [5, 12, 20, 27]),
}
# (feeder, solver, member, form)
CASES = [
    ("radial1", "fbs", "fbs_flow2s", ""), ("radial31", "fbs", "fbs_flow2h", ""), ("radial32", "fbs", "fbs_flow2h", ""),
    ("radial33", "fbs", "fbs_flow2h", ""), ("radial139", "fbs", "fbs_flow2x", ""), ("ieee13", "fbs", "fbs_flow2s", ""),
    ("ieee13", "nr", "nr_flow2s", ""), ("radial33", "fbs", "fbs_flow2h", "_pz"), ("radial33", "fbs", "fbs_flow2h", "_pl"),
    ("radial33_stacked", "fbs", "fbs_flow2h", ""), ("radial33_stacked", "nr", "nr_flow2", ""),
]


def instance_data(fs, form):
    return M.instance_data(M.Row("", form, "", "", B), fs)


def oracle_share(fs, solver, actions, rx, pl):
    """the oracle on the CHECKED instances: ({b: [(obs, reward, terminated, truncated, info, tie) per step]}, check_limits' state)"""
    ref = {}
    state = dict(vm=np.empty((T, len(CHECKED), fs.n)), loading=np.empty((T, len(CHECKED), fs.m)), frequency=np.empty((T, len(CHECKED))))
    for q, b in enumerate(CHECKED):
        steps = M.oracle_instance_steps(fs, M.instance_feeder(fs, b, rx, pl), solver, b, actions[:, b], require_converged=False)
        assert all(s[4]["power_flow_converged"] for s in steps), b
        ref[b] = [s[:6] for s in steps]
        for t, s in enumerate(steps):
            state["vm"][t, q], state["loading"][t, q], state["frequency"][t, q] = s[6], s[7], s[8]
    return ref, state


def make_envs(fs, solver, rx, pl, monkeypatch, n_lean=1, **extra):
    """n_lean handles as built by default and one with GS_EAGER_ROWS=1"""
    kw = dict(num_envs=B, line_impedances=rx, load_powers=pl, **M.env_kwargs(fs, solver, **extra))
    lean = [P.BatchedGridEnvironment(fs, **kw) for _ in range(n_lean)]
    monkeypatch.setenv("GS_EAGER_ROWS", "1")
    eager = P.BatchedGridEnvironment(fs, **kw)
    monkeypatch.delenv("GS_EAGER_ROWS")
    return lean, eager


def start(env):
    env.reset(seed=np.arange(100, 100 + B, dtype=np.uint64))
    st = env.get_state()
    st[:, env.state_column("time")] = M.T0
    env.set_state(st)


def same(u, v):
    if isinstance(u, dict):
        return u.keys() == v.keys() and all(same(u[q], v[q]) for q in u)
    return np.array_equal(np.asarray(u), np.asarray(v))


def assert_steps_equal(a, b, where):
    for k, (u, v) in enumerate(zip(a[:4], b[:4])):      # observation, reward, terminated, truncated
        assert np.array_equal(u, v), (where, k)
    assert same(a[4], b[4]), where                      # every info array


@pytest.mark.parametrize("feeder,solver,member,form", CASES, ids=[f"{c[0]}-{c[2]}{c[3]}" for c in CASES])
def test_epilogue_meets_the_oracle_and_the_eager_rows(feeder, solver, member, form, monkeypatch):
    fs = FEEDERS[feeder]()
    rx, pl = instance_data(fs, form)
    actions = np.random.default_rng(B * 7 + fs.n).uniform(-1, 1, (T, B, fs.action_dim))
    ref, _ = oracle_share(fs, solver, actions, rx, pl)
    (lean,), eager = make_envs(fs, solver, rx, pl, monkeypatch)
    for env in (lean, eager):
        d = env.handle.describe()
        assert d["kernel"] == member, d["kernel"]
        assert d["per_instance_z"] == int("_pz" in form) and d["per_instance_loads"] == int("_pl" in form), d
        start(env)
    nw, ni, iw = M.SHAPE[member]
    if member == "fbs_flow2x":                           # more passes of the line phase than the default member ever takes
        assert -(-fs.m // ((64 // iw) * nw)) > 4
    got = []
    for t in range(T):
        a = tuple(copy.deepcopy(v) for v in lean.step(actions[t]))
        b = tuple(copy.deepcopy(v) for v in eager.step(actions[t]))
        assert_steps_equal(a, b, t)
        assert a[4]["power_flow_converged"].all(), t
        got.append(a)
    assert np.array_equal(lean.get_state(), eager.get_state())        # (the lean handle restores the row pairs on demand)
    assert same(lean.last_solution(), eager.last_solution())
    M.against_oracle(got, ref)
    lean.close(); eager.close()


def test_fused_checks_form_on_the_33_line_feeder(monkeypatch):
    """gs_k_stepc_fbs_flow2h: bit for bit the step kernel and the eager handle, the oracle, and the checks against checks_np"""
    fs = FEEDERS["radial33"]()
    actions = np.random.default_rng(B * 7 + fs.n).uniform(-1, 1, (T, B, fs.action_dim))
    ref, state = oracle_share(fs, "fbs", actions, None, None)
    kw, ccfg, mcfg = M.check_limits(state)
    (plain, fused), eager = make_envs(fs, "fbs", None, None, monkeypatch, n_lean=2)
    ck = PostStepChecks(fused, loading="environment", fused=True, fused_masks=True, **kw)
    row = M.Row("fbs_flow2h", "", "radial33", "fbs", B)
    assert M.assert_describes(plain.handle.describe(), row, False) == "gs_k_step_fbs_flow2h"
    assert M.assert_describes(fused.handle.describe(), row, True) == "gs_k_stepc_fbs_flow2h"
    for env in (plain, fused, eager):
        start(env)
    lay = fused.state_layout()
    oracle = M.ChecksOracle(ccfg, mcfg)
    got, downs = [], []
    for t in range(T):
        a = tuple(copy.deepcopy(v) for v in plain.step(actions[t]))
        b = tuple(copy.deepcopy(v) for v in fused.step(actions[t]))
        c = tuple(copy.deepcopy(v) for v in eager.step(actions[t]))
        assert_steps_equal(a, b, ("fused", t)); assert_steps_equal(a, c, ("eager", t))
        assert b[4]["power_flow_converged"].all(), t
        got.append(b)
        down = {k: np.array(v, copy=True) for k, v in ck.download(masks=True).items()}
        st = fused.get_state()
        M.assert_checks_equal(down, oracle.step(st[:, lay["vm"]], st[:, lay["frequency"]], st[:, lay["line_loading"]], fused.last_solution()), f"t={t}")
        downs.append(down)
    M.against_oracle(got, ref)
    for k in ("bus_mask", "line_mask"):                  # the limits cut through the data
        assert any(np.any(s[k] != 0) for s in downs) and any(np.any(s[k] == 0) for s in downs), k
    ck.close(); plain.close(); fused.close(); eager.close()


def test_rollout_rewards_and_done_flags_across_resets_on_the_33_line_feeder(monkeypatch):
    """gs_rollout, 12 steps, actions drawn on the device, episodes of 5 steps: two in-kernel resets per instance"""
    fs = FEEDERS["radial33"]()
    R, first = 12, 2000
    (lean,), eager = make_envs(fs, "fbs", None, None, monkeypatch, episode_length=5, first_instance=first)
    assert lean.handle.describe()["kernel"] == "fbs_flow2h"
    data = P.collect_random_data(lean, R, seed=21)
    n_terminal = lean.handle.rollout_device_view().n_terminal
    data_e = P.collect_random_data(eager, R, seed=21)
    for k in ("observations", "actions", "rewards", "next_observations", "terminals"):
        assert np.array_equal(data[k], data_e[k]), k
    cfg = M.oracle_cfg(fs, "fbs", episode_length=5)
    cfg["T"] = R
    ref = oracle_collect(fs, cfg, None, np.uint64(21) + np.arange(B, dtype=np.uint64), first, policy_seed=21)
    assert ref["converged"].all()
    term = data["terminals"].reshape(R, B)
    assert np.array_equal(term, ref["terminals"]) and term[4].all() and term[9].all() and term.sum() == 2 * B and n_terminal == 2 * B
    assert np.allclose(data["actions"].reshape(R, B, -1), ref["actions"], rtol=0, atol=1e-15)
    for k in ("observations", "next_observations"):
        g, want = data[k].reshape(R, B, -1), ref[k]
        err = np.abs(g - want) / np.maximum(1.0, np.abs(want))
        assert err.max() < 1e-8, (k, np.unravel_index(np.argmax(err), err.shape), err.max())
    assert np.max(np.abs(data["rewards"].reshape(R, B) - ref["rewards"]) / np.maximum(1.0, np.abs(ref["rewards"]))) < 1e-7
    lean.close(); eager.close()
