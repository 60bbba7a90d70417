"""The case table of tests/test_gpu_step_matrix.py and the oracle side of its comparisons -- importable without a GPU: one row per
(second-generation step member, form) pair, the names of the kernels a row launches, each row's per-instance data, and the NumPy
oracle runs (environment and post-step checks) the device is held to.  tests/test_step_matrix_static.py checks the table against
the kernels the library holds and against the host-side planner."""
import copy
from collections import namedtuple

import numpy as np

import grid_fed_rl_gym_amd as P
from grid_fed_rl_gym_amd import _lib
from oracle import checks_np as CK
from oracle import oracle_np as O
from tests.helpers import broom, chain, oracle_spec, stack_devices, star, tree

TOL = 1e-9
T0 = 18.0 * 3600.0        # the peak of the daily load profile
# test_gpu_step_limits.py's rule: where the oracle's stopping measure comes within TIE of the tolerance at one of its iterations, a
# kernel may stop one iteration earlier or later than the oracle
TIE = 1e-2

# member: (solver, feeder, batch = one full workgroup and a ragged second one).  The smallest feeders that pin the member: star(8)
# gives fbs_flow2s and nr_flow2s, chain(18) is the first chain fbs_flow2s hands over to fbs_flow2h, chain(130) the first one
# fbs_flow2h hands over to fbs_flow2x, chain(65) fills every bus-group item of nr_flow2, and a 20-bus feeder with 4 loops gives
# nr_mesh2.  The planner accepts every form on the same feeder: test_step_matrix_static.py asks it for every row.
MEMBERS = {
    "fbs_flow2s": ("fbs", "star8", 13),
    "fbs_flow2h": ("fbs", "chain18", 21),
    "fbs_flow2x": ("fbs", "chain130", 21),
    "nr_flow2s": ("nr", "star8", 13),
    "nr_flow2": ("nr", "chain65", 37),
    "nr_mesh2": ("nr", "meshed20", 13),
}
# (nw wavefronts, ni items per sub-group, iw instances per workgroup) of csrc/members.h: the fused checks' bus loop takes
# (64 / iw) * nw buses per pass
SHAPE = {"fbs_flow2s": (2, 1, 8), "fbs_flow2h": (8, 4, 16), "fbs_flow2x": (8, 8, 16), "nr_flow2s": (4, 1, 8), "nr_flow2": (8, 8, 32),
         "nr_mesh2": (4, 10, 8)}
FORMS = {m: ("", "_pz", "_pl", "_pz_pl") if m != "nr_mesh2" else ("", "_pl") for m in MEMBERS}      # (the meshed member has no _pz kernels)


def _twin(levels):
    """Two chains of `levels` buses under the slack: every level holds two buses."""
    return tree(f"twin{levels}", [-1, 0, 0] + list(range(1, 2 * levels - 1)), seed=levels)


FEEDERS = {
    "star8": lambda: star(8), "chain18": lambda: chain(18), "chain130": lambda: chain(130), "chain65": lambda: chain(65),
    "meshed20": lambda: P.random_meshed(20, 4, seed=1),
    # the limit shapes of test_gpu_step_limits.py, and a meshed feeder of ieee123's size
    "chain129": lambda: chain(129), "chain252": lambda: chain(252, gens=False), "twin62": lambda: _twin(62), "broom60x8": lambda: broom(60, 8),
    "star8_stacked": lambda: stack_devices(star(8), [1, 2, 9]), "meshed123": lambda: P.random_meshed(123, 26, seed=5),
}

Row = namedtuple("Row", "member form feeder solver B")
ROWS = [Row(m, form, MEMBERS[m][1], MEMBERS[m][0], MEMBERS[m][2]) for m in MEMBERS for form in FORMS[m]]
# the fused checks on |S| / rating ("solution") as well as on |P| / rating ("environment"): one row per member
SOLUTION_ROWS = [r for r in ROWS if r.form == ""]
# the rollout under GS_POLICY_RANDOM as well as under uploaded actions: one sweep row, one radial Newton-Raphson row, the meshed row
RANDOM_ROWS = [r for r in ROWS if (r.member, r.form) in (("fbs_flow2h", "_pz_pl"), ("nr_flow2", "_pl"), ("nr_mesh2", ""))]

# fused checks at the members' limit shapes: (feeder, solver, member, batch, per-instance line impedances)
LIMIT_ROWS = [("chain129", "fbs", "fbs_flow2h", 19), ("chain252", "fbs", "fbs_flow2x", 19), ("twin62", "nr", "nr_flow2", 35),
              ("broom60x8", "nr", "nr_flow2", 35), ("star8_stacked", "nr", "nr_flow2s", 11), ("star8_stacked", "fbs", "fbs_flow2s", 11),
              ("meshed123", "nr", "nr_mesh2", 11)]
LIMIT_ROWS = [Row(m, form, f, s, B) for f, s, m, B in LIMIT_ROWS
              for form in (("", "_pz") if f in ("chain129", "chain252", "twin62", "broom60x8") else ("",))]


def row_id(row):
    return f"{row.member}{row.form}" if row in ROWS else f"{row.feeder}-{row.member}{row.form}"


def kernel_name(row, fused):
    """gs_k_step + (c with a checks object fused) + _ + describe()["kernel"] + (_pz) + (_pl)"""
    return f"gs_k_step{'c' if fused else ''}_{row.member}{row.form}"


def table_kernel_names():
    return {kernel_name(r, fused) for r in ROWS for fused in (False, True)}


def instance_data(row, fs):
    """(line_impedances (r, x) or None, load_powers or None) of the row's form"""
    rx = P.randomized_line_impedances(fs, row.B, rel=0.1, seed=11) if "_pz" in row.form else None
    pl = P.randomized_load_powers(fs, row.B, low=0.5, high=1.5, seed=4, per_load=True) if "_pl" in row.form else None
    return rx, pl


def env_kwargs(fs, solver, **extra):
    return dict(dict(solver=solver, stochastic_loads=True, weather_variation=True, jacobian="exact", tolerance=TOL, max_iterations=100,
                     power_base=fs.base_power_va), **extra)


def oracle_cfg(fs, solver, **extra):
    return dict(dict(stochastic_loads=True, weather_variation=True, power_base=fs.base_power_va, solver=solver, tolerance=TOL,
                     max_iterations=100, jacobian_mode="exact", zero_z="open"), **extra)


def plan(row):
    """describe() of the row's handle, from the host-side planner"""
    fs = FEEDERS[row.feeder]()
    rx, pl = instance_data(row, fs)
    cfg = _lib.make_config(solver_kind=_lib.SOLVER[row.solver], jacobian_mode=_lib.JACOBIAN["exact"], tolerance=TOL, max_iterations=100,
                           power_base=fs.base_power_va)
    return _lib.plan_describe(fs, cfg, row.B, line_impedances=None if rx is None else _lib.check_line_impedances(fs, rx[0], rx[1], row.B),
                              load_powers=None if pl is None else _lib.check_load_powers(fs, pl, row.B))


def assert_describes(d, row, fused):
    """the launched kernel follows from these describe() fields and from whether a checks object is fused"""
    assert d["kernel"] == row.member, (d["kernel"], d["flow2"], d["mesh2"])
    assert d["per_instance_z"] == int("_pz" in row.form) and d["per_instance_loads"] == int("_pl" in row.form), d
    assert d["instances_per_workgroup"] == SHAPE[row.member][2], d
    return kernel_name(row, fused)


def instance_feeder(fs, b, rx, pl):
    """the feeder instance b solves: its own line impedances and load powers"""
    f = copy.copy(fs)
    if rx is not None:
        f.r, f.x = np.array(rx[0][b], dtype=np.float64), np.array(rx[1][b], dtype=np.float64)
    if pl is not None:
        f.load_base = np.array(pl[b], dtype=np.float64)
    return f


def oracle_instance_steps(fs, f, solver, b, actions_b, seed0=100, require_converged=True, **cfg):
    """Instance b on its own feeder f (instance_feeder) from seed seed0 + b at the load peak through actions_b [T, A]:
    [(obs, reward, terminated, truncated, info, tie, |V| [n], loading [m], frequency) per step]
    tie: the step's stopping measure came within TIE of the tolerance (test_gpu_step_limits.py's _oracle).  cfg: oracle_cfg's
    overrides (max_iterations); require_converged=False leaves an unsolved step to the caller (tests/unsolved_cases.py)."""
    trace = []
    mismatch = O.mismatch

    def measure(*a):
        out = mismatch(*a)
        trace.append(2.0 * (np.sum(np.abs(out[1])) + np.sum(np.abs(out[2]))) if solver == "fbs" else out[3])
        return out
    steps = []
    O.mismatch = measure
    try:
        spec = oracle_spec(f, **oracle_cfg(fs, solver, **cfg))
        _, st = O.env_reset(spec, seed=seed0 + b, instance=b)
        st.time = T0
        for t in range(len(actions_b)):
            trace.clear()
            o, rw, te, tr, inf = O.env_step(spec, st, actions_b[t])
            if require_converged:
                assert inf["power_flow_converged"] and inf["min_voltage"] > 0.9, (b, t, inf["min_voltage"])
            steps.append((o, rw, te, tr, inf, any(abs(q / TOL - 1.0) < TIE for q in trace), st.Vm.copy(), st.loading.copy(), float(st.freq)))
    finally:
        O.mismatch = mismatch
    return steps


def oracle_steps(fs, solver, actions, rx, pl, seed0=100):
    """Every instance on its own lines and loads, from seed seed0 + b at the load peak, through actions [T, B, A]:
    ({b: [(obs, reward, terminated, truncated, info, tie) per step]}, dict(vm [T, B, n], loading [T, B, m], frequency [T, B]))
    tie: the step's stopping measure came within TIE of the tolerance (test_gpu_step_limits.py's _oracle)."""
    T, B = actions.shape[:2]
    ref = {}
    state = dict(vm=np.empty((T, B, fs.n)), loading=np.empty((T, B, fs.m)), frequency=np.empty((T, B)))
    for b in range(B):
        steps = oracle_instance_steps(fs, instance_feeder(fs, b, rx, pl), solver, b, actions[:, b], seed0)
        ref[b] = [s[:6] for s in steps]
        for t, s in enumerate(steps):
            state["vm"][t, b], state["loading"][t, b], state["frequency"][t, b] = s[6], s[7], s[8]
    return ref, state


def against_oracle(got, ref):
    """the bars of test_gpu_step_limits.py, on every instance and step"""
    for b, steps in ref.items():
        for t, (o, rw, te, tr, inf, tie) in enumerate(steps):
            obs, rew, term, trunc, info = got[t]
            rel = np.max(np.abs(obs[b] - o) / np.maximum(1.0, np.abs(o)))
            assert rel < 1e-8, (t, b, rel, int(np.argmax(np.abs(obs[b] - o))))
            assert abs(rew[b] - rw) <= 1e-7 * max(1.0, abs(rw)), (t, b, rew[b], rw)
            assert bool(term[b]) == te and bool(trunc[b]) == tr, (t, b)
            assert bool(info["power_flow_converged"][b]), (t, b)
            assert abs(int(info["iterations"][b]) - int(inf["iterations"])) <= (1 if tie else 0), (t, b, info["iterations"][b], inf["iterations"])
            assert int(info["status"][b]) == int(inf["status"]), (t, b, info["status"][b], inf["status"])
            assert abs(info["total_losses"][b] - inf["total_losses"]) < 1e-8, (t, b)


# ---- the post-step checks ----

def check_limits(state):
    """Limits that cut through the data, from the ORACLE's first step (vm, loading, frequency [T, B, ...] of oracle_steps) and its
    first two steps' rates of change: the keyword dictionaries of PostStepChecks and the matching oracle configurations."""
    vlo, vem, vhi = (float(q) for q in np.quantile(state["vm"][0], [0.2, 0.02, 0.97]))
    llim = float(np.quantile(state["loading"][0], 0.95))
    rate_v = float(np.median(np.max(np.abs(state["vm"][1] - state["vm"][0]), axis=1)))
    rate_f = float(np.median(np.abs(state["frequency"][1] - state["frequency"][0])))
    kw = dict(checker=dict(voltage_limits=(vlo, vhi), line_loading_limit=llim, rate_of_change_limits={"voltage": rate_v, "frequency": rate_f}),
              monitor=dict(voltage_limits=(vlo, vhi), emergency_voltage_limits=(vem, 1.2), line_loading_limit=llim))
    ccfg = CK.CheckerConfig((vlo, vhi), (59.5, 60.5), llim, rate_v, rate_f)
    mcfg = CK.MonitorConfig((vlo, vhi), (59.0, 61.0), llim, (vem, 1.2), (57.0, 63.0))
    return kw, ccfg, mcfg


class ChecksOracle:
    """checks_np's SafetyChecker / SafetyMonitor / quality gate, stateful over the steps"""
    C_KEYS = ("n_voltage_low", "n_voltage_high", "frequency_low", "frequency_high", "n_line_overload", "voltage_rate_violation",
              "frequency_rate_violation", "total", "severity")
    M_KEYS = ("n_voltage_high", "n_voltage_low", "n_voltage_emergency", "frequency_high", "frequency_low", "frequency_emergency",
              "n_line_overload", "total_violations", "emergency_action_required", "consecutive_violations", "emergency_mode")

    def __init__(self, ccfg, mcfg, quality_tolerance=1e-6):
        self.ccfg, self.mcfg, self.qtol = ccfg, mcfg, quality_tolerance
        self.cs, self.ms = CK.CheckerState(), CK.MonitorState()

    def step(self, vm, freq, loading, sol=None):
        """One check of every instance; returns what PostStepChecks.download(masks=True) must hold, under its keys, and `had_prev`:
        the instances whose rate values mean something (a checker without a previous state reports none)."""
        B = vm.shape[0]
        had_prev = np.zeros(B, dtype=bool) if self.cs.has_prev is None else self.cs.has_prev.copy()
        oc = CK.checker_step(self.ccfg, self.cs, vm, freq, loading, 1.0)
        om = CK.monitor_step(self.mcfg, self.ms, vm, freq, loading)
        out = {"c_" + k: np.asarray(oc[k]).astype(np.int64) for k in self.C_KEYS}
        out.update({"m_" + k: np.asarray(om[k]).astype(np.int64) for k in self.M_KEYS})
        em = (vm > self.mcfg.emergency_voltage_limits[1]) | (vm < self.mcfg.emergency_voltage_limits[0])
        out["bus_mask"] = (oc["voltage_low"] * 1 + oc["voltage_high"] * 2 + om["voltage_low"] * 4 + om["voltage_high"] * 8 + em * 16).astype(np.uint8)
        out["line_mask"] = (oc["line_overload"] * 1 + om["line_overload"] * 2).astype(np.uint8)
        out["voltage_rate"], out["frequency_rate"], out["had_prev"] = oc["voltage_rate"], oc["frequency_rate"], had_prev
        if sol is not None:
            out["quality"] = CK.quality(sol["converged"], sol["iterations"], sol["max_mismatch"], sol["bus_voltages"], sol["line_loadings"],
                                        sol["line_flows"], self.qtol)
        return out

    def reset(self, mask):
        """freshly constructed objects for the masked instances"""
        mask = np.asarray(mask, dtype=bool)
        self.cs.has_prev[mask] = False; self.cs.prev_v[mask] = 0.0; self.cs.prev_f[mask] = 0.0
        self.ms.consecutive[mask] = 0; self.ms.emergency_mode[mask] = False


def assert_checks_equal(got, want, where):
    """integers, flags and masks identical; the rate values and the quality score exactly, as test_gpu_checks.py holds them (the
    rates where the checker had a previous state)"""
    for k, v in want.items():
        if k in ("had_prev", "voltage_rate", "frequency_rate", "quality"):
            continue
        np.testing.assert_array_equal(np.asarray(got[k]).astype(np.int64), np.asarray(v).astype(np.int64), err_msg=f"{k} {where}")
    hp = want["had_prev"]
    np.testing.assert_array_equal(got["voltage_rate"][hp], want["voltage_rate"][hp], err_msg=f"voltage_rate {where}")
    np.testing.assert_array_equal(got["frequency_rate"][hp], want["frequency_rate"][hp], err_msg=f"frequency_rate {where}")
    if "quality" in want:
        np.testing.assert_array_equal(got["quality"], want["quality"], err_msg=f"quality {where}")


def checks_cut_through(seq, steps):
    """the conditions without which a checks comparison is empty, over the per-step results `seq` (download()s, or the oracle's)"""
    assert max(int(np.max(s["c_total"])) for s in seq) > 0
    assert any(np.any(s["c_voltage_rate_violation"]) for s in seq)
    assert max(int(np.max(s["m_consecutive_violations"])) for s in seq) == steps
    for k in ("bus_mask", "line_mask"):
        assert any(np.any(s[k] != 0) for s in seq) and any(np.any(s[k] == 0) for s in seq), k
