"""CPU-only: per-instance line impedances -- which step member a handle carrying them is planned on (gs_plan_describe), which
configurations are rejected, the Python validation and the randomisation helper."""
import numpy as np
import pytest

import grid_fed_rl_gym_amd as P
from grid_fed_rl_gym_amd import _lib

PREFIX = "per-instance line impedances need a second-generation radial step member: "


def _cfg(solver, **kw):
    kw.setdefault("jacobian_mode", _lib.JACOBIAN["exact"])
    kw.setdefault("tolerance", 1e-9)
    return _lib.make_config(solver_kind=_lib.SOLVER[solver], **kw)


@pytest.mark.parametrize("feeder,solver,member", [
    ("ieee13", "fbs", "fbs_flow2s"), ("ieee13", "nr", "nr_flow2s"),
    ("ieee123", "fbs", "fbs_flow2h"), ("ieee123", "nr", "nr_flow2"),
    ("wide", "fbs", "fbs_flow2x"),
])
def test_plan_takes_the_per_instance_member(feeder, solver, member):
    fs = {"ieee13": lambda: P.ieee13_like("epsilon"), "ieee123": P.ieee123_like, "wide": lambda: P.random_meshed(200, 0, seed=5)}[feeder]()
    B = 37
    r, x = P.randomized_line_impedances(fs, B, rel=0.1, seed=3)
    d = _lib.plan_describe(fs, _cfg(solver), B, line_impedances=(r, x))
    assert d["kernel"] == member and d["per_instance_z"] == 1 and d["nr_flat_start_table"] == 0
    shared = _lib.plan_describe(fs, _cfg(solver), B)
    assert shared["kernel"] == member and shared["per_instance_z"] == 0
    assert shared["nr_flat_start_table"] == (1 if solver == "nr" else 0)


def _rejected(fs, cfg, B=8):
    r, x = P.randomized_line_impedances(fs, B, rel=0.1, seed=1)
    with pytest.raises(P.PowerFlowError) as e:
        _lib.plan_describe(fs, cfg, B, line_impedances=(r, x))
    assert PREFIX in str(e.value) and "(-4)" in str(e.value), str(e.value)
    return str(e.value)


def test_plan_rejects_a_meshed_feeder():
    _rejected(P.random_meshed(40, 6, seed=2), _cfg("nr"))


def test_plan_rejects_a_pv_bus():
    fs = P.ieee13_like("epsilon")
    bt = np.array(fs.bus_type, copy=True)
    bt[5] = 1
    fs.bus_type = bt
    _rejected(fs, _cfg("nr"))


def test_plan_rejects_warm_start():
    assert "warm start" in _rejected(P.ieee123_like(), _cfg("fbs", fbs_warm_start=1))


def test_plan_rejects_the_as_coded_jacobian():
    assert "as-coded Jacobian" in _rejected(P.ieee13_like("epsilon"), _cfg("nr", jacobian_mode=_lib.JACOBIAN["as_coded"]))


def test_plan_rejects_one_array_alone():
    fs = P.ieee13_like("epsilon")
    r, x = P.randomized_line_impedances(fs, 4)
    t, keep = _lib._topology_of(fs, (r, x))
    t.line_x_inst = None
    import ctypes
    buf = ctypes.create_string_buffer(4096)
    lib = _lib.load()
    assert lib.gs_plan_describe(ctypes.byref(t), ctypes.byref(_cfg("fbs")), 4, 256, buf, 4096) == _lib.GS_E_INVALID
    assert b"go together" in lib.gs_last_error(None)


def _with_zero_line():
    """ieee13_like with its last line at zero impedance (the reference's zero-length switch, treated as open)"""
    fs = P.ieee13_like("epsilon")
    fs.r = np.array(fs.r, copy=True); fs.x = np.array(fs.x, copy=True)
    fs.r[-1] = 0.0; fs.x[-1] = 0.0
    return fs, fs.m - 1, 0


@pytest.mark.parametrize("case", ["shape", "nan", "negative_r", "zeroed_line", "changed_zero_line"])
def test_python_validation_raises_value_error(case):
    fs, kz, knz = _with_zero_line()
    B = 5
    r, x = P.randomized_line_impedances(fs, B, seed=2)
    if case == "shape":
        r = r[:, :-1]
    elif case == "nan":
        x[2, knz] = np.nan
    elif case == "negative_r":
        r[1, knz] = -1e-3
    elif case == "zeroed_line":
        r[3, knz] = 0.0; x[3, knz] = 0.0
    elif case == "changed_zero_line":
        r[0, kz] = 1e-3
    with pytest.raises(ValueError):
        _lib.check_line_impedances(fs, r, x, B)
    # the environment checks before it creates a handle (no device needed to get there)
    with pytest.raises(ValueError):
        P.BatchedGridEnvironment(fs, num_envs=B, solver="fbs", tolerance=1e-9, line_impedances=(r, x))
    # and the library applies the same rules (GS_E_INVALID) where shapes allow
    if case != "shape":
        with pytest.raises(P.PowerFlowError, match=r"\(-1\)"):
            _lib.plan_describe(fs, _cfg("fbs"), B, line_impedances=(r, x))


def test_randomized_line_impedances_is_seeded_bounded_and_keeps_zero_lines():
    fs, _, _ = _with_zero_line()
    a = P.randomized_line_impedances(fs, 50, rel=0.2, seed=7)
    b = P.randomized_line_impedances(fs, 50, rel=0.2, seed=7)
    c = P.randomized_line_impedances(fs, 50, rel=0.2, seed=8)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert not np.array_equal(a[0], c[0])
    nz = np.hypot(fs.r, fs.x) > 1e-12
    for arr, nom in ((a[0], fs.r), (a[1], fs.x)):
        assert arr.shape == (50, fs.m)
        ratio = arr[:, nz & (nom != 0)] / nom[nz & (nom != 0)]
        assert (ratio >= 0.8).all() and (ratio <= 1.2).all() and ratio.std() > 0.01
        assert np.array_equal(arr[:, ~nz], np.broadcast_to(nom[~nz], (50, int((~nz).sum()))))
    _lib.check_line_impedances(fs, a[0], a[1], 50)
