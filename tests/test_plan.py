"""CPU-only: which kernel members a handle gets, and why a member is refused, from the host-side plan (gs_plan_describe, the JSON
gs_describe prints for a handle built from the same arguments).  The feeders, configurations and GS_* switches are those of the GPU
tests that assert the same facts on real handles; test_gpu_solver.py checks that the two agree."""
import pytest

import grid_fed_rl_gym_amd as P
from grid_fed_rl_gym_amd import _lib
from tests.helpers import broom, chain, stack_devices, star
from tests.unsolved_cases import ISLANDS, ISLAND_REASON


def config(spec, solver="nr", jacobian="exact", linear_solver="auto", tolerance=1e-6, max_iterations=50):
    """The gs_config BatchedGridEnvironment / the batched solvers build for these settings (the fields planning reads)."""
    return _lib.make_config(solver_kind=_lib.SOLVER[solver], jacobian_mode=_lib.JACOBIAN[jacobian], linear_solver=_lib.LINSOLVE[linear_solver],
                            tolerance=float(tolerance), max_iterations=int(max_iterations), power_base=spec.base_power_va)


def _star():
    import numpy as np
    from grid_fed_rl_gym_amd.feeders import FeederSpec
    n = 20
    rng = np.random.default_rng(11)
    return FeederSpec(name="star", bus_ids=list(range(n)), bus_type=np.array([2] + [0] * (n - 1), dtype=np.uint8), v_set=np.ones(n),
                      frm=np.asarray([0] + [1] * 13 + [2, 15, 16, 3, 18], dtype=np.int32), to=np.asarray(list(range(1, n)), dtype=np.int32),
                      r=rng.uniform(0.005, 0.02, n - 1), x=rng.uniform(0.005, 0.03, n - 1), rating=np.full(n - 1, 5e6))


def _pv(spec, bus):
    import dataclasses
    bt = spec.bus_type.copy(); bt[bus] = 1
    return dataclasses.replace(spec, bus_type=bt)


# (id, feeder, batch, config settings, GS_* switches, expected describe() entries)
CASES = [
    # test_gpu_env.py: the fused step kernels under an iteration cap
    ("ieee123_fbs_B37", P.ieee123_like, 37, dict(solver="fbs", tolerance=1e-9, max_iterations=2), {}, dict(kernel="fbs_flow2h")),
    ("ieee123_nr_B37", P.ieee123_like, 37, dict(tolerance=1e-9, max_iterations=1), {}, dict(kernel="nr_flow2")),
    ("ieee123_nr_B1", P.ieee123_like, 1, dict(tolerance=1e-9, max_iterations=2), {}, dict(kernel="nr_flow2")),
    ("ieee13_fbs_B9", lambda: P.ieee13_like("epsilon"), 9, dict(solver="fbs", tolerance=1e-9, max_iterations=3), {}, dict(kernel="fbs_flow2s")),
    ("ieee13_nr_B1", lambda: P.ieee13_like("epsilon"), 1, dict(tolerance=1e-9, max_iterations=2), {}, dict(kernel="nr_flow2s")),
    ("radial200_fbs_B5", lambda: P.random_meshed(200, 0, seed=5), 5, dict(solver="fbs", tolerance=1e-9, max_iterations=2), {}, dict(kernel="fbs_flow2x")),
    # test_gpu_env.py: the dataflow sweeps against the level-synchronous kernel
    ("ieee123_fbs_B130", P.ieee123_like, 130, dict(solver="fbs", tolerance=1e-4), {}, dict(kernel="fbs_flow2h", solve_kernel="fbs_flow")),
    ("ieee123_fbs_B130_iw32", P.ieee123_like, 130, dict(solver="fbs", tolerance=1e-4), {"GS_FLOW2_IW": "32"}, None),
    ("ieee123_fbs_B130_noflow2", P.ieee123_like, 130, dict(solver="fbs", tolerance=1e-4), {"GS_NO_FLOW2": "1"},
     dict(kernel="fbs_flow", flow2="disabled by GS_NO_FLOW2")),
    ("ieee123_fbs_B130_noflow", P.ieee123_like, 130, dict(solver="fbs", tolerance=1e-4), {"GS_NO_FLOW2": "1", "GS_NO_FLOW": "1"}, dict(kernel="fbs_lds")),
    ("radial256_fbs_B20_noflow", lambda: P.random_meshed(256, 0, seed=6), 20, dict(solver="fbs", tolerance=1e-4), {"GS_NO_FLOW2": "1"}, dict(kernel="fbs")),
    ("ieee123_fbs_B40", P.ieee123_like, 40, dict(solver="fbs"), {}, dict(kernel="fbs_flow2h")),
    ("ieee123_fbs_B64_waves4", P.ieee123_like, 64, dict(solver="fbs", tolerance=1e-9), {"GS_WAVES": "4"}, dict(kernel="fbs_lds", waves_per_group=4)),
    # two half-grid launches on two streams where each half still fills the device
    ("ieee123_fbs_B8192", P.ieee123_like, 8192, dict(solver="fbs", tolerance=1e-9, max_iterations=100), {}, dict(kernel="fbs_flow2h", step_launches=2)),
    ("ieee123_fbs_B8192_nosplit", P.ieee123_like, 8192, dict(solver="fbs", tolerance=1e-9, max_iterations=100), {"GS_NO_SPLIT": "1"},
     dict(kernel="fbs_flow2h", step_launches=1)),
    # test_gpu_mesh2.py: the meshed member, and the networks it does not take
    ("meshed60_B9", lambda: P.random_meshed(60, 10, seed=2), 9, dict(tolerance=1e-9), {}, dict(kernel="nr_mesh2", solve_kernel="nr_sparse_lu", mesh2="on")),
    ("scalable40_lu", lambda: P.scalable_like(40, seed=3), 9, dict(linear_solver="sparse_lu", tolerance=1e-8), {}, dict(kernel="nr_sparse_lu", mesh2="neighbours")),
    ("meshed40_lu_ascoded", lambda: P.random_meshed(40, 6, seed=2), 9, dict(linear_solver="sparse_lu", jacobian="as_coded", tolerance=1e-8), {},
     dict(kernel="nr_sparse_lu", mesh2="as-coded Jacobian")),
    ("meshed40_lu_pv", lambda: _pv(P.random_meshed(40, 6, seed=2), 5), 9, dict(linear_solver="sparse_lu", tolerance=1e-8), {},
     dict(kernel="nr_sparse_lu", mesh2="not a PQ bus")),
    ("meshed40_lu_nomesh2", lambda: P.random_meshed(40, 6, seed=2), 9, dict(linear_solver="sparse_lu", tolerance=1e-8), {"GS_NO_MESH2": "1"},
     dict(kernel="nr_sparse_lu", mesh2="GS_NO_MESH2")),
    # test_gpu_solver.py: AUTO's linear solver for meshed networks, and the first-generation dataflow sweep
    ("scalable40_auto_B70", lambda: P.scalable_like(40, seed=3), 70, dict(tolerance=1e-9, max_iterations=30), {},
     dict(solve_kernel="nr_dense_mfma", dense_form="block_row", dense_workgroups=70)),
    ("meshed40_auto_B2", lambda: P.random_meshed(40, 6, seed=2), 2, dict(tolerance=1e-9, max_iterations=30), {}, dict(solve_kernel="nr_sparse_lu")),
    ("star_fbs_B70", _star, 70, dict(solver="fbs", tolerance=1e-10, max_iterations=100), {}, dict(solve_kernel="fbs_flow")),
    ("star_fbs_B70_noflow", _star, 70, dict(solver="fbs", tolerance=1e-10, max_iterations=100), {"GS_NO_FLOW": "1"}, dict(solve_kernel="fbs_lds")),
    # test_gpu_step_limits.py: the second-generation members at the limits the planner accepts, and the reason on the far side
    ("chain17_fbs", lambda: chain(17), 13, dict(solver="fbs", tolerance=1e-9), {}, dict(kernel="fbs_flow2s")),
    ("chain18_fbs", lambda: chain(18), 21, dict(solver="fbs", tolerance=1e-9), {}, dict(kernel="fbs_flow2h")),
    ("chain129_fbs", lambda: chain(129), 35, dict(solver="fbs", tolerance=1e-9), {}, dict(kernel="fbs_flow2h")),
    ("chain130_fbs", lambda: chain(130), 19, dict(solver="fbs", tolerance=1e-9), {}, dict(kernel="fbs_flow2x")),
    ("chain252_fbs", lambda: chain(252, gens=False), 33, dict(solver="fbs", tolerance=1e-9), {}, dict(kernel="fbs_flow2x")),
    ("chain253_fbs", lambda: chain(253, gens=False), 33, dict(solver="fbs", tolerance=1e-9), {},
     dict(kernel="fbs_lds", flow2="LDS tables do not fit")),
    ("chain258_fbs", lambda: chain(258, gens=False), 33, dict(solver="fbs", tolerance=1e-9), {},
     dict(kernel="fbs_lds", flow2="more than 256 buses below the slack")),
    ("chain65_nr", lambda: chain(65), 33, dict(tolerance=1e-9), {}, dict(kernel="nr_flow2")),
    ("chain66_nr", lambda: chain(66), 33, dict(tolerance=1e-9), {}, dict(kernel="nr_tree_lds", flow2="more than 8 bus groups per wave")),
    ("broom60x8_nr", lambda: broom(60, 8), 40, dict(tolerance=1e-9), {}, dict(kernel="nr_flow2")),
    ("star8_nr", lambda: star(8), 11, dict(tolerance=1e-9), {}, dict(kernel="nr_flow2s")),
    ("star9_nr", lambda: star(9), 11, dict(tolerance=1e-9), {}, dict(kernel="nr_tree_lds", flow2="a bus has more than 8 children")),
    ("stacked2_fbs", lambda: stack_devices(chain(40), [39, 5, 20]), 20, dict(solver="fbs", tolerance=1e-9), {}, dict(kernel="fbs_flow2h")),
    ("stacked2_nr", lambda: stack_devices(chain(40), [39, 5, 20]), 35, dict(tolerance=1e-9), {}, dict(kernel="nr_flow2")),
    ("stacked2_mesh", lambda: stack_devices(P.random_meshed(60, 10, seed=2), [5, 17, 59]), 12, dict(tolerance=1e-9), {}, dict(kernel="nr_mesh2")),
    ("three_loads_fbs", lambda: stack_devices(chain(40), [20], loads=3, gens=0, bats=0), 20, dict(solver="fbs", tolerance=1e-9), {},
     dict(kernel="fbs_flow", flow2="more than two devices of a kind at one bus")),
    ("three_loads_nr", lambda: stack_devices(chain(40), [20], loads=3, gens=0, bats=0), 35, dict(tolerance=1e-9), {},
     dict(kernel="nr_tree_lds", flow2="more than two devices of a kind at one bus")),
    ("three_gens_nr", lambda: stack_devices(chain(40), [20], loads=0, gens=3, bats=0), 35, dict(tolerance=1e-9), {},
     dict(kernel="nr_tree_lds", flow2="more than two devices of a kind at one bus")),
    ("three_bats_fbs", lambda: stack_devices(chain(40), [20], loads=0, gens=0, bats=3), 20, dict(solver="fbs", tolerance=1e-9), {},
     dict(kernel="fbs_flow", flow2="more than two devices of a kind at one bus")),
    ("three_loads_mesh", lambda: stack_devices(P.random_meshed(60, 10, seed=2), [5], loads=3, gens=0, bats=0), 12, dict(tolerance=1e-9), {},
     dict(kernel="nr_sparse_lu", mesh2="more than two devices of a kind at one bus")),
    # test_gpu_step_unsolved.py: a leaf cut off by a line of zero impedance -- the meshed member reads its flat-start iteration from
    # a table without testing a pivot, so the network stays with the sparse LU, which reports the singular block
] + [(f"{isl.name}_island", isl.maker, 13, dict(tolerance=1e-9), {}, dict(kernel="nr_sparse_lu", solve_kernel="nr_sparse_lu", mesh2=ISLAND_REASON))
     for isl in ISLANDS if isl.meshed]


def _plan(spec, B, settings, switches, monkeypatch, cus=256):
    for k, v in switches.items():
        monkeypatch.setenv(k, v)
    try:
        return _lib.plan_describe(spec, config(spec, **settings), B, cus)
    finally:
        for k in switches:
            monkeypatch.delenv(k)


@pytest.mark.parametrize("name,maker,B,settings,switches,expect", CASES, ids=[c[0] for c in CASES])
def test_the_plan_picks_the_members_the_gpu_tests_see(name, maker, B, settings, switches, expect, monkeypatch):
    d = _plan(maker(), B, settings, switches, monkeypatch)
    if expect is None:      # GS_FLOW2_IW=32: the 32-instance member exists in a library built with `make EXPERIMENTS=1` only
        expect = dict(kernel="fbs_flow2" if _lib.experiments() else "fbs_flow2h")
    for k, v in expect.items():
        if k in ("flow2", "mesh2") and v != "on":
            assert v in d[k], (k, d[k])
        else:
            assert d[k] == v, (k, d[k], v)


def test_the_dense_launch_shape_follows_the_compute_units(monkeypatch):
    spec = P.scalable_like(40, seed=3)
    for cus, grid in ((256, 300), (80, 160)):
        assert _plan(spec, 300, dict(tolerance=1e-9), {}, monkeypatch, cus=cus)["dense_workgroups"] == grid


@pytest.mark.parametrize("maker,settings,message", [
    (lambda: P.random_meshed(40, 6, seed=2), dict(linear_solver="tree"), "tree elimination requested but the active network has loops"),
    (lambda: P.random_meshed(150, 10, seed=3), dict(linear_solver="dense_mfma"),
     "dense_mfma needs the exact Jacobian and at most 128 non-slack buses (have 149)"),
    (lambda: P.random_meshed(40, 6, seed=2), dict(linear_solver="dense_mfma", jacobian="as_coded"), "dense_mfma needs the exact Jacobian"),
    (lambda: P.random_meshed(40, 6, seed=2), dict(solver="fbs"), "FBS: "),
])
def test_rejections_say_why(maker, settings, message):
    spec = maker()
    with pytest.raises(P.PowerFlowError, match="gs_plan_describe failed") as e:
        _lib.plan_describe(spec, config(spec, **settings), 8)
    assert message in str(e.value)


def test_sparse_lds_is_refused_by_the_default_build():
    if _lib.experiments():
        pytest.skip("a library built with EXPERIMENTS=1 takes the member")
    spec = P.random_meshed(40, 6, seed=2)
    with pytest.raises(P.PowerFlowError, match=r"linear_solver sparse_lds is an experiment .*make EXPERIMENTS=1"):
        _lib.plan_describe(spec, config(spec, linear_solver="sparse_lds"), 8)


def test_bad_arguments_are_refused_as_by_gs_create():
    spec = P.ieee13_like("epsilon")
    cfg = config(spec)
    cfg.struct_size = 3
    with pytest.raises(P.PowerFlowError, match="struct_size mismatch"):
        _lib.plan_describe(spec, cfg, 8)
    with pytest.raises(P.PowerFlowError, match="batch must be > 0"):
        _lib.plan_describe(spec, config(spec), 0)
