"""CPU-only: the conditions without which tests/test_gpu_step_unsolved.py would be empty, held on the oracle and on the host-side
planner alone -- the bad instance of every row of tests/unsolved_cases.py ends in the oracle the way its kind says, every other
instance converges (in the slow rows strictly before the cap), the planner gives every row its member in the _pl form, and a
network with a bus that has no path to the slack goes to a kernel that tests its pivots."""
import os
import warnings

import numpy as np
import pytest

from tests import step_matrix as M
from tests import unsolved_cases as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "grid_fed_rl_gym_amd", "libgridstep.so")
needs_lib = pytest.mark.skipif(not os.path.exists(LIB), reason="libgridstep.so not built")

SLOW = [c for c in U.CASES if c.kind == "slow"]
DIVERGING = [c for c in U.CASES if c.kind == "diverging"]


def test_the_table_has_every_member_kind_and_position():
    assert {(c.member, c.kind) for c in U.CASES} == {(m, k) for m in M.MEMBERS for k in ("slow", "diverging", "overflow")}
    assert len(U.CASES) == 36 and len({U.case_id(c) for c in U.CASES}) == 36
    for c in U.CASES:
        nw, ni, iw = M.SHAPE[c.member]
        assert (c.feeder, c.solver, c.B) == (M.MEMBERS[c.member][1], M.MEMBERS[c.member][0], M.MEMBERS[c.member][2])
        assert c.bad in (U.BAD_FIRST, c.B - 1) and U.BAD_FIRST < iw - 1          # healthy instances on both sides in its wavefront
        assert c.B > iw and c.B % iw != 0 and (c.B - 1) // iw == c.B // iw     # the second position: the ragged last workgroup
        assert c.cap <= 100
        pl, tw = U.load_powers(c), U.load_powers(c, twin=True)
        others = U.healthy(c)
        assert np.array_equal(pl[others], tw[others]) and np.array_equal(tw[c.bad], U.feeder(c.feeder).load_base)
        assert np.isfinite(pl).all() and (pl[c.bad] == U.OVERFLOW_W).all() == (c.kind == "overflow")


def _healthy_converged(c, ref, strictly_before_cap):
    for b in U.healthy(c):
        for t, (o, rw, te, tr, inf, tie) in enumerate(ref[b]):
            assert inf["power_flow_converged"] and inf["status"] == 0 and inf["min_voltage"] > 0.9, (b, t, inf["status"], inf["min_voltage"])
            assert np.isfinite(o).all() and not te and not tr
            # (a tie: the kernel may stop one iteration later than the oracle -- which must still be inside the cap)
            assert inf["iterations"] + (1 if tie else 0) <= c.cap - (1 if strictly_before_cap else 0), (b, t, inf["iterations"], tie)


@pytest.mark.parametrize("c", SLOW, ids=U.case_id)
def test_slow_rows_reach_the_cap_still_contracting(c):
    ref, _ = U.oracle_steps_mixed(c)
    for t, (o, rw, te, tr, inf, tie) in enumerate(ref[c.bad]):
        assert inf["status"] == 1 and inf["iterations"] == c.cap and not inf["power_flow_converged"], (t, inf["status"], inf["iterations"])
        assert inf["max_mismatch"] < 1e-3 and inf["min_voltage"] > 0.8 and np.isfinite(o).all(), (t, inf["max_mismatch"], inf["min_voltage"])
        assert not tie
    _healthy_converged(c, ref, strictly_before_cap=True)
    # at factor 1 the same instance is done inside the cap: the twin batch is healthy throughout
    twin, _ = U.oracle_steps_mixed(c, twin=True)
    assert all(s[4]["power_flow_converged"] and s[4]["iterations"] <= c.cap and not s[5] for s in twin[c.bad])


@pytest.mark.parametrize("c", DIVERGING, ids=U.case_id)
def test_diverging_rows_reach_the_cap_far_from_a_solution(c):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ref, _ = U.oracle_steps_mixed(c)
    assert c.cap == U.DIVERGING_CAP == 12
    for t, (o, rw, te, tr, inf, tie) in enumerate(ref[c.bad]):
        assert inf["status"] == 1 and inf["iterations"] == c.cap and not inf["power_flow_converged"], (t, inf["status"], inf["iterations"])
        assert inf["max_mismatch"] > 1.0 and np.isfinite(o).all() and np.isfinite(rw), (t, inf["max_mismatch"])
    _healthy_converged(c, ref, strictly_before_cap=False)


@pytest.mark.parametrize("c", U.ROLLOUT_CASES, ids=U.case_id)
def test_rollout_rows_never_solve_the_bad_instance(c):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ref = U.oracle_rollout(c)
    others = U.healthy(c)
    assert not ref["converged"][:, c.bad].any()
    assert ref["converged"][:, others].all() and ref["min_voltage"][:, others].min() > 0.9
    term = ref["terminals"]
    assert term[2].all() and term[5].all() and term.sum() == 2 * c.B       # two episode boundaries, no truncation: the bad instance's neither


@needs_lib
@pytest.mark.parametrize("c", U.CASES + U.ROLLOUT_CASES, ids=U.case_id)
def test_the_planner_gives_every_row_its_member_with_per_instance_loads(c):
    for twin in (False, True):
        d = U.plan(c, twin)
        M.assert_describes(d, U.row_of(c), False)
        assert d["per_instance_loads"] == 1 and d["per_instance_z"] == 0


# ---- islands ----

@pytest.mark.parametrize("isl", U.ISLANDS, ids=lambda i: i.name)
def test_the_oracle_leaves_an_islanded_network_at_the_flat_start(isl):
    """power_flow.py:188-190: the first linear solve raises, the loop breaks with the flat voltages"""
    fs = isl.maker()
    assert int(np.sum(np.hypot(fs.r, fs.x) == 0.0)) == 1
    for b, (o, rw, te, tr, inf, vm) in enumerate(U.island_oracle(isl)):
        assert inf["status"] == 2 and inf["iterations"] == 1 and not inf["power_flow_converged"], (b, inf["status"], inf["iterations"])
        assert np.all(vm == 1.0) and np.isfinite(o).all() and np.isfinite(rw), b


@needs_lib
@pytest.mark.parametrize("isl", U.ISLANDS, ids=lambda i: i.name)
def test_the_planner_keeps_an_islanded_network_off_the_tables_nobody_checks(isl):
    d = U.island_plan(isl)
    if isl.meshed:      # the meshed member reads its flat-start iteration from a table without testing a pivot
        assert d["kernel"] == "nr_sparse_lu" and U.ISLAND_REASON in d["mesh2"], (d["kernel"], d["mesh2"])
    else:               # the radial members' connectivity rule (topology.cpp): a first-generation kernel
        assert d["kernel"] in ("nr_tree_lds", "nr_tree") and d["flow2"] != "on" and not any(g in d["kernel"] for g in ("flow2", "mesh2")), d
