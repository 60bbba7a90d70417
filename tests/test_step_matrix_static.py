"""CPU-only: the case table of tests/step_matrix.py has a row for every second-generation step kernel the library holds, and the
host-side planner gives every row the member and form it is there for.  A member or form added later fails here until it has a row
(and with it the GPU cases of tests/test_gpu_step_matrix.py).  Names only: no instruction is inspected."""
import os
import sys

import pytest

from tests import step_matrix as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

LIB = os.path.join(ROOT, "grid_fed_rl_gym_amd", "libgridstep.so")
# what marks a second-generation member among the gs_k_step_* / gs_k_stepc_* kernels (the first generation: gs_k_step_nr_tree, ...)
SECOND_GENERATION = ("flow2", "mesh2")


def test_the_table_has_one_row_per_member_and_form():
    assert len(M.ROWS) == 22 and len({(r.member, r.form) for r in M.ROWS}) == 22
    assert len(M.table_kernel_names()) == 44
    assert {r.member for r in M.SOLUTION_ROWS} == set(M.MEMBERS) and len(M.SOLUTION_ROWS) == len(M.MEMBERS)
    assert all(r in M.ROWS for r in M.RANDOM_ROWS) and {r.solver for r in M.RANDOM_ROWS} == {"fbs", "nr"}
    assert any(r.member == "nr_mesh2" for r in M.RANDOM_ROWS) and any(r.member in ("nr_flow2", "nr_flow2s") for r in M.RANDOM_ROWS)


@pytest.mark.skipif(not os.path.exists(LIB), reason="libgridstep.so not built")
def test_the_table_names_every_second_generation_step_kernel_of_the_library():
    from kernel_resources import resources
    built = {name for name in resources(LIB)
             if name.startswith(("gs_k_step_", "gs_k_stepc_")) and any(tag in name for tag in SECOND_GENERATION)}
    from grid_fed_rl_gym_amd import _lib
    if _lib.experiments():      # (the 32-instance sweep member of `make EXPERIMENTS=1`, reached through GS_FLOW2_IW=32 only)
        built -= {"gs_k_step_fbs_flow2", "gs_k_stepc_fbs_flow2"}
    assert built == M.table_kernel_names(), (sorted(built - M.table_kernel_names()), sorted(M.table_kernel_names() - built))


@pytest.mark.skipif(not os.path.exists(LIB), reason="libgridstep.so not built")
@pytest.mark.parametrize("row", M.ROWS + M.LIMIT_ROWS, ids=M.row_id)
def test_the_planner_gives_every_row_its_member_and_form(row):
    M.assert_describes(M.plan(row), row, False)
    nw, ni, iw = M.SHAPE[row.member]
    assert row.B > iw and row.B % iw != 0                    # one full workgroup and a ragged one
