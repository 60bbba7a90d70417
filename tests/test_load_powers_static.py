"""CPU-only: the per-instance-load step kernels (gs_k_step*_pl, gs_k_step*_pz_pl) exist for every second-generation member and keep
limits of the kind test_kernel_resources_static.py and test_line_impedances_static.py hold the other forms to."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

LIB = os.path.join(ROOT, "grid_fed_rl_gym_amd", "libgridstep.so")

# kernel: (scalar spills at most, vector spills at most) = the values measured on the build that introduced the kernels; a _pz_pl
# form whose _pz form has a larger limit in test_line_impedances_static.py takes that one.  Measured (scalar / vector), _pl forms:
# fbs_flow2h 25/8, 24/15 (stepc); fbs_flow2s 29/0, 33/0; fbs_flow2x 25/0, 24/0; nr_flow2s 30/0, 31/0; nr_flow2 54/1, 63/4;
# nr_mesh2 31/35, 35/42.  _pz_pl forms: fbs_flow2h 29/15, 30/18; fbs_flow2s 31/0, 33/0; fbs_flow2x 33/0, 28/0; nr_flow2s 32/0, 31/0;
# nr_flow2 57/3, 60/7.
LIMITS = {
    "gs_k_step_fbs_flow2h_pl": (25, 8),
    "gs_k_stepc_fbs_flow2h_pl": (24, 15),
    "gs_k_step_fbs_flow2s_pl": (29, 0),
    "gs_k_stepc_fbs_flow2s_pl": (33, 0),
    "gs_k_step_fbs_flow2x_pl": (25, 0),
    "gs_k_stepc_fbs_flow2x_pl": (24, 0),
    "gs_k_step_nr_flow2s_pl": (30, 0),
    "gs_k_stepc_nr_flow2s_pl": (31, 0),
    "gs_k_step_nr_flow2_pl": (54, 1),
    "gs_k_stepc_nr_flow2_pl": (63, 4),
    "gs_k_step_nr_mesh2_pl": (31, 35),
    "gs_k_stepc_nr_mesh2_pl": (35, 42),
    "gs_k_step_fbs_flow2h_pz_pl": (60, 15),
    "gs_k_stepc_fbs_flow2h_pz_pl": (60, 24),
    "gs_k_step_fbs_flow2s_pz_pl": (60, 0),
    "gs_k_stepc_fbs_flow2s_pz_pl": (60, 0),
    "gs_k_step_fbs_flow2x_pz_pl": (60, 0),
    "gs_k_stepc_fbs_flow2x_pz_pl": (60, 0),
    "gs_k_step_nr_flow2s_pz_pl": (60, 0),
    "gs_k_stepc_nr_flow2s_pz_pl": (60, 0),
    "gs_k_step_nr_flow2_pz_pl": (80, 3),
    "gs_k_stepc_nr_flow2_pz_pl": (80, 8),
}


@pytest.mark.skipif(not os.path.exists(LIB), reason="libgridstep.so not built")
def test_per_instance_load_step_kernels_exist_and_stay_within_their_register_limits():
    from kernel_resources import resources
    res = resources(LIB)
    for name, (smax, vmax) in LIMITS.items():
        assert name in res, name
        r = res[name]
        assert 0 <= r["sspill"] <= smax, (name, r)
        assert 0 <= r["vspill"] <= vmax, (name, r)
    # two workgroups per CU (amdgpu_waves_per_eu(4, 4)): a condition of the member, not a measurement
    for name in ("gs_k_step_fbs_flow2h_pl", "gs_k_stepc_fbs_flow2h_pl", "gs_k_step_fbs_flow2h_pz_pl", "gs_k_stepc_fbs_flow2h_pz_pl"):
        assert res[name]["vgpr"] <= 128, (name, res[name])
    for name in ("gs_k_step_nr_flow2_pl", "gs_k_stepc_nr_flow2_pl", "gs_k_step_nr_flow2_pz_pl", "gs_k_stepc_nr_flow2_pz_pl",
                 "gs_k_step_nr_mesh2_pl", "gs_k_stepc_nr_mesh2_pl"):
        assert res[name]["vgpr"] <= 256, (name, res[name])
    for name in ("gs_k_load_params", "gs_k_load_columns"):
        assert name in res and res[name]["vspill"] == 0 and res[name]["sspill"] == 0, name


@pytest.mark.skipif(not os.path.exists(LIB), reason="libgridstep.so not built")
def test_the_library_exports_the_two_entry_points():
    import ctypes
    lib = ctypes.CDLL(LIB)
    assert hasattr(lib, "gs_set_load_powers") and hasattr(lib, "gs_get_load_powers")
