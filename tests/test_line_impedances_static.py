"""CPU-only: the per-instance-impedance step kernels (gs_k_step*_pz) keep limits of the kind test_kernel_resources_static.py
holds the shared members to."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

LIB = os.path.join(ROOT, "grid_fed_rl_gym_amd", "libgridstep.so")

# kernel: (scalar spills at most, vector spills at most), measured on the build that introduced them: 25/8, 26/19, 23/0, 26/0,
# 23/0, 24/0, 23/0, 25/0, 50/0, 60/5
LIMITS = {
    "gs_k_step_fbs_flow2h_pz": (60, 8),
    "gs_k_stepc_fbs_flow2h_pz": (60, 24),
    "gs_k_step_fbs_flow2s_pz": (60, 0),
    "gs_k_stepc_fbs_flow2s_pz": (60, 0),
    "gs_k_step_fbs_flow2x_pz": (60, 0),
    "gs_k_stepc_fbs_flow2x_pz": (60, 0),
    "gs_k_step_nr_flow2s_pz": (60, 0),
    "gs_k_stepc_nr_flow2s_pz": (60, 0),
    "gs_k_step_nr_flow2_pz": (80, 0),
    "gs_k_stepc_nr_flow2_pz": (80, 8),
}


@pytest.mark.skipif(not os.path.exists(LIB), reason="libgridstep.so not built")
def test_per_instance_step_kernels_stay_within_their_register_limits():
    from kernel_resources import resources
    res = resources(LIB)
    for name, (smax, vmax) in LIMITS.items():
        assert name in res, name
        r = res[name]
        assert 0 <= r["sspill"] <= smax, (name, r)
        assert 0 <= r["vspill"] <= vmax, (name, r)
    assert res["gs_k_step_fbs_flow2h_pz"]["vgpr"] <= 128 and res["gs_k_stepc_fbs_flow2h_pz"]["vgpr"] <= 128
    assert res["gs_k_step_nr_flow2_pz"]["vgpr"] <= 256 and res["gs_k_stepc_nr_flow2_pz"]["vgpr"] <= 256
    assert "gs_k_line_params" in res and res["gs_k_line_params"]["vspill"] == 0
