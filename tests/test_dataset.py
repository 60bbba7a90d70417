"""CPU-only: the device-resident dataset's ABI section (gs_dataset_*, include/gridstep.h) as far as it can be seen without a GPU --
struct layouts, the refusals that need no device, and the index contract of the on-device draw restated from the oracle's Philox."""
import ctypes
import types

import numpy as np
import pytest

import grid_fed_rl_gym_amd as G
from grid_fed_rl_gym_amd import _lib
from oracle.oracle_np import philox4x32


def test_struct_sizes_match_the_header_layout():
    # gs_dataset_stats_view: int32 x 2, int64, int32 x 2, six pointers; gs_dataset_batch: five pointers
    assert ctypes.sizeof(_lib.gs_dataset_stats_view) == 2 * 4 + 8 + 2 * 4 + 6 * 8
    assert _lib.gs_dataset_stats_view.n.offset == 8 and _lib.gs_dataset_stats_view.obs_mean.offset == 24
    assert ctypes.sizeof(_lib.gs_dataset_batch) == 5 * 8
    assert [f for f, _ in _lib.gs_dataset_batch._fields_] == list(_lib.DATASET_KEYS)


def test_every_entry_point_refuses_a_null_handle_without_a_device():
    lib = _lib.load()
    v = _lib.gs_dataset_stats_view(ctypes.sizeof(_lib.gs_dataset_stats_view))
    b = _lib.gs_dataset_batch()
    assert lib.gs_dataset_build(None, 0) == _lib.GS_E_INVALID
    assert lib.gs_dataset_build(None, _lib.GS_DATASET_KEEP_STATS) == _lib.GS_E_INVALID
    assert lib.gs_dataset_stats(None, ctypes.byref(v)) == _lib.GS_E_INVALID
    assert lib.gs_dataset_set_stats(None, ctypes.byref(v)) == _lib.GS_E_INVALID
    assert lib.gs_dataset_sample(None, 4, None, 0, 0, 0, 1, ctypes.byref(b), None) == _lib.GS_E_INVALID
    assert b"NULL" in lib.gs_last_error(None)


def _indices_from_the_oracle(seed, draw, n, N):
    out = []
    for i in range(n):
        w = philox4x32((i >> 2, draw & 0xFFFFFFFF, (draw >> 32) & 0xFFFFFFFF, 0x534D504C), (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
        out.append((w[i & 3] * N) >> 32)
    return np.array(out, dtype=np.int64)


@pytest.mark.parametrize("N", [1, 185, 2 ** 31 - 1])
@pytest.mark.parametrize("n", [1, 4, 5, 257])
def test_indices_np_is_the_philox_contract(n, N):
    for seed, draw in ((0, 0), (7, 1), (0x0123456789ABCDEF, (3 << 32) + 9)):
        idx = G.DeviceGridDataset.indices_np(seed, draw, n, N)
        assert idx.dtype == np.int64 and idx.shape == (n,)
        assert np.array_equal(idx, _indices_from_the_oracle(seed, draw, n, N))
        assert idx.min() >= 0 and idx.max() < N
    if N > 1 and n > 1:
        assert not np.array_equal(G.DeviceGridDataset.indices_np(7, 0, n, N), G.DeviceGridDataset.indices_np(7, 1, n, N))
        assert not np.array_equal(G.DeviceGridDataset.indices_np(7, 0, n, N), G.DeviceGridDataset.indices_np(7, 1 << 32, n, N))


def test_two_draws_give_different_batches_and_a_prefix_is_a_prefix():
    a, b = G.DeviceGridDataset.indices_np(3, 0, 257, 185), G.DeviceGridDataset.indices_np(3, 1, 257, 185)
    assert not np.array_equal(a, b)
    assert np.array_equal(G.DeviceGridDataset.indices_np(3, 0, 5, 185), a[:5])           # sample i does not depend on n
    with pytest.raises(ValueError):
        G.DeviceGridDataset.indices_np(0, 0, 4, 2 ** 31)
    with pytest.raises(ValueError):
        G.DeviceGridDataset.indices_np(0, 0, 4, 0)


def test_device_dataset_refuses_an_environment_without_a_rollout():
    # (refused before any device call: these stand-ins have nothing a call could reach)
    for handle in (types.SimpleNamespace(_rollout_T=0), types.SimpleNamespace()):
        with pytest.raises(G.PowerFlowError, match="no rollout"):
            G.DeviceGridDataset(types.SimpleNamespace(handle=handle))
