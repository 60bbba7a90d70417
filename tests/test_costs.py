"""CPU-only: the host side of the constraint costs of a rollout (include/gridstep.h) -- costs_np on rows computed
by hand, formula by formula, the rules of gs_cost_config_check one by one, the ctypes struct layouts, and rollout_costs_np on a
synthetic rollout with terminal rows."""
import ctypes
import math

import numpy as np
import pytest

import grid_fed_rl_gym_amd as P
from grid_fed_rl_gym_amd import _lib
from grid_fed_rl_gym_amd.rollout import ConstraintLimits, costs_np, rollout_costs_np

N, M = 3, 2                       # Vm at 0, 2, 4; Va at 1, 3, 5; flows at 6, 8; loadings at 7, 9; f at 10; two further columns
OBS_DIM = 2 * N + 2 * M + 3
LIM = ConstraintLimits(voltage=(0.95, 1.05), frequency=(59.5, 60.5), thermal=0.8)
V, F, T = 0, 1, 2


def _row(vm=(1.0, 1.0, 1.0), load=(0.5, 0.5), f=60.0, va=(0.1, -0.2, 0.3), flow=(1e5, -2e5), rest=(7.0, -7.0)):
    o = np.empty(OBS_DIM)
    o[0:2 * N:2], o[1:2 * N:2] = vm, va
    o[2 * N:2 * N + 2 * M:2], o[2 * N + 1:2 * N + 2 * M:2] = flow, load
    o[2 * N + 2 * M] = f
    o[2 * N + 2 * M + 1:] = rest
    return o


def _one(row, kinds="excess", limits=LIM, nm=(N, M)):
    m, c, k = costs_np(row[None], nm, limits, kinds)
    assert m.shape == c.shape == k.shape == (1, 3) and m.dtype == np.float64 and c.dtype == np.int32 and k.dtype == np.float64
    return m[0], c[0], k[0]


def test_margins_counts_and_costs_of_a_safe_row():
    m, c, k = _one(_row(vm=(0.97, 1.0, 1.04), load=(0.3, -0.6), f=60.2))
    assert m[V] == min(0.97 - 0.95, 1.05 - 1.04)             # safe.py:513-522: min_i min(Vm_i - vlo, vhi - Vm_i)
    assert m[F] == min(60.2 - 59.5, 60.5 - 60.2)             # safe.py:534-542
    assert m[T] == 0.8 - 0.6                                 # safe.py:554-561: lim - max_k |L_k|, the sign of the loading dropped
    assert c.tolist() == [0, 0, 0] and k.tolist() == [0.0, 0.0, 0.0]


def test_margins_counts_and_costs_of_a_violating_row_by_kind():
    row = _row(vm=(0.93, 1.07, 1.0), load=(-0.9, 0.85), f=59.2)
    m, c, k = _one(row)
    assert m[V] == min(0.93 - 0.95, 1.05 - 1.07) and m[F] == 59.2 - 59.5 and m[T] == 0.8 - 0.9
    assert c.tolist() == [2, 1, 2]                            # base.py:153-167: buses outside the band; lines above the limit
    assert k.tolist() == [-m[V], -m[F], -m[T]]                # safe.py:471: max(0, -value)
    assert _one(row, "indicator")[2].tolist() == [1.0, 1.0, 1.0]     # safe.py:282
    assert _one(row, "count")[2].tolist() == [2.0, 1.0, 2.0]
    m2, c2, k2 = _one(row, ("count", "excess", "indicator"))
    assert k2.tolist() == [2.0, -m[F], 1.0] and np.array_equal(m2, m) and np.array_equal(c2, c)
    # one bus low only: the count is per bus, the margin the worst of them
    m, c, k = _one(_row(vm=(0.949, 1.0, 1.05)))
    assert c[V] == 1 and m[V] == 0.949 - 0.95 and k[V] == 0.95 - 0.949


def test_a_limit_exactly_at_the_extreme_is_safe():
    lim = ConstraintLimits(voltage=(0.97, 1.04), frequency=(60.2, 60.2), thermal=0.6)
    m, c, k = _one(_row(vm=(0.97, 1.0, 1.04), load=(0.3, -0.6), f=60.2), limits=lim)
    assert m.tolist() == [0.0, 0.0, 0.0] and c.tolist() == [0, 0, 0] and k.tolist() == [0.0, 0.0, 0.0]
    for kinds in ("indicator", "count"):
        assert _one(_row(vm=(0.97, 1.0, 1.04), load=(0.3, -0.6), f=60.2), kinds, lim)[2].tolist() == [0.0, 0.0, 0.0]


def test_nan_reaches_only_the_channel_whose_input_it_is():
    base = _one(_row(vm=(0.93, 1.0, 1.0), load=(0.9, 0.1), f=59.0))
    assert base[1].tolist() == [1, 1, 1]

    def poked(col):
        row = _row(vm=(0.93, 1.0, 1.0), load=(0.9, 0.1), f=59.0)
        row[col] = np.nan
        return _one(row), _one(row, "indicator")[2], _one(row, "count")[2]

    (m, c, k), ind, cnt = poked(2)                            # a Vm column (of a bus inside the band)
    assert math.isnan(m[V]) and m[F] == base[0][F] and m[T] == base[0][T]
    assert c.tolist() == [1, 1, 1] and k[V] == 0.0 and ind[V] == 0.0 and cnt[V] == 1.0      # a NaN margin costs nothing; the count stands
    (m, c, k), ind, cnt = poked(0)                            # the violating bus itself: it no longer counts
    assert math.isnan(m[V]) and c.tolist() == [0, 1, 1] and k[V] == 0.0
    for col in (1, 6, OBS_DIM - 1, OBS_DIM - 2):              # an angle, a flow, the columns behind the prefix: ignored
        (m, c, k), ind, cnt = poked(col)
        assert np.array_equal(m, base[0]) and np.array_equal(c, base[1]) and np.array_equal(k, base[2])
    (m, c, k), ind, cnt = poked(7)                            # a loading column
    assert math.isnan(m[T]) and m[V] == base[0][V] and m[F] == base[0][F] and c.tolist() == [1, 1, 0] and k[T] == 0.0
    (m, c, k), ind, cnt = poked(2 * N + 2 * M)                # the frequency
    assert math.isnan(m[F]) and m[V] == base[0][V] and m[T] == base[0][T] and c.tolist() == [1, 0, 1] and k[F] == 0.0 and ind[F] == 0.0


def test_no_lines_gives_the_limit_itself():
    row = np.array([0.9, 0.0, 1.0, 0.0, 60.0, 99.0])          # n = 2, m = 0: f at column 4
    m, c, k = _one(row, nm=(2, 0))
    assert m[T] == 0.8 and c[T] == 0 and k[T] == 0.0 and m[V] == 0.9 - 0.95 and c[V] == 1 and m[F] == 0.5


def test_costs_np_accepts_a_feeder_and_any_leading_shape():
    fs = P.ieee13_like("epsilon")
    rng = np.random.default_rng(0)
    obs = rng.uniform(0.9, 1.1, (4, 5, fs.obs_dim))
    m, c, k = costs_np(obs, fs, LIM, "count")
    assert m.shape == (4, 5, 3)
    m2, c2, k2 = costs_np(obs.reshape(20, -1), (fs.n, fs.m), LIM, "count")
    assert np.array_equal(m.reshape(20, 3), m2) and np.array_equal(c.reshape(20, 3), c2) and np.array_equal(k.reshape(20, 3), k2)
    with pytest.raises(KeyError):
        costs_np(obs, fs, LIM, "penalty")
    with pytest.raises(ValueError):
        costs_np(obs, fs, LIM, ("excess", "count"))


def test_constraint_limits_defaults():
    assert ConstraintLimits() == ConstraintLimits((0.95, 1.05), (59.5, 60.5), 0.8)

    class Env:
        voltage_limits, frequency_limits = [0.9, 1.1], (59.0, 61.0)
    assert ConstraintLimits.of(Env) == ConstraintLimits((0.9, 1.1), (59.0, 61.0), 0.8)
    assert ConstraintLimits.of(Env, thermal=1.0).thermal == 1.0


# ---- the ABI's host-only paths -----------------------------------------------------------------------------------------------------

def test_struct_sizes_match_the_header():
    # natural alignment: int32 x 4, then doubles / pointers
    assert ctypes.sizeof(_lib.gs_cost_config) == 4 * 4 + 5 * 8
    assert ctypes.sizeof(_lib.gs_cost_gae_config) == 2 * 4 + 12 * 8
    assert ctypes.sizeof(_lib.gs_rollout_costs_dev) == 2 * 4 + 4 * 8 + 12 * 8
    assert ctypes.sizeof(_lib.gs_rollout_costs_host) == 4 * 8 + 12 * 8
    assert _lib.gs_cost_config.voltage_limits.offset == 16 and _lib.gs_cost_gae_config.gamma.offset == 8
    assert _lib.gs_rollout_costs_dev.margins.offset == 8 and _lib.gs_rollout_costs_dev.values.offset == 40
    assert _lib.COST_CHANNELS == ("voltage", "frequency", "thermal") and _lib.COST_KIND == {"excess": 0, "indicator": 1, "count": 2}


def test_cost_config_check_refuses_each_rule_without_a_device():
    ok = _lib.cost_config(LIM, ("excess", "indicator", "count"))
    assert _lib.cost_config_check(ok) == (_lib.GS_OK, "")
    assert list(ok.kind) == [0, 1, 2] and list(ok.voltage_limits) == [0.95, 1.05] and ok.line_loading_limit == 0.8

    def refused(c, word):
        rc, msg = _lib.cost_config_check(c)
        assert rc == _lib.GS_E_INVALID and word in msg, (rc, msg)

    refused(_lib.cost_config(LIM, struct_size=8), "struct_size")
    for ch in range(3):
        for bad in (-1, 3):
            kinds = [0, 0, 0]
            kinds[ch] = bad
            refused(_lib.cost_config(LIM, kinds), f"kind[{ch}]")
    for bad in (np.nan, np.inf, -np.inf):
        refused(_lib.cost_config(ConstraintLimits((bad, 1.05), LIM.frequency, 0.8)), "finite")
        refused(_lib.cost_config(ConstraintLimits((0.95, bad), LIM.frequency, 0.8)), "finite")
        refused(_lib.cost_config(ConstraintLimits(LIM.voltage, (bad, 60.5), 0.8)), "finite")
        refused(_lib.cost_config(ConstraintLimits(LIM.voltage, (59.5, bad), 0.8)), "finite")
        refused(_lib.cost_config(ConstraintLimits(LIM.voltage, LIM.frequency, bad)), "finite")
    refused(_lib.cost_config(ConstraintLimits((1.05, 0.95), LIM.frequency, 0.8)), "voltage_limits: lo > hi")
    refused(_lib.cost_config(ConstraintLimits(LIM.voltage, (60.5, 59.5), 0.8)), "frequency_limits: lo > hi")
    assert _lib.cost_config_check(_lib.cost_config(ConstraintLimits((1.0, 1.0), (60.0, 60.0), 0.0))) == (_lib.GS_OK, "")      # lo = hi is a band
    lib = _lib.load()
    assert lib.gs_cost_config_check(None) == _lib.GS_E_INVALID and b"NULL" in lib.gs_last_error(None)


def test_entries_refuse_a_null_handle_and_the_critic_check_refuses_a_policy_head():
    lib = _lib.load()
    cfg = _lib.cost_config(LIM)
    assert lib.gs_cost_config_default(None, ctypes.byref(cfg)) == _lib.GS_E_INVALID
    assert lib.gs_rollout_costs(None, ctypes.byref(cfg)) == _lib.GS_E_INVALID
    assert lib.gs_costs_eval(None, None, None, 1, None, None, None) == _lib.GS_E_INVALID
    assert lib.gs_rollout_evaluate_costs(None, None) == _lib.GS_E_INVALID
    assert lib.gs_rollout_costs_view(None, None, None) == _lib.GS_E_INVALID
    assert lib.gs_rollout_costs_download(None, None) == _lib.GS_E_INVALID
    assert lib.gs_cost_value_mlp_set(None, 0, None, None) == _lib.GS_E_INVALID and b"handle" in lib.gs_last_error(None)
    # a cost critic passes the rules of gs_value_mlp_check (what gs_cost_value_mlp_set runs before it touches the device)
    rng = np.random.default_rng(0)
    ws, bs = [rng.normal(0, 0.1, (8, OBS_DIM)), rng.normal(0, 0.1, (2, 8))], [np.zeros(8), np.zeros(2)]
    f32, keep = _lib.policy_opts("float32")
    gauss, keep_g = _lib.policy_struct(ws, bs, "relu", "gaussian_tanh", False)
    rc, msg = _lib.value_check(gauss, f32, OBS_DIM)
    assert rc == _lib.GS_E_INVALID and "GS_HEAD_LINEAR" in msg
    critic, keep_c = P.MLPValue([ws[0], ws[1][:1]], [bs[0], bs[1][:1]]).to_struct()
    assert _lib.value_check(critic, f32, OBS_DIM) == (_lib.GS_OK, "")


# ---- rollout_costs_np ----------------------------------------------------------------------------------------------------------------

def test_rollout_costs_np_reads_the_terminal_row_not_the_row_after_the_reset():
    """A synthetic five-array rollout, T = 3, B = 2: instance 1 ends its episode at t = 1 on a violating observation and is reset to a
    safe one.  `next_observations[1, 1]` holds the terminal row (as gs_rollout_download files it), `observations[2, 1]` the fresh one."""
    Tn, B = 3, 2
    safe, bad = _row(), _row(vm=(0.9, 1.0, 1.0), load=(0.95, 0.1), f=61.0)
    observations = np.tile(safe, (Tn, B, 1))
    next_observations = np.tile(safe, (Tn, B, 1))
    next_observations[1, 1] = bad
    next_observations[0, 0] = _row(vm=(1.0, 1.06, 1.0))
    terminals = np.zeros((Tn, B), dtype=np.uint8)
    terminals[1, 1] = 2
    assert np.array_equal(observations[2, 1], safe)           # the row after the reset is safe
    margins, counts, costs, n_violating = rollout_costs_np(next_observations, (N, M), LIM, "indicator")
    assert margins.shape == counts.shape == costs.shape == (3, Tn, B) and margins.flags.c_contiguous
    assert costs[:, 1, 1].tolist() == [1.0, 1.0, 1.0] and counts[:, 1, 1].tolist() == [1, 1, 1]
    assert margins[V, 1, 1] == 0.9 - 0.95 and margins[F, 1, 1] == 60.5 - 61.0 and margins[T, 1, 1] == 0.8 - 0.95
    assert costs[:, 0, 0].tolist() == [1.0, 0.0, 0.0]
    assert n_violating.dtype == np.int64 and n_violating.tolist() == [2, 1, 1]
    assert costs.sum() == 4.0
    # from the post-reset rows instead, the terminal transition would look safe
    wrong = rollout_costs_np(np.concatenate([observations[1:], safe[None, None].repeat(B, 1)]), (N, M), LIM, "indicator")
    assert wrong[2][:, 1, 1].tolist() == [0.0, 0.0, 0.0]
    # the flat [T * B, obs_dim] layout of collect_*_data gives the same numbers, channel-major
    flat = rollout_costs_np(next_observations.reshape(Tn * B, -1), (N, M), LIM, "indicator")
    assert np.array_equal(flat[0], margins.reshape(3, -1)) and np.array_equal(flat[3], n_violating)
    # a NaN margin is no violation
    next_observations[2, 0, 0] = np.nan
    assert rollout_costs_np(next_observations, (N, M), LIM)[3].tolist() == [2, 1, 1]
