"""CPU-only: the host side of episode accounting -- ``episodes_np`` against a plain per-episode loop, the
carry across rollouts, the start modes, costs, ``EpisodeMonitor``'s merge, and the new symbols and structs of the C ABI."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

from grid_fed_rl_gym_amd import _lib
from grid_fed_rl_gym_amd.rollout import EpisodeMonitor, episodes_np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARTIAL = _lib.GS_EPISODE_PARTIAL


def _loop(rewards, terminals):
    """The reference's evaluation loop (benchmark_suite.py:374-416), one instance at a time: ``episode_return += reward``, break on
    done.  Returns the records (t_end, b, return, length, ordinal, flags) in the order instance, then time."""
    T, B = rewards.shape
    out = []
    for b in range(B):
        t, ordinal = 0, 0
        while t < T:
            episode_return, steps, ended = 0.0, 0, None
            while t < T:
                episode_return += float(rewards[t, b])
                steps += 1
                t += 1
                if terminals[t - 1, b]:
                    ended = t - 1
                    break
            if ended is None:
                break
            out.append((ended, b, episode_return, steps, ordinal, int(terminals[ended, b]) & 3))
            ordinal += 1
    return out


def _assert_records(rec, want):
    assert rec["episode_index"].tolist() == [[w[0], w[1]] for w in want]
    assert np.array_equal(rec["episode_return"], np.array([w[2] for w in want], dtype=np.float64))
    assert rec["episode_length"].tolist() == [w[3] for w in want]
    assert rec["episode_ordinal"].tolist() == [w[4] for w in want]
    assert rec["episode_flags"].tolist() == [w[5] for w in want]
    assert rec["episode_index"].dtype == np.int32 and rec["episode_return"].dtype == np.float64


def _case(B, T, seed, ends):
    """rewards of mixed magnitude (so that the order of the additions shows) and done flags at ``ends`` [(t, b, flag)]"""
    rng = np.random.default_rng(seed)
    rewards = rng.normal(size=(T, B)) * 10.0 ** rng.integers(-3, 6, size=(T, B))
    terminals = np.zeros((T, B), dtype=np.uint8)
    for t, b, flag in ends:
        terminals[t, b] = flag
    return rewards, terminals


CASES = {
    "B1_T1_no_end": (1, 1, []),
    "B1_T1_end": (1, 1, [(0, 0, 1)]),
    "B1_T7_three_ends": (1, 7, [(1, 0, 1), (2, 0, 2), (5, 0, 1)]),
    "B3_T1_all_end": (3, 1, [(0, 0, 1), (0, 1, 2), (0, 2, 1)]),
    "B3_T7_mixed": (3, 7, [(0, 2, 1), (3, 2, 2), (6, 2, 1), (4, 0, 2)]),        # instance 1 never ends; instance 2 ends three times, last on T - 1
    "B3_T7_same_step": (3, 7, [(3, 0, 1), (3, 1, 1), (3, 2, 3)]),
    "B3_T7_last_step": (3, 7, [(6, 0, 1), (6, 1, 2)]),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_episodes_np_is_the_per_episode_loop(name):
    B, T, ends = CASES[name]
    rewards, terminals = _case(B, T, 1, ends)
    rec, stats, carry = episodes_np(rewards, terminals)
    want = _loop(rewards, terminals)
    assert len(want) == len(ends)
    _assert_records(rec, want)
    assert stats.count == len(want) and stats.count_partial == 0
    # the carries: what the loop had summed when the rollout ended
    for b in range(B):
        last = max([t for t, bb, _ in ends if bb == b], default=-1)
        tail = 0.0
        for t in range(last + 1, T):
            tail += float(rewards[t, b])
        assert carry["ep_return"][b] == tail and carry["ep_length"][b] == T - 1 - last
        assert carry["ep_ordinal"][b] == sum(1 for _, bb, _ in ends if bb == b) and carry["ep_partial"][b] == 0


def test_carry_across_rollouts_gives_the_uncut_records_bit_for_bit():
    B, T = 3, 21
    # episodes that straddle the cut at 7, the cut at 8, and both (instance 1: 2 .. 15)
    ends = [(2, 0, 1), (7, 0, 2), (12, 0, 1), (1, 1, 1), (15, 1, 1), (6, 2, 1), (9, 2, 2), (20, 2, 1)]
    rewards, terminals = _case(B, T, 2, ends)
    costs = np.abs(np.random.default_rng(3).normal(size=(3, T, B))) * 10.0 ** np.random.default_rng(4).integers(-3, 4, size=(3, T, B))
    margins = np.random.default_rng(5).normal(size=(3, T, B))
    whole, _, carry_whole = episodes_np(rewards, terminals, costs, margins)
    pieces, carry, t0 = [], None, 0
    for n in (7, 1, 13):
        sl = slice(t0, t0 + n)
        rec, _, carry = episodes_np(rewards[sl], terminals[sl], costs[:, sl], margins[:, sl], carry=carry, start="fresh" if t0 == 0 else "continue")
        rec["episode_index"][:, 0] += t0
        pieces.append(rec)
        t0 += n
    joined = {k: np.concatenate([p[k] for p in pieces], axis=-1 if whole[k].ndim == 2 and k != "episode_index" else 0) for k in whole}
    order = np.lexsort((joined["episode_index"][:, 0], joined["episode_index"][:, 1]))
    assert len(order) == len(ends)
    for k in whole:
        got = joined[k][order] if k == "episode_index" or joined[k].ndim == 1 else joined[k][:, order]
        assert got.dtype == whole[k].dtype and np.array_equal(got, whole[k]), k
    for k in carry_whole:
        assert np.array_equal(carry[k], carry_whole[k]), k
    with pytest.raises(ValueError, match="continue"):
        episodes_np(rewards, terminals, start="continue")


def test_unknown_start_marks_each_instances_first_record_partial():
    B, T = 3, 7
    ends = [(0, 2, 1), (3, 2, 2), (6, 2, 1), (4, 0, 2)]
    rewards, terminals = _case(B, T, 6, ends)
    rec, stats, carry = episodes_np(rewards, terminals, start="unknown")
    fresh, fstats, _ = episodes_np(rewards, terminals, start="fresh")
    first = np.array([o == 0 for o in rec["episode_ordinal"]])
    assert np.array_equal((rec["episode_flags"] & PARTIAL) != 0, first) and first.sum() == 2
    assert np.array_equal(rec["episode_flags"] & 3, fresh["episode_flags"]) and np.array_equal(rec["episode_return"], fresh["episode_return"])
    full = rec["episode_return"][~first]
    assert stats.count == 2 and stats.count_partial == 2 and fstats.count == 4 and fstats.count_partial == 0
    assert stats.return_min == full.min() and stats.return_max == full.max() and stats.return_mean == np.mean(full)
    assert stats.length_min == 3 and stats.length_max == 3
    assert carry["ep_partial"].tolist() == [0, 1, 0]        # instance 1 never finished: its open episode is still the unseen one
    # nothing complete: NaN statistics, zero counts
    rec, stats, _ = episodes_np(rewards[:3], terminals[:3], start="unknown")
    assert len(rec["episode_return"]) == 1 and stats.count == 0 and stats.count_partial == 1 and stats.n_success == 0
    for k in ("return_mean", "return_std", "return_min", "return_max", "length_mean", "length_min", "length_max"):
        assert math.isnan(getattr(stats, k)), k
    rec, stats, _ = episodes_np(rewards[:1, :2], terminals[:1, :2])
    assert len(rec["episode_return"]) == 0 and stats.count == 0 and math.isnan(stats.return_mean) and rec["episode_index"].shape == (0, 2)


def test_costs_sum_in_step_order_and_count_negative_margins():
    B, T = 2, 6
    rewards, terminals = _case(B, T, 7, [(2, 0, 1), (5, 0, 2), (4, 1, 1)])
    rng = np.random.default_rng(8)
    costs = np.abs(rng.normal(size=(3, T, B))) * 10.0 ** rng.integers(-6, 6, size=(3, T, B))
    margins = rng.normal(size=(3, T, B))
    margins[0, 1, 0] = np.nan           # counts as nothing
    margins[:, 3, 0] = [-1.0, -2.0, 0.5]   # two channels at once: one step for any_violating
    rec, stats, carry = episodes_np(rewards, terminals, costs, margins, success_return=-np.inf)
    spans = {(2, 0): range(0, 3), (5, 0): range(3, 6), (4, 1): range(0, 5)}
    for k, (t_end, b) in enumerate(rec["episode_index"].tolist()):
        anyv = 0
        for c in range(3):
            s, v = 0.0, 0
            for t in spans[(t_end, b)]:
                s += float(costs[c, t, b])
                v += bool(margins[c, t, b] < 0)
            assert rec["episode_cost"][c, k] == s and rec["episode_violating"][c, k] == v
        for t in spans[(t_end, b)]:
            anyv += bool((margins[:, t, b] < 0).any())
        assert rec["episode_any_violating"][k] == anyv
    assert rec["episode_violating"][:, 0].sum() <= 3 * 3 - 1 and carry["ep_length"].tolist() == [0, 1]
    assert carry["ep_cost"][:, 1].tolist() == costs[:, 5, 1].tolist()
    assert stats.violating.tolist() == rec["episode_violating"].sum(axis=1).tolist()
    assert stats.n_success == int((rec["episode_any_violating"] == 0).sum())
    assert np.array_equal(stats.cost_mean, np.array([np.mean(rec["episode_cost"][c]) for c in range(3)]))
    with pytest.raises(ValueError):
        episodes_np(rewards, terminals, costs=costs)


def test_success_return_is_a_strict_floor():
    rewards = np.array([[1.0, -5.0, 2.0]])
    terminals = np.ones((1, 3), dtype=np.uint8)
    assert episodes_np(rewards, terminals, success_return=1.0)[1].n_success == 1        # 1.0 > 1.0 is false
    assert episodes_np(rewards, terminals, success_return=np.nextafter(1.0, 0.0))[1].n_success == 2
    assert episodes_np(rewards, terminals, success_return=-np.inf)[1].n_success == 3
    for bad in (np.nan, np.inf):
        with pytest.raises(ValueError, match="success_return"):
            episodes_np(rewards, terminals, success_return=bad)


def test_episode_monitor_merges_rollouts_like_the_concatenated_list():
    rng = np.random.default_rng(9)
    T, B = 40, 17
    rewards = rng.normal(-300.0, 40.0, size=(3 * T, B))
    terminals = (rng.random((3 * T, B)) < 0.15).astype(np.uint8)
    costs, margins = np.abs(rng.normal(size=(3, 3 * T, B))), rng.normal(0.5, 1.0, size=(3, 3 * T, B))
    mon, carry = EpisodeMonitor(None, window=50), None
    rets, lens, csts = [], [], []
    for r in range(3):
        sl = slice(r * T, (r + 1) * T)
        rec, stats, carry = episodes_np(rewards[sl], terminals[sl], costs[:, sl], margins[:, sl], carry=carry,
                                        start="fresh" if r == 0 else "continue", success_return=-1500.0)
        mon.merge(stats, rec["episode_return"], rec["episode_length"])
        rets.extend(rec["episode_return"].tolist()); lens.extend(rec["episode_length"].tolist()); csts.append(rec["episode_cost"])
    whole, wstats, _ = episodes_np(rewards, terminals, costs, margins, success_return=-1500.0)
    n = len(rets)
    assert n > 100 and mon.count == n == wstats.count and sorted(rets) == sorted(whole["episode_return"].tolist())
    assert mon.min_return == min(rets) and mon.max_return == max(rets)
    mean = math.fsum(rets) / n
    std = math.sqrt(math.fsum((x - mean) ** 2 for x in rets) / n)
    bound = 4 * 2.0 ** -53 * (abs(mean) + std) * math.log2(n + 1)
    print(f"monitor: n {n}, mean error {abs(mon.mean_return - mean):.3e}, std error {abs(mon.std_return - std):.3e}, bound {bound:.3e}")
    assert abs(mon.mean_return - mean) <= bound and abs(mon.std_return - std) <= bound
    assert mon.mean_length == sum(lens) / n and mon.n_success == wstats.n_success and mon.success_rate == wstats.n_success / n
    assert mon.violating.tolist() == wstats.violating.tolist()
    allc = np.concatenate(csts, axis=1)
    for c in range(3):
        want = math.fsum(allc[c].tolist()) / n
        assert abs(mon.mean_cost[c] - want) <= 4 * 2.0 ** -53 * abs(want) * math.log2(n + 1)
    assert len(mon.returns) == 50 and list(mon.returns) == rets[-50:] and mon.window_mean_return == float(np.mean(rets[-50:]))


def test_new_symbols_and_structs_agree_with_the_header():
    src = open(os.path.join(ROOT, "include", "gridstep.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = _lib.load()
    bound = {name for name, _, _ in _lib.SYMBOLS}
    for name in ("gs_rollout_episodes", "gs_rollout_episodes_view", "gs_rollout_episodes_download", "gs_episodes_clear"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", code), name
        assert hasattr(lib, name) and name in bound, name
    assert lib.gs_version() == 2 == _lib.GS_ABI_VERSION
    assert ctypes.sizeof(_lib.gs_episode_config) == 24
    assert [f[0] for f in _lib.gs_episode_config._fields_] == ["struct_size", "start", "with_costs", "reserved", "success_return"]
    assert [getattr(_lib.gs_episode_config, f).offset for f in ("struct_size", "start", "with_costs", "reserved", "success_return")] == [0, 4, 8, 12, 16]
    body = re.search(r"typedef struct gs_episode_config \{(.*?)\} gs_episode_config;", code, flags=re.S).group(1)
    assert re.findall(r"\b(struct_size|start|with_costs|reserved|success_return)\b", body) == ["struct_size", "start", "with_costs", "reserved", "success_return"]
    assert "GS_EPISODES_CONTINUE = 0, GS_EPISODES_FRESH = 1, GS_EPISODES_UNKNOWN = 2" in code
    assert "GS_EPISODE_TERMINATED = 1, GS_EPISODE_TRUNCATED = 2, GS_EPISODE_PARTIAL = 4" in code
    assert _lib.EPISODES_START == {"continue": 0, "fresh": 1, "unknown": 2} and PARTIAL == 4
    assert ctypes.sizeof(_lib.gs_episode_stats) == 16 * 8
    # the view structs: every field of the header, in its order
    for struct in (_lib.gs_rollout_episodes_dev, _lib.gs_rollout_episodes_host):
        body = re.search(r"typedef struct " + struct.__name__ + r" \{(.*?)\} " + struct.__name__ + ";", code, flags=re.S).group(1)
        names = re.findall(r"(\w+)\s*[;,]", body)
        assert names == [f[0] for f in struct._fields_], struct.__name__
    # host-side refusals need no device
    cfg = _lib.episode_config("fresh")
    assert lib.gs_rollout_episodes(None, ctypes.byref(cfg)) == _lib.GS_E_INVALID and lib.gs_episodes_clear(None) == _lib.GS_E_INVALID
