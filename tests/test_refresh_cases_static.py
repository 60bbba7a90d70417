"""CPU-only: the case table of tests/refresh_cases.py holds what DESIGN.md section 27 "The edges" claims of it -- each fact by the
list's NAME, so that dropping or changing that list fails here --, the NumPy model of ``gs_k_refresh_terms`` equals ``refresh_rows_np``
on every list, and the lists DISCRIMINATE: the model without its chunk carry, or without its mask, gives another answer, so the
device comparison of tests/test_gpu_refresh_edges.py cannot pass by accident.  No device is used."""
import os

import numpy as np
import pytest

from grid_fed_rl_gym_amd import _lib
from grid_fed_rl_gym_amd.rollout import permutation_np, refresh_rows_np
from tests import q_next_cases as Q
from tests import refresh_cases as R

FLAGS = R.base_flags()
ORDERS = (None, 4)             # the base's terminal list ascending and shuffled: the device appends in no particular order


def _model(idx, tb, mask=3, **kw):
    return R.refresh_terms_np(idx, FLAGS, R.terminal_map_np(tb, R.BASE.T, R.BASE.B), mask, **kw)


def test_the_models_constants_and_steps_are_the_kernels():
    here = os.path.join(os.path.dirname(_lib.__file__), "csrc")
    for name, texts in (("refresh.h", ("constexpr int GS_RF_TERM_THREADS = 256;", "#define GS_RF_CLAMP(j, N) ((j) < 0 ? 0 : ((j) >= (N) ? (N) - 1 : (j)))")),
                        ("kernels_refresh.hip", ("constexpr int WAVES = GS_RF_TERM_THREADS / 64;", "for (int base = 0; base < G.n; base += GS_RF_TERM_THREADS)",
                                                 "if (G.done[j] & G.mask) e = G.map[j];", "const int before = __popcll(ballot & ((1ull << lane) - 1ull));",
                                                 "if (w < wave) off += wsum[w];", "k = off + before;", "running += total;", "if (tid == 0) G.count[0] = running;"))):
        src = open(os.path.join(here, name)).read()
        for text in texts:
            assert text in src, (name, text)
    assert (R.GS_RF_TERM_THREADS, R.WAVE, R.WAVES) == (256, 64, 4)


def test_the_datasets_are_the_recipes_the_issue_names():
    assert R.BASE is Q.BASE and R.BASE == ("ieee13", 65, 4, 2, (0.5, 1.5)) and R.N == 260 and R.TERM_CAP == 130
    assert R.SMALL is Q.DATA["ieee13"] and R.SMALL == ("ieee13", 5, 37, 14, (0.98, 1.02)) and R.SMALL.T * R.SMALL.B == 185
    flat = FLAGS.reshape(-1)
    assert FLAGS.shape == (4, 65) and set(np.unique(flat)) == {0, 1}
    assert np.array_equal(np.nonzero(flat)[0], np.concatenate([np.arange(65, 130), np.arange(195, 260)]))
    for seed in ORDERS:
        tb = R.base_terminal_index(seed)
        assert tb.shape == (130, 2) and np.array_equal(np.sort(tb[:, 0].astype(np.int64) * 65 + tb[:, 1]), np.nonzero(flat)[0])
    assert not np.array_equal(R.base_terminal_index(4), R.base_terminal_index())
    small = R.small_lists()
    perm = permutation_np(5, 3, 185)
    assert list(small) == ["all", "twice"] and np.array_equal(small["all"], perm) and np.array_equal(small["twice"], np.concatenate([perm, perm[::-1]]))
    assert np.array_equal(np.sort(perm), np.arange(185)) and len(small["twice"]) == 370       # two chunks: 256 and 114


def test_every_list_is_what_the_table_says():
    L = R.BASE_LISTS
    assert list(L) == ["all3", "perm3", "terminal", "terminal4", "edges", "n256", "n257", "n512", "n513"] and sorted(L) == sorted(R.BASE_PATHS)
    assert {k: len(v) for k, v in L.items()} == dict(all3=780, perm3=780, terminal=130, terminal4=520, edges=64, n256=256, n257=257, n512=512, n513=513)
    flat = FLAGS.reshape(-1)
    tb = R.base_terminal_index()
    # all3: arange(260) three times over; four chunks of 126, 126, 126 and 12 terminal rows; count 390 > term_cap
    assert np.array_equal(L["all3"], np.concatenate([np.arange(260)] * 3))
    m = _model(L["all3"], tb)
    assert [sum(w) for _, w in m.chunks] == [126, 126, 126, 12] and [c for c, _ in m.chunks] == [0, 126, 252, 378]
    assert m.count == 390 > R.TERM_CAP and m.count <= len(L["all3"])
    # perm3: the same rows under permutation_np(5, 3, 780) applied to positions; every chunk holds a terminal row
    assert np.array_equal(L["perm3"], L["all3"][permutation_np(5, 3, 780)]) and np.array_equal(np.sort(L["perm3"]), np.sort(L["all3"]))
    m = _model(L["perm3"], tb)
    assert len(m.chunks) == 4 and all(sum(w) > 0 for _, w in m.chunks) and m.count == 390
    assert not np.array_equal(L["perm3"], L["all3"])
    # terminal: the 130 terminal transitions, ascending: waves 0 and 1 with all 64 lanes set, wave 2 with two
    assert np.array_equal(L["terminal"], np.nonzero(flat)[0]) and (np.diff(L["terminal"]) > 0).all()
    m = _model(L["terminal"], tb)
    assert m.chunks == [(0, (64, 64, 2, 0))] and m.count == 130
    # terminal4: four times over; every lane of every full wave is set, count = n = 520 (the scratch holds n pairs)
    assert np.array_equal(L["terminal4"], np.concatenate([L["terminal"]] * 4))
    m = _model(L["terminal4"], tb)
    assert m.chunks == [(0, (64, 64, 64, 64)), (256, (64, 64, 64, 64)), (512, (8, 0, 0, 0))] and m.count == len(L["terminal4"]) == 520
    assert np.array_equal(m.pos, np.arange(520)) and set(m.ie[:, 1]) == set(range(130))
    # the prefixes: terminal rows at positions 255 and 256, 511 and 512 -- epoch 3's permutation has them at 255 and 256 alone
    assert R.PREFIX_EPOCH == 15
    source = L["all3"][permutation_np(5, R.PREFIX_EPOCH, 780)]
    for n in (256, 257, 512, 513):
        assert np.array_equal(L[f"n{n}"], source[:n])
    assert flat[source[[255, 256, 511, 512]]].all() and not flat[L["perm3"][[511, 512]]].any()
    assert all(not flat[L["all3"][permutation_np(5, e, 780, positions=[255, 256, 511, 512])]].all() for e in range(3, R.PREFIX_EPOCH))
    for n, chunks in ((256, 1), (257, 2), (512, 2), (513, 3)):
        m = _model(L[f"n{n}"], tb)
        assert len(m.chunks) == chunks and m.pos[n - 1] == m.count - 1 >= 0, n      # the last row is terminal: the last pair
        if n in (257, 513):
            assert sum(m.chunks[-1][1]) == 1 and m.chunks[-1][0] == m.count - 1 > 0       # one row in the last chunk, placed by the carry alone
    # edges
    assert list(L["edges"][:7]) == [-1, -2 ** 31, 0, 259, 260, 265, 2 ** 31 - 1] and np.array_equal(L["edges"][7:], L["perm3"][:57])
    assert L["edges"].min() >= np.iinfo(np.int32).min and L["edges"].max() <= np.iinfo(np.int32).max
    assert set(R.CARRY_LISTS) == {"all3", "perm3", "terminal4", "n257", "n513"}


@pytest.mark.parametrize("order", ORDERS)
def test_the_model_is_refresh_rows_np_on_every_list(order):
    tb = R.base_terminal_index(order)
    for name, idx in R.BASE_LISTS.items():
        for mask in (1, 2, 3):
            own, nxt, pairs = refresh_rows_np(idx, R.BASE.T, R.BASE.B, FLAGS, tb, mask)
            m = _model(idx, tb, mask)
            assert m.count == len(pairs) and np.array_equal(m.ie[:m.count], pairs), (name, mask)
            assert (m.ie[m.count:] == -1).all()
            want = np.full(len(idx), -1)
            want[pairs[:, 0]] = np.arange(len(pairs))                      # pos is the list's inverse
            assert np.array_equal(m.pos, want), (name, mask)
            if mask == 2:                                                   # every done row is a time limit: the terminal path is on, the list is empty
                assert m.count == 0 and (m.pos == -1).all()
    # the 185-row lists, on a synthetic flag array that holds both bits and a shuffled terminal list
    T, B = R.SMALL.T, R.SMALL.B
    flags, tb = _both_bits(T, B)
    for name, idx in R.small_lists().items():
        for mask in (1, 2, 3):
            _, _, pairs = refresh_rows_np(idx, T, B, flags, tb, mask)
            m = R.refresh_terms_np(idx, flags, R.terminal_map_np(tb, T, B), mask)
            assert m.count == len(pairs) > 0 and np.array_equal(m.ie[:m.count], pairs), (name, mask)


def _both_bits(T, B):
    rng = np.random.default_rng(6)
    flags = rng.choice(np.array([0, 0, 0, 1, 2, 3], dtype=np.uint8), size=(T, B))
    tb = np.argwhere(flags != 0).astype(np.int32)
    return flags, tb[rng.permutation(len(tb))]


@pytest.mark.parametrize("order", ORDERS)
def test_the_lists_tell_a_kernel_without_its_chunk_carry_from_the_right_one(order):
    """``running += total`` dropped: the count is 0 on every list, and on every list longer than one chunk -- those of
    ``CARRY_LISTS`` and ``n512`` -- a row's place in the compacted list is wrong too, so the terminal blocks reach the wrong entries"""
    tb = R.base_terminal_index(order)
    for name, idx in R.BASE_LISTS.items():
        _, _, pairs = refresh_rows_np(idx, R.BASE.T, R.BASE.B, FLAGS, tb, 3)
        right, wrong = _model(idx, tb), _model(idx, tb, carry=False)
        assert wrong.count == 0 != len(pairs)
        misplaced = not np.array_equal(wrong.pos, right.pos)
        assert misplaced == (len(idx) > R.GS_RF_TERM_THREADS) and (misplaced or name not in R.CARRY_LISTS), name
        first = sum(right.chunks[0][1])
        assert np.array_equal(wrong.ie[:first], pairs[:first]) != misplaced, name      # later chunks overwrote the first one's pairs


def test_the_lists_tell_a_kernel_without_its_mask_from_the_right_one():
    T, B = R.SMALL.T, R.SMALL.B
    flags, tb = _both_bits(T, B)
    assert (flags == 1).any() and (flags == 2).any() and (flags == 3).any()
    entry = R.terminal_map_np(tb, T, B)
    for name, idx in R.small_lists().items():
        for mask in (1, 2):
            _, _, pairs = refresh_rows_np(idx, T, B, flags, tb, mask)
            wrong = R.refresh_terms_np(idx, flags, entry, mask, use_mask=False)
            assert wrong.count > len(pairs) and not np.array_equal(wrong.ie[:len(pairs)], pairs), (name, mask)
            assert np.array_equal(wrong.ie[:wrong.count], refresh_rows_np(idx, T, B, flags, tb, 3)[2])      # (it is mask 3's list)
            lone = R.lone_done_row_between_pairs(idx, flags, tb, T, B, mask)
            assert len(lone) and ((flags.reshape(-1)[idx[lone]] & mask) == 0).all() and (flags.reshape(-1)[idx[lone]] != 0).all()
    # on the base every done row is a time limit: mask 1 filters nothing, mask 2 everything
    tb = R.base_terminal_index()
    for name, idx in R.BASE_LISTS.items():
        assert np.array_equal(_model(idx, tb, 1).ie, _model(idx, tb, 3).ie)
        assert _model(idx, tb, 2).count == 0 < _model(idx, tb, 2, use_mask=False).count


def test_refresh_rows_np_clamps_the_edges_as_stated():
    idx = R.BASE_LISTS["edges"]
    tb = R.base_terminal_index(4)
    own, nxt, pairs = refresh_rows_np(idx, R.BASE.T, R.BASE.B, FLAGS, tb, 3)
    assert list(own[:7]) == [0, 0, 0, 259, 259, 259, 259] and np.array_equal(own, R.clamp(idx, 260)) and np.array_equal(nxt, own + 65)
    assert (own[:7] == 0).sum() == 3 and (own[:7] == 259).sum() == 4 and np.array_equal(own[7:], idx[7:])
    # row 259 is terminal: the clamped indices reach the terminal path, each occurrence a pair of its own with the entry of (3, 64)
    e = int(np.nonzero((tb[:, 0] == 3) & (tb[:, 1] == 64))[0][0])
    assert FLAGS.reshape(-1)[259] == 1 and FLAGS.reshape(-1)[0] == 0
    assert [tuple(p) for p in pairs[:4]] == [(3, e), (4, e), (5, e), (6, e)]
    # under a shorter rollout on the same handle (T = 1: N = 65) index N lands on row N - 1
    assert list(R.clamp([65, 259, -1, 64], 65)) == [64, 64, 0, 64]
    own1, _, pairs1 = refresh_rows_np(np.array([65, 259]), 1, 65, np.zeros((1, 65), dtype=np.uint8), np.zeros((0, 2), dtype=np.int32), 3)
    assert list(own1) == [64, 64] and len(pairs1) == 0
