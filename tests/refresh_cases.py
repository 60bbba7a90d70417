"""The case table of the per-minibatch refresh (``gs_learner_refresh``: the kernels of kernels_refresh.hip, the terminal map and the
scratch blocks of abi_refresh.hip) at its chunk, mask, clamp and buffer edges, and a NumPy model of
``gs_k_refresh_terms`` as it is written: tests/test_refresh_cases_static.py holds the table to its rules on the host and shows that the
lists tell a kernel without its chunk carry, or without its mask, from the right one; tests/test_gpu_refresh_edges.py runs the table
on the device.  No pytest code, no device, no library load: importable anywhere.

The datasets are recipes of tests/q_next_cases.py: ``BASE`` (13-bus, B = 65, T = 4, ``episode_length`` 2 under limits nothing
reaches: 260 rows whose 130 terminal entries are exactly the transitions 65 .. 129 and 195 .. 259, all of the time-limit kind) and
``DATA["ieee13"]`` (B = 5, T = 37, ``episode_length`` 14: 185 rows, both done bits)."""
from collections import namedtuple

import numpy as np

from grid_fed_rl_gym_amd.rollout import permutation_np
from tests import q_next_cases as Q

# csrc/refresh.h
GS_RF_TERM_THREADS, WAVE = 256, 64
WAVES = GS_RF_TERM_THREADS // WAVE

BASE, SMALL = Q.BASE, Q.DATA["ieee13"]
N = BASE.T * BASE.B                     # 260
TERM_CAP = 130                          # the base rollout's terminal entries
PERM_SEED, PERM_EPOCH = 5, 3            # tests/test_gpu_refresh.py's permutation


def base_flags():
    """``terminals`` [T, B] of the base rollout: every instance ends an episode at the time limit (bit 0) after steps 1 and 3"""
    flags = np.zeros((BASE.T, BASE.B), dtype=np.uint8)
    flags[BASE.episode_length - 1::BASE.episode_length] = 1
    return flags


def base_terminal_index(seed=None):
    """a terminal list [(t, b)] of the base rollout: ascending, or (``seed``) in another order -- the device appends in no particular one"""
    tb = np.argwhere(base_flags() != 0).astype(np.int32)
    return tb if seed is None else tb[np.random.default_rng(seed).permutation(len(tb))]


def terminal_map_np(terminal_index, T, B):
    """transition -> terminal entry, -1: none (``terminal_map_fill``; where a (t, b) occurs twice the last entry counts)"""
    entry = np.full(T * B, -1, dtype=np.int64)
    tb = np.asarray(terminal_index, dtype=np.int64).reshape(-1, 2)
    entry[tb[:, 0] * B + tb[:, 1]] = np.arange(len(tb))
    return entry


def clamp(indices, n_rows):
    """GS_RF_CLAMP"""
    return np.clip(np.asarray(indices, dtype=np.int64), 0, n_rows - 1)


# ---- the index lists over BASE --------------------------------------------------------------------------------------------------------

def _prefix_epoch():
    """the first epoch from PERM_EPOCH on whose permutation of ``all3`` has terminal rows at positions 255, 256, 511 and 512 (epoch 3
    has them at 255 and 256 only): found here, on the host; tests/test_refresh_cases_static.py states the number"""
    flat = base_flags().reshape(-1)
    all3 = np.tile(np.arange(N), 3)
    epoch = PERM_EPOCH
    while not flat[all3[permutation_np(PERM_SEED, epoch, 3 * N, positions=[255, 256, 511, 512])]].all():
        epoch += 1
    return epoch


def _base_lists():
    all3 = np.tile(np.arange(N), 3)
    perm3 = all3[permutation_np(PERM_SEED, PERM_EPOCH, 3 * N)]
    source = all3[permutation_np(PERM_SEED, PREFIX_EPOCH, 3 * N)]
    terminal = np.nonzero(base_flags().reshape(-1))[0]
    edges = np.concatenate([[-1, -2 ** 31, 0, N - 1, N, N + 5, 2 ** 31 - 1], perm3[:57]])
    out = {"all3": all3, "perm3": perm3, "terminal": terminal, "terminal4": np.tile(terminal, 4), "edges": edges}
    out.update({f"n{n}": source[:n] for n in (256, 257, 512, 513)})
    return {k: v.astype(np.int64) for k, v in out.items()}


PREFIX_EPOCH = _prefix_epoch()
BASE_LISTS = _base_lists()
# name: the path the list is there for (DESIGN.md section 27 "The edges")
BASE_PATHS = {
    "all3": "four chunks, the carry into chunks 1, 2, 3 is 126, 252, 378; count 390 > term_cap 130",
    "perm3": "four chunks, a terminal row in every one, in no order",
    "terminal": "waves 0 and 1 with all 64 lanes set, wave 2 with two",
    "terminal4": "every lane of every full wave set; count = n = 520, the largest k the scratch holds",
    "n256": "exactly one chunk, its last row terminal",
    "n257": "a second chunk of one row, terminal: the carry decides its place",
    "n512": "exactly two chunks, the last row terminal",
    "n513": "a third chunk of one row, terminal",
    "edges": "indices below 0 and at or above N: three clamp to row 0, four to row 259, which is terminal",
}
CARRY_LISTS = ("all3", "perm3", "terminal4", "n257", "n513")         # a kernel without its chunk carry misplaces rows of these (and of n512)


def small_lists():
    """``all`` and ``twice`` of tests/test_gpu_refresh.py over the 185-row dataset"""
    perm = permutation_np(PERM_SEED, PERM_EPOCH, SMALL.T * SMALL.B)
    return {"all": perm, "twice": np.concatenate([perm, perm[::-1]])}


def lone_done_row_between_pairs(indices, terminals, terminal_index, T, B, mask):
    """batch rows i, in list order, whose transition ended an episode (done != 0) but NOT under ``mask`` -- no pair -- and which lie
    between two rows that have one: what ``done[j] & mask`` filters and the compaction steps over"""
    j = clamp(indices, T * B)
    flags = np.asarray(terminals).astype(np.uint8).reshape(-1)[j]
    paired = ((flags & mask) != 0) & (terminal_map_np(terminal_index, T, B)[j] >= 0)
    rows = np.nonzero(paired)[0]
    if len(rows) < 2:
        return np.zeros(0, dtype=np.int64)
    lone = np.nonzero((flags != 0) & ~paired)[0]
    return lone[(lone > rows[0]) & (lone < rows[-1])]


# ---- gs_k_refresh_terms, as written ---------------------------------------------------------------------------------------------------

Terms = namedtuple("Terms", "ie pos count chunks")


def refresh_terms_np(indices, terminals, entry_map, mask, carry=True, use_mask=True):
    """``gs_k_refresh_terms`` (kernels_refresh.hip) restated step for step: ONE workgroup of 256 threads walks the batch in chunks of
    256; per chunk every wave of 64 takes the ballot of its lanes with ``done[j] & mask`` and ``map[j] >= 0``, a lane's place is
    ``running`` + the counts of the lower waves + the set lanes below it, and ``running`` grows by the chunk's total.  Returns
    ``ie`` [n, 2] (rows from ``count`` on: -1, never written), ``pos`` [n], ``count`` (= ``running`` at the end) and per chunk
    (``running`` on entry, the four waves' counts).  ``carry=False``: ``running += total`` is dropped.  ``use_mask=False``:
    ``done[j]`` stands in place of ``done[j] & mask``."""
    idx = np.asarray(indices, dtype=np.int64)
    done = np.asarray(terminals).astype(np.uint8).reshape(-1)
    entry_map = np.asarray(entry_map, dtype=np.int64)
    n, n_rows = len(idx), done.size
    ie, pos = np.full((n, 2), -1, dtype=np.int64), np.full(n, -1, dtype=np.int64)
    running, chunks = 0, []
    for base in range(0, n, GS_RF_TERM_THREADS):
        i = base + np.arange(GS_RF_TERM_THREADS)
        live = i < n
        e = np.full(GS_RF_TERM_THREADS, -1, dtype=np.int64)
        j = clamp(idx[i[live]], n_rows)
        flag = (done[j] & mask) if use_mask else done[j]
        e[live] = np.where(flag != 0, entry_map[j], -1)
        ballot = (e >= 0).reshape(WAVES, WAVE)
        wsum = ballot.sum(axis=1)
        before = np.cumsum(ballot, axis=1) - ballot                       # the set lanes below a lane
        off = running + np.concatenate([[0], np.cumsum(wsum)[:-1]])        # the counts of the lower waves
        k = np.where(ballot, off[:, None] + before, -1).reshape(-1)
        hit = live & (k >= 0)
        ie[k[hit], 0], ie[k[hit], 1] = i[hit], e[hit]
        pos[i[live]] = k[live]
        chunks.append((running, tuple(int(w) for w in wsum)))
        if carry:
            running += int(wsum.sum())
    return Terms(ie, pos, running, chunks)
