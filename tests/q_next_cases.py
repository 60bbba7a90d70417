"""The case table of the policy-action TD targets (gs_k_policy_rows_f32 and gs_k_q_next_td of kernels_q_next.hip, gs_k_q_mlp_rows_f32
of kernels_q.hip, the buffers of abi_q_next.hip) at their tile, head and buffer edges:
tests/test_q_next_cases_static.py checks on the host that the table reaches every branch it is there for and that no row is
degenerate, tests/test_gpu_q_next_shapes.py runs it on the device.  No pytest code, no device: importable anywhere.

The kernels pick their branches from the layer widths, (D, A) and the row counts alone (csrc/policy.h, csrc/q_next.h,
csrc/mlp_f32.h); the functions below restate those rules, so the coverage of the table is a statement about numbers, not about what
ran.  The network shapes are those of tests/learner_cases.py (``TABLE`` as the policy with twins of the same hidden widths, ``TWINS``
A to E), whose ``facts`` gives the per-layer tiles."""
import math
from collections import namedtuple

import numpy as np

from tests import learner_cases as L

# csrc/policy.h, csrc/q_next.h
GS_POL_WAVES, GS_VAL_ROWS, GS_VAL_PANEL_KB = L.GS_POL_WAVES, 64, L.GS_VAL_PANEL_KB
LOG_STD_MIN, LOG_STD_MAX, TANH_CAP = -20.0, 2.0, 40.0      # the head's clamp (gs_k_policy_rows_f32) and gw_tanh's cap (gw_math.h)


def _ceil(a, b):
    return -(-a // b)


def head_tiles(A):
    """the last layer's column tiles, 2 A columns padded to whole tiles of 16, and the wavefront that owns each (tile t: t mod 4)"""
    nt = _ceil(2 * A, 16)
    return dict(nt=nt, owners=tuple(t % GS_POL_WAVES for t in range(nt)), last_full=(2 * A) % 16 == 0)


def noise_quads(A):
    """(Philox calls a row, the components of the last one that are used)"""
    quads = _ceil(A, 4)
    return quads, A - 4 * (quads - 1)


def term_stride(A):
    """gs_qn_term_stride: doubles per row of the head's log-probability terms in LDS"""
    return A | 1


def panel_kb(kb0):
    """gs_val_panel_kb: the k blocks of the first layer spread evenly over panels of at most GS_VAL_PANEL_KB"""
    panels = _ceil(kb0, GS_VAL_PANEL_KB)
    return _ceil(kb0, panels)


def panels(width):
    """the k blocks of each panel of a staged input of ``width`` columns"""
    kb0 = _ceil(width, 16)
    step = panel_kb(kb0)
    return tuple(min(step, kb0 - k) for k in range(0, kb0, step))


def stage(D):
    """gq_stage's form: ``even`` (EVEN = true: 16-byte loads of column pairs), ``whole`` (D % 16 == 0: no padded column), ``kb0``"""
    return dict(even=D % 2 == 0, whole=D % 16 == 0, kb0=_ceil(D, 16), panels=panels(D))


def tiles(n):
    """(workgroups of GS_VAL_ROWS rows over n rows or list entries, whether the last one is full); n = 0: (0, None), every
    workgroup returns at ``row0 >= rows``"""
    return (_ceil(n, GS_VAL_ROWS), n % GS_VAL_ROWS == 0) if n else (0, None)


# ---- feeders ---------------------------------------------------------------------------------------------------------------------

Feeder = namedtuple("Feeder", "make D A solver")
FEEDERS = {
    "ieee13": Feeder(("ieee13_like", "epsilon"), 71, 3, "fbs"),
    "ieee123": Feeder(("ieee123_like",), 684, 8, "fbs"),
    "scal6": Feeder(("scalable_like", 6, 1), 40, 1, "nr"),          # A = 1: term stride 1, e / A degenerate; D even, three blocks
    "scal9": Feeder(("scalable_like", 9, 3), 82, 2, "nr"),          # A = 2
    "scal21": Feeder(("scalable_like", 21, 1), 345, 5, "nr"),       # kb0 = 22: panels 11 + 11; the second noise quad holds one component
    "scal20": Feeder(("scalable_like", 20, 3), 320, 7, "nr"),       # D = 16 * 20, even: no padded column, one panel of 20; three of the second quad
    "scal48": Feeder(("scalable_like", 48, 1), 1193, 18, "nr"),     # 2 A = 36: three head tiles; kb0 = 75: panels 19, 19, 19, 18
}


def feeder(name):
    import grid_fed_rl_gym_amd as P
    kind, *args = FEEDERS[name].make
    if kind == "scalable_like":
        return P.scalable_like(args[0], seed=args[1])
    return getattr(P, kind)(*args)


# ---- (a) network shapes: learner_cases.TABLE and TWINS on their datasets ------------------------------------------------------------

Data = namedtuple("Data", "feeder B T episode_length limits")
DATA = {
    "ieee13": Data("ieee13", 5, 37, 14, (0.98, 1.02)),               # 185 rows: tiles of 64, 64, 57; both done bits
    "ieee123": Data("ieee123", 70, 3, 2, (0.98, 1.02)),              # 210 rows
}
HIDDEN = tuple((r.hidden, r.activation) for r in L.TABLE)
TWINS = tuple(t.name for t in L.TWINS)

# ---- (b) head and staging widths: hidden (64, 64) relu --------------------------------------------------------------------------------

# rows and terminal rows of a wide feeder (D >= 320) are chosen by ``chain_yardstick``, not on the device
YARDSTICK_DRAWS, YARDSTICK_BOUND = 20, 3.0
WIDE_D = 320
Head = namedtuple("Head", "feeder B T episode_length limits")
HEADS = (
    Head("scal6", 9, 9, 3, (0.98, 1.02)),         # 81 rows, at least 27 terminal rows
    Head("scal9", 9, 9, 3, (0.98, 1.02)),
    # the wide feeders: limits so wide that only the time limit ends an episode, so the terminal rows are the yardstick's count
    Head("scal21", 9, 18, 2, (0.5, 1.5)),         # 162 rows, 81 terminal rows
    Head("scal20", 9, 18, 2, (0.5, 1.5)),
    Head("scal48", 10, 46, 2, (0.5, 1.5)),        # 460 rows, 230 terminal rows
)
HEAD_CASES = {h.feeder: h for h in HEADS}


def head_rows(h):
    """(rollout rows, terminal rows when only the time limit ends episodes; violations end more)"""
    return h.B * h.T, h.B * (h.T // h.episode_length)


def chain_yardstick(D, rows, draws=YARDSTICK_DRAWS, H=64):
    """DESIGN.md section 25's yardstick for E_ref over ``rows`` rows of ``D`` columns, on the host alone: E_ref is NumPy's own
    float32 error, and NumPy's product is more accurate than one float32 chain where it sums in blocks.  Per draw: rows of N(0, 1)
    and an [H, D] layer of N(0, 1 / D), both float32; the error of ONE ascending chain of fused multiply-adds in float32 (each step
    the float64 sum of the float32 accumulator and the exact product, rounded to float32) against the float64 product, over the
    error of NumPy's float32 product.  Returns (median, largest) of that ratio over the draws."""
    out = []
    for s in range(draws):
        rng = np.random.default_rng(1000 + s)
        x = rng.normal(0.0, 1.0, (rows, D)).astype(np.float32)
        w = rng.normal(0.0, 1.0 / math.sqrt(D), (H, D)).astype(np.float32)
        x64, w64 = x.astype(np.float64), w.astype(np.float64)
        exact = x64 @ w64.T
        e_ref = float(np.max(np.abs((x @ w.T).astype(np.float64) - exact)))
        acc = np.zeros((rows, H), dtype=np.float32)
        for k in range(D):
            acc = (acc.astype(np.float64) + x64[:, k:k + 1] * w64[None, :, k]).astype(np.float32)
        out.append(float(np.max(np.abs(acc.astype(np.float64) - exact))) / e_ref)
    return float(np.median(out)), float(np.max(out))


# ---- (c) the head's extremes: two policies on the 13-bus dataset, hidden (64, 64) relu ------------------------------------------------

# last-layer biases per action column, (mean | log_std); the weights keep the 0.3 scale, so the biases decide
EXTREMES = {
    "high": ((45.0, 0.0, 0.0), (0.0, 6.0, -30.0)),          # mean about +45 | log_std above 2 | log_std below -20
    "low": ((-45.0, 0.0, 0.0), (0.0, -30.0, 6.0)),          # mean about -45 | log_std below -20 | log_std above 2
}


def extremes_reached(pre_head, eps, actions, log_probs):
    """What (c) asserts of a policy of ``EXTREMES``, from the pre-head values [n, 2 A] the head read, its noise [n, A] and its
    outputs: log_std lies beyond both clamp ends, |mean + exp(clamped log_std) eps| passes gw_tanh's cap, actions of exactly +-1.0
    occur and so do actions below 0.5 in magnitude, every output is finite.  Returns how many rows are ``above`` and ``below`` the
    clamp and ``capped``."""
    pre = np.asarray(pre_head, dtype=np.float64)
    A = pre.shape[1] // 2
    mean, ls = pre[:, :A], pre[:, A:]
    above, below = (ls > LOG_STD_MAX).any(axis=1), (ls < LOG_STD_MIN).any(axis=1)
    capped = (np.abs(mean + np.exp(np.clip(ls, LOG_STD_MIN, LOG_STD_MAX)) * eps) > TANH_CAP).any(axis=1)
    assert above.any() and below.any() and capped.any()
    assert (np.abs(actions) == 1.0).any() and (np.abs(actions) < 0.5).any()
    assert np.isfinite(pre).all() and np.isfinite(actions).all() and np.isfinite(log_probs).all()
    return dict(above=int(above.sum()), below=int(below.sum()), capped=int(capped.sum()))


# ---- (d) row and terminal tiles, (e) buffer reuse: 13-bus, limits so wide that only the time limit ends an episode -------------------

BASE = Data("ieee13", 65, 4, 2, (0.5, 1.5))                 # 260 rows, 130 terminal entries: two full tiles and two
Replay = namedtuple("Replay", "name T B stochastic")
REPLAYS = (
    Replay("T3-B65", 3, 65, True),          # 195 rows; 65 entries: one full tile and one; the base's B, so the base's noise index
    Replay("T4-B32", 4, 32, False),         # 128 rows: two full tiles; 64 entries: exactly one full tile
    Replay("T2-B32", 2, 32, False),         # 64 rows; 32 entries
    Replay("T1-B65", 1, 65, True),          # 65 rows; no entry
    Replay("T1-B1", 1, 1, False),           # 1 row; no entry
)
REPLAY_CASES = {r.name: r for r in REPLAYS}
# (e): on one handle the base's rollout, then the replay of one step, then the base's again; on a second handle one step first
REUSE = (("T4", "T1", "T4"), ("T1", "T4"))


def replay_rows(r, base=BASE):
    """(rollout rows, terminal entries) of the first ``r.T`` steps of the first ``r.B`` instances: an episode ends every
    ``base.episode_length`` steps, all instances together"""
    return r.T * r.B, r.B * (r.T // base.episode_length)


# ---- the branch facts of a case -----------------------------------------------------------------------------------------------------

def facts(D, A, policy_hidden, rows, terminal):
    """What gs_k_policy_rows_f32 and the two ``rows_dev`` launches branch on for a (D, A) feeder, a policy of hidden widths
    ``policy_hidden``, ``rows`` rollout rows and ``terminal`` list entries: ``head`` (``head_tiles``), ``quads`` (``noise_quads``),
    ``term_stride``, ``stage``, ``layers`` (``learner_cases.facts`` of the policy: per layer kb, nt, full, tiles owned per wavefront),
    ``row_tiles`` and ``terminal_tiles`` (``tiles``)."""
    f = L.facts([D, *policy_hidden, 2 * A])
    return dict(head=head_tiles(A), quads=noise_quads(A), term_stride=term_stride(A), stage=stage(D), layers=f["layers"], n_layers=f["n_layers"],
                row_tiles=tiles(rows), terminal_tiles=tiles(terminal))


def q_panels(D, A):
    """the panels of a twin's staged input [obs | act]"""
    return panels(D + A)


# ---- networks --------------------------------------------------------------------------------------------------------------------

LAST_SCALE = 0.3            # tests/test_gpu_q_next.py's: mean and log_std stay moderate unless a case's biases say otherwise
SQUARE = (64, 64)           # the hidden widths of (b) .. (e), relu


def policy_layers(D, A, hidden, bias=None):
    """(weights, biases) of a policy as tests/test_gpu_q_next.py draws it (``learner_cases.draw`` under the policy's seed, the
    last layer's weights scaled by LAST_SCALE); ``bias``: (mean, log_std) per action column, added to the last layer's biases"""
    ws, bs = L.draw([D, *hidden, 2 * A], L.SEEDS["policy"])
    ws[-1] = ws[-1] * LAST_SCALE
    if bias is not None:
        bs[-1] = bs[-1] + np.concatenate([np.asarray(b, dtype=np.float64) for b in bias])
    return ws, bs


def q_layers(D, A, hidden, seed):
    return L.draw([D + A, *hidden, 1], seed)


def twin_hiddens(case):
    """(hidden widths, seed) per twin of a (a) case, None where that twin is not installed.  A ``TABLE`` row: both twins with the
    row's hidden widths, two seeds.  A ``TWINS`` case: its q1 and q2 under ``learner_cases.q_seed``."""
    if isinstance(case, L.Twins):
        return tuple(None if q is None else (q, L.q_seed(q)) for q in (case.q1, case.q2))
    return tuple((case.hidden, L.q_seed(case.hidden) + w) for w in range(2))


Shape = namedtuple("Shape", "name data policy policy_activation twins q_activation")
SHAPES = tuple(Shape(L.row_id(r), r.feeder, r.hidden, r.activation, twin_hiddens(r), r.activation) for r in L.TABLE) + \
    tuple(Shape("twins-" + t.name, t.feeder, t.policy, t.policy_activation, twin_hiddens(t), t.q_activation) for t in L.TWINS)
SHAPE_CASES = {s.name: s for s in SHAPES}
