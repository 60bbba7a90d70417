"""The shape table of the training kernels (kernels_train.hip, gs_k_q_mlp_f32 of kernels_q.hip, kernels_pathwise.hip and the launch
tables and scratch sizing of abi_learner.hip) on non-square, shallow and deep networks: tests/test_learner_cases_static.py checks on
the host that the table reaches every branch it is there for and that no row is degenerate, tests/test_gpu_learner_shapes.py runs
it on the device.  No pytest code, no device: importable anywhere.

The kernels pick their branches from the layer widths and the minibatch size alone (csrc/policy.h, csrc/train.h, csrc/pathwise.h);
``facts(dims, n)`` restates those rules, so the coverage of the table is a statement about numbers, not about what ran.

Networks are drawn as tests/test_gpu_learner.py draws them (``draw``: weights N(0, 1 / fan_in), biases N(0, 0.1)); a twin's seed
belongs to its hidden shape, not to its index, so that the same network can be installed as either twin."""
import math
import zlib
from collections import namedtuple

import numpy as np

# widths and block counts of csrc/policy.h, csrc/train.h and csrc/pathwise.h
GS_POL_WAVES, GS_POL_MAX_WIDTH, GS_POLICY_MAX_LAYERS = 4, 256, 4
GS_VAL_PANEL_KB = 21
GS_TR_ROWS, GS_TR_SEG, GS_TR_WT_OUT, GS_TR_WT = 32, 256, 2, 4
GS_TR_RED_THREADS, GS_TR_RED_PER_THREAD = 256, 4
GS_PW_JT = 64
FULL_TILES = GS_POL_MAX_WIDTH // 16
REDUCE_WIDTH = GS_TR_RED_THREADS * GS_TR_RED_PER_THREAD

WIDTHS = {"ieee13": (71, 3), "ieee123": (684, 8)}            # (obs_dim, action_dim), asserted against the feeders
ROLLOUT = {"ieee13": (37, 5), "ieee123": (70, 3)}            # (B, T) of a row's collection unless a size needs more
SEGMENT_ROLLOUT = (37, 14)                                   # 518 rows: n = 513 is two weight-gradient segments and one row

Row = namedtuple("Row", "feeder hidden activation sizes")
Twins = namedtuple("Twins", "name feeder policy policy_activation q1 q2 q_activation")

# policy / critic rows: the hidden widths shape the policy, the reward critic and the thermal cost critic alike.  Activations rotate
# so that each of relu / tanh / elu meets a rectangular layer.
TABLE = (
    Row("ieee13", (), "relu", (33, 185)),                    # one layer: no backward-data launch, no transposed image
    Row("ieee13", (17,), "tanh", (33, 185)),                 # two layers, nt = 2: two wavefronts idle
    Row("ieee13", (65,), "relu", (33, 185)),                 # nt = 5: one wavefront with two tiles; a partial second input block for the head
    Row("ieee13", (96, 40), "relu", (33, 185, 513)),         # T[1] is 3 x 6; a half-empty out block; a partial in block
    Row("ieee13", (40, 96), "elu", (33, 185)),               # the transpose of it
    Row("ieee13", (256, 17, 256), "relu", (33, 185)),        # four layers; full, then narrow, then full
    Row("ieee13", (17, 240, 1), "tanh", (33, 185)),          # a one-unit layer; nt = 15
    Row("ieee13", (200, 24, 136), "elu", (33, 185)),         # nt = 13, 2, 9
)

# actor / twin rows; q1 / q2: a twin's hidden widths, None: that twin is not installed
TWINS = (
    Twins("A", "ieee13", (96, 40), "relu", (65,), (40, 96, 17), "relu"),       # twins differ in depth, width and row_stride
    Twins("B", "ieee13", (96, 40), "relu", (40, 96, 17), (65,), "relu"),       # the same twins, wider one first
    Twins("C", "ieee13", (), "elu", (), (256, 17, 256), "elu"),               # linear policy; linear twin (H0 = 1); a twin with H0 = 256
    Twins("D", "ieee13", (17, 240, 1), "tanh", None, (200,), "relu"),         # one twin only; policy and twin with different activations
    Twins("E", "ieee123", (17,), "relu", (), (17,), "relu"),                  # Q input of 692 columns in three panels
)
TWIN_CASES = {t.name: t for t in TWINS}


def row_id(row):
    return "%s-%s-%s" % (row.feeder, "x".join(map(str, row.hidden)) or "single", row.activation)


def policy_dims(feeder, hidden):
    D, A = WIDTHS[feeder]
    return [D, *hidden, 2 * A]


def value_dims(feeder, hidden):
    return [WIDTHS[feeder][0], *hidden, 1]


def q_dims(feeder, hidden):
    D, A = WIDTHS[feeder]
    return [D + A, *hidden, 1]


def _ceil(a, b):
    return -(-a // b)


def facts(dims, n=1):
    """The branch facts of a network of widths ``dims`` at a minibatch of ``n`` rows, by the rules of csrc/train.h:
    ``layers``       per layer (kb, nt, full, owned): 16-wide k blocks and column tiles of the forward image, whether gq_layer<RT, true>
                     runs, and how many column tiles wavefront 0 .. 3 owns (tile t belongs to wavefront t mod 4)
    ``T``            {l: (kb, nt)} of the transposed image of layer l >= 1: kb = the layer's nt, nt = its kb
    ``grad``         per layer, gs_k_train_grad: in_blocks (64 inputs each), out_blocks (32 outputs each), half_empty_out (the last
                     output block's second 16-wide tile does not exist), partial_in (the operand's columns -- the observation's, or the
                     padded width of the previous layer -- end inside the last input block), partial_in_past_64 (... and that block is not
                     the first), n_in_below_padded (the layer's inputs end before the previous layer's padded width)
    ``row_stride``, ``P``, ``reduce_blocks``, ``segments``, ``row_tiles`` (workgroups of the forward and backward-data kernels)."""
    L = len(dims) - 1
    assert 1 <= L <= GS_POLICY_MAX_LAYERS and all(1 <= d for d in dims) and all(d <= GS_POL_MAX_WIDTH for d in dims[1:])
    layers, grad, T = [], [], {}
    for l in range(L):
        kb, nt = _ceil(dims[l], 16), _ceil(dims[l + 1], 16)
        layers.append((kb, nt, nt == FULL_TILES, tuple(len(range(w, nt, GS_POL_WAVES)) for w in range(GS_POL_WAVES))))
        if l:
            T[l] = (nt, kb)
        bcols = dims[0] if l == 0 else 16 * kb
        in_blocks = _ceil(dims[l], 16 * GS_TR_WT)
        grad.append(dict(in_blocks=in_blocks, out_blocks=_ceil(dims[l + 1], 16 * GS_TR_WT_OUT), half_empty_out=nt % GS_TR_WT_OUT == 1,
                         partial_in=bcols % (16 * GS_TR_WT) != 0, partial_in_past_64=bcols % (16 * GS_TR_WT) != 0 and in_blocks > 1,
                         n_in_below_padded=l > 0 and dims[l] < 16 * kb))
    P = sum(dims[l + 1] * (dims[l] + 1) for l in range(L))
    return dict(n_layers=L, layers=tuple(layers), T=T, grad=tuple(grad), row_stride=sum(16 * nt for _, nt, _, _ in layers), P=P,
                reduce_blocks=_ceil(P, REDUCE_WIDTH), segments=_ceil(n, GS_TR_SEG), row_tiles=_ceil(n, GS_TR_ROWS))


def q_facts(feeder, hidden):
    """``facts`` of a Q network plus what the pathwise step and gs_k_q_mlp_f32 branch on: ``H0`` (the first layer's width, the
    chain of gs_k_pw_input_grad, staged GS_PW_JT rows at a time), ``panels`` (of the staged input, at most GS_VAL_PANEL_KB blocks
    each) and ``linear`` (the dot-product last layer reads the input panels directly)."""
    d = q_dims(feeder, hidden)
    f = facts(d)
    kb0 = f["layers"][0][0]
    f.update(H0=d[1], panels=_ceil(kb0, GS_VAL_PANEL_KB), linear=len(hidden) == 0, input_grad_stages=_ceil(d[1], GS_PW_JT))
    return f


# ---- networks --------------------------------------------------------------------------------------------------------------------

def draw(dims, seed):
    """tests/test_gpu_learner.py's ``_layers``"""
    rng = np.random.default_rng(seed)
    ws = [rng.normal(0.0, 1.0 / math.sqrt(dims[l]), (dims[l + 1], dims[l])) for l in range(len(dims) - 1)]
    bs = [rng.normal(0.0, 0.1, dims[l + 1]) for l in range(len(dims) - 1)]
    return ws, bs


SEEDS = {"policy": 1, "value": 2, "voltage": 10, "thermal": 12}      # tests/test_gpu_learner.py's


def q_seed(hidden):
    """the seed of the Q network with these hidden widths, whichever twin it is installed as"""
    return 100 + (zlib.crc32(repr(tuple(hidden)).encode()) & 0xFFFF)


def synthetic(dims_in, n, A, seed):
    """seeded inputs of a minibatch for the restatements: normalised observations [n, dims_in], stored actions [n, A] inside (-1, 1),
    advantages, returns and noise"""
    rng = np.random.default_rng(seed)
    return dict(obs=rng.normal(0.0, 1.0, (n, dims_in)).astype(np.float32), actions=np.tanh(rng.normal(0.0, 0.7, (n, A))),
                adv=rng.normal(0.0, 1.0, n).astype(np.float32), ret=rng.normal(0.0, 1.0, n).astype(np.float32), eps=rng.normal(0.0, 1.0, (n, A)),
                lp_shift=rng.normal(0.0, 0.25, n))
