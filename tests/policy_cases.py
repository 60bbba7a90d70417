"""The case table of the MLP policy kernels (gs_k_policy_mlp, gs_k_policy_mlp_f32) at the edges of their tiling and head:
tests/test_policy_cases_static.py checks on the host that the table reaches every branch it is there for and that its policies can
see a mistake, tests/test_gpu_policy_tiling.py runs it on the device.  No pytest code, no device: importable anywhere.

One row per case: (feeder, solver, B, hidden, activation, head, compute).  The kernels pick their branches from obs_dim, the layer
widths and the batch alone (csrc/policy.h); `branches(row)` restates those rules, so the coverage of the table is a statement
about numbers, not about what ran.

Policies.  Weights N(0, 1 / fan_in) and biases N(0, 0.1) as tests/test_gpu_policy.py draws them, with the observation
normalisation folded the same way (columns that do not vary are scaled by their own size: `normalisation`).  The statistics come from the same short random rollout
(4 steps from reset(seed=11), random actions of seed 11), but of NORM_B instances evaluated with the NumPy oracle instead of the
row's own handle: the host test and the device test then hold the SAME policy, whatever the row's B (a B = 1 row would otherwise
normalise with four samples)."""
import functools
import math
import zlib
from collections import namedtuple

import numpy as np

import grid_fed_rl_gym_amd as P
from oracle import oracle_np as O
from tests import helpers as H

Row = namedtuple("Row", "feeder solver B hidden activation head compute")

FEEDERS = {
    "chain2": lambda: H.chain(2),                                     # obs_dim 16: one 16-block (f64 kb = 2, f32 kb = 1)
    "chain3": lambda: H.chain(3),                                     # 22: even, not a multiple of 16 (min(k, D - 2) with padded k)
    "star8": lambda: H.star(8),                                       # 64: a multiple of 16, no padded k
    "chain18": lambda: H.chain(18),                                   # 112: odd f32 block count (kb = 7)
    "star8_stacked": lambda: H.stack_devices(H.star(8), [1, 2, 9]),   # 81 / 12: odd, three noise quads, every noise component
    "chain168": lambda: H.chain(168),                                 # 1012: even, two f32 panels of 63 + 1 blocks
    "chain252": lambda: H.chain(252, gens=False),                     # 1511 / 1: odd, panels of 63 + 32 blocks, action_dim 1
}
WIDTHS = {"chain2": (16, 5), "chain3": (22, 5), "star8": (64, 5), "chain18": (112, 5), "star8_stacked": (81, 12),
          "chain168": (1012, 5), "chain252": (1511, 1)}              # (obs_dim, action_dim), asserted against the feeders
SOLVER = {"chain2": "fbs", "chain3": "nr", "star8": "fbs", "chain18": "nr", "star8_stacked": "nr", "chain168": "fbs", "chain252": "fbs"}
WIDE = ("chain168", "chain252")
HIDDEN = ((), (1,), (15,), (16,), (17,), (48,), (64,), (65,), (240,), (255,), (256,), (256, 17, 256), (17, 240, 1))
BATCHES = (1, 31, 32, 33, 64, 65)
B_DEFAULT = 33                   # two workgroups, the second with one instance: the row clamp and the head's break on every row
COMPUTES = ("float64", "float32")
ACTIVATIONS = ("relu", "tanh", "elu")
HEADS = ("gaussian_tanh", "tanh")

# widths and block counts of csrc/policy.h
GS_POL_ROWS, GS_POL_WAVES, GS_POL_MAX_WIDTH, GS_POL32_PANEL_KB, GS_POLICY_MAX_LAYERS = 32, 4, 256, 63, 4
FULL_TILES = GS_POL_MAX_WIDTH // 16


@functools.lru_cache(maxsize=None)
def feeder(name):
    return FEEDERS[name]()


# The rows, by the rules tests/test_policy_cases_static.py restates and holds the table to: every hidden shape once per compute path on
# the two stars; every feeder with a single layer and with (256, 256); the two wide feeders with (17,); the batch edges on chain3
# with (64,).  float64 rows rotate through relu / tanh / elu, float32 rows use relu (tests/test_gpu_policy_f32.py has tanh and elu at
# the shapes its 4 E_ref rule was established on).  B = 33 elsewhere: two workgroups, the second with a single instance.
TABLE = (
    Row("star8", "fbs", 33, (), "relu", "gaussian_tanh", "float64"),
    Row("star8_stacked", "nr", 33, (1,), "tanh", "tanh", "float64"),
    Row("star8", "fbs", 33, (15,), "elu", "gaussian_tanh", "float64"),
    Row("star8_stacked", "nr", 33, (16,), "relu", "gaussian_tanh", "float64"),
    Row("star8", "fbs", 33, (17,), "tanh", "tanh", "float64"),
    Row("star8_stacked", "nr", 33, (48,), "elu", "gaussian_tanh", "float64"),
    Row("star8", "fbs", 33, (64,), "relu", "gaussian_tanh", "float64"),
    Row("star8_stacked", "nr", 33, (65,), "tanh", "tanh", "float64"),
    Row("star8", "fbs", 33, (240,), "elu", "gaussian_tanh", "float64"),
    Row("star8_stacked", "nr", 33, (255,), "relu", "gaussian_tanh", "float64"),
    Row("star8", "fbs", 33, (256,), "tanh", "tanh", "float64"),
    Row("star8_stacked", "nr", 33, (256, 17, 256), "elu", "gaussian_tanh", "float64"),
    Row("star8", "fbs", 33, (17, 240, 1), "relu", "gaussian_tanh", "float64"),
    Row("chain2", "fbs", 33, (), "tanh", "tanh", "float64"),
    Row("chain2", "fbs", 33, (256, 256), "elu", "gaussian_tanh", "float64"),
    Row("chain3", "nr", 33, (), "relu", "gaussian_tanh", "float64"),
    Row("chain3", "nr", 33, (256, 256), "tanh", "tanh", "float64"),
    Row("star8", "fbs", 33, (256, 256), "elu", "gaussian_tanh", "float64"),
    Row("chain18", "nr", 33, (), "relu", "gaussian_tanh", "float64"),
    Row("chain18", "nr", 33, (256, 256), "tanh", "tanh", "float64"),
    Row("star8_stacked", "nr", 33, (), "elu", "gaussian_tanh", "float64"),
    Row("star8_stacked", "nr", 33, (256, 256), "relu", "gaussian_tanh", "float64"),
    Row("chain168", "fbs", 33, (), "tanh", "tanh", "float64"),
    Row("chain168", "fbs", 33, (256, 256), "elu", "gaussian_tanh", "float64"),
    Row("chain252", "fbs", 33, (), "relu", "gaussian_tanh", "float64"),
    Row("chain252", "fbs", 33, (256, 256), "tanh", "tanh", "float64"),
    Row("chain168", "fbs", 33, (17,), "elu", "gaussian_tanh", "float64"),
    Row("chain252", "fbs", 33, (17,), "relu", "gaussian_tanh", "float64"),
    Row("chain3", "nr", 1, (64,), "tanh", "tanh", "float64"),
    Row("chain3", "nr", 31, (64,), "elu", "gaussian_tanh", "float64"),
    Row("chain3", "nr", 32, (64,), "relu", "gaussian_tanh", "float64"),
    Row("chain3", "nr", 33, (64,), "tanh", "tanh", "float64"),
    Row("chain3", "nr", 64, (64,), "elu", "gaussian_tanh", "float64"),
    Row("chain3", "nr", 65, (64,), "relu", "gaussian_tanh", "float64"),
    Row("star8", "fbs", 33, (), "relu", "tanh", "float32"),
    Row("star8_stacked", "nr", 33, (1,), "relu", "gaussian_tanh", "float32"),
    Row("star8", "fbs", 33, (15,), "relu", "gaussian_tanh", "float32"),
    Row("star8_stacked", "nr", 33, (16,), "relu", "tanh", "float32"),
    Row("star8", "fbs", 33, (17,), "relu", "gaussian_tanh", "float32"),
    Row("star8_stacked", "nr", 33, (48,), "relu", "gaussian_tanh", "float32"),
    Row("star8", "fbs", 33, (64,), "relu", "tanh", "float32"),
    Row("star8_stacked", "nr", 33, (65,), "relu", "gaussian_tanh", "float32"),
    Row("star8", "fbs", 33, (240,), "relu", "gaussian_tanh", "float32"),
    Row("star8_stacked", "nr", 33, (255,), "relu", "tanh", "float32"),
    Row("star8", "fbs", 33, (256,), "relu", "gaussian_tanh", "float32"),
    Row("star8_stacked", "nr", 33, (256, 17, 256), "relu", "gaussian_tanh", "float32"),
    Row("star8", "fbs", 33, (17, 240, 1), "relu", "tanh", "float32"),
    Row("chain2", "fbs", 33, (), "relu", "gaussian_tanh", "float32"),
    Row("chain2", "fbs", 33, (256, 256), "relu", "gaussian_tanh", "float32"),
    Row("chain3", "nr", 33, (), "relu", "tanh", "float32"),
    Row("chain3", "nr", 33, (256, 256), "relu", "gaussian_tanh", "float32"),
    Row("star8", "fbs", 33, (256, 256), "relu", "gaussian_tanh", "float32"),
    Row("chain18", "nr", 33, (), "relu", "tanh", "float32"),
    Row("chain18", "nr", 33, (256, 256), "relu", "gaussian_tanh", "float32"),
    Row("star8_stacked", "nr", 33, (), "relu", "gaussian_tanh", "float32"),
    Row("star8_stacked", "nr", 33, (256, 256), "relu", "tanh", "float32"),
    Row("chain168", "fbs", 33, (), "relu", "gaussian_tanh", "float32"),
    Row("chain168", "fbs", 33, (256, 256), "relu", "gaussian_tanh", "float32"),
    Row("chain252", "fbs", 33, (), "relu", "tanh", "float32"),
    Row("chain252", "fbs", 33, (256, 256), "relu", "gaussian_tanh", "float32"),
    Row("chain168", "fbs", 33, (17,), "relu", "gaussian_tanh", "float32"),
    Row("chain252", "fbs", 33, (17,), "relu", "tanh", "float32"),
    Row("chain3", "nr", 1, (64,), "relu", "gaussian_tanh", "float32"),
    Row("chain3", "nr", 31, (64,), "relu", "gaussian_tanh", "float32"),
    Row("chain3", "nr", 32, (64,), "relu", "tanh", "float32"),
    Row("chain3", "nr", 33, (64,), "relu", "gaussian_tanh", "float32"),
    Row("chain3", "nr", 64, (64,), "relu", "gaussian_tanh", "float32"),
    Row("chain3", "nr", 65, (64,), "relu", "tanh", "float32"),
)


def key(row):
    return (row.feeder, row.B, row.hidden, row.compute)


def row_id(row):
    return "%s-B%d-%s-%s-%s-%s" % (row.feeder, row.B, "x".join(map(str, row.hidden)) or "single", row.activation, row.head, row.compute)


def dims(row):
    obs_dim, action_dim = WIDTHS[row.feeder]
    return [obs_dim, *row.hidden, 2 * action_dim if row.head == "gaussian_tanh" else action_dim]


def branches(row):
    """The branches of the row's kernel, by the rules of csrc/policy.h: `even` (GpSrcObs<EVEN> / gq_stage<EVEN>), per layer
    (kb, nt, FULL), `idle_wave` (some layer leaves a wavefront without a column tile), `panels` (float32: the staged panels of the
    observation, (count, blocks in the last one); None for float64)."""
    d = dims(row)
    f32 = row.compute == "float32"
    layers = []
    for l in range(len(d) - 1):
        k16, nt = (d[l] + 15) // 16, (d[l + 1] + 15) // 16
        layers.append((k16 if f32 else 2 * k16, nt, nt == FULL_TILES))
    panels = None
    if f32:
        count = (layers[0][0] + GS_POL32_PANEL_KB - 1) // GS_POL32_PANEL_KB
        panels = (count, layers[0][0] - GS_POL32_PANEL_KB * (count - 1))
    return dict(compute=row.compute, even=d[0] % 2 == 0, n_layers=len(layers), layers=tuple(layers),
                idle_wave=any(nt < GS_POL_WAVES for _, nt, _ in layers), panels=panels)


# ---- the environment's configuration, on the device and in the oracle ----------------------------------------------------------

def env_kw(fs, solver, episode_length=5):
    return dict(solver=solver, stochastic_loads=True, weather_variation=True, jacobian="exact", tolerance=1e-9,
                max_iterations=100 if solver == "fbs" else 50, power_base=fs.base_power_va, episode_length=episode_length)


def oracle_cfg(fs, solver, episode_length=5):
    return dict(stochastic_loads=True, weather_variation=True, power_base=fs.base_power_va, solver=solver, tolerance=1e-9,
                max_iterations=100 if solver == "fbs" else 50, jacobian_mode="exact", zero_z="open", episode_length=episode_length)


def stand_observations(name, B, seed=3, action_seed=5, T=2):
    """[B, obs_dim]: where the instances stand after reset(seed) and T steps of the random actions of `action_seed` (a rollout with
    GS_POLICY_RANDOM), from the oracle -- the observations tests/test_gpu_policy_tiling.py evaluates the policies on"""
    return _stand(name, B, seed, action_seed, T).copy()


@functools.lru_cache(maxsize=None)
def _stand(name, B, seed, action_seed, T):
    fs = feeder(name)
    d = H.oracle_collect(fs, dict(oracle_cfg(fs, SOLVER[name]), T=T), None, [seed + b for b in range(B)], 0, policy_seed=action_seed)
    assert d["converged"].all() and not d["terminals"].any(), name
    return d["next_observations"][-1]


def reset_observations(name, B, seed=3):
    """[B, obs_dim]: what reset(seed) shows instance b (seed + b), from the oracle"""
    fs = feeder(name)
    spec = H.oracle_spec(fs, **oracle_cfg(fs, SOLVER[name]))
    return np.stack([O.env_reset(spec, seed=seed + b, instance=b)[0] for b in range(B)])


# ---- policies --------------------------------------------------------------------------------------------------------------------

NORM_B, NORM_T, NORM_SEED = 16, 4, 11


@functools.lru_cache(maxsize=None)
def normalisation(name):
    """(mean, std) per observation column over collect_random_data(env, 4, seed=11) of NORM_B instances, from the oracle; columns
    that do not vary at all (the static load powers) get std = max(1, |mean|), the others std + 1e-6.  tests/test_gpu_policy.py's
    _normalisation gives the constant columns std = 1, which is enough at the 1e5 W of its feeders; the loads of a two-bus chain are
    3e7 W, and a folded weight times 3e7 cancels against the folded bias to an absolute 3e7 * 2^-53 = 4e-9 in ANY summation order --
    as there, a property of the normalisation and not of the kernel, so the column is scaled by its own size instead."""
    fs = feeder(name)
    d = H.oracle_collect(fs, dict(oracle_cfg(fs, "fbs"), T=NORM_T), None, [NORM_SEED + b for b in range(NORM_B)], 0, policy_seed=NORM_SEED)
    assert d["converged"].all(), name
    obs = d["observations"].reshape(NORM_T * NORM_B, fs.obs_dim)
    mean, std = obs.mean(axis=0), obs.std(axis=0)
    constant = std <= 1e-12 * np.maximum(1.0, np.abs(mean))
    return mean, np.where(constant, np.maximum(1.0, np.abs(mean)), std + 1e-6)


def draw(dims_, seed):
    rng = np.random.default_rng(seed)
    ws = [rng.normal(0.0, 1.0 / math.sqrt(dims_[l]), (dims_[l + 1], dims_[l])) for l in range(len(dims_) - 1)]
    bs = [rng.normal(0.0, 0.1, dims_[l + 1]) for l in range(len(dims_) - 1)]
    return ws, bs


VARIANTS = (None, "last_column", "last_unit")
LAST_UNIT_BIAS = 3.0             # the last hidden unit's bias: three standard deviations of its pre-activation, so that a relu keeps it alive


def policy(row, variant=None):
    """The row's MLPPolicy.  variant "last_column": the first layer's weights on observation column obs_dim - 1 zeroed;
    "last_unit": the last hidden unit's outgoing weights zeroed (None for a single layer, which has no hidden unit, and for a last
    hidden layer of one unit, without which the policy is a constant: the policy as drawn already rests on that unit) -- the last
    real column and the last real row of the padded tiles, which a kernel that never read them would not miss otherwise."""
    ws, bs = draw(dims(row), zlib.crc32(repr(key(row)).encode()) & 0xFFFF)
    if row.hidden:
        bs[-2][-1] = LAST_UNIT_BIAS
    if variant == "last_column":
        ws[0][:, -1] = 0.0
    elif variant == "last_unit":
        if not row.hidden or row.hidden[-1] == 1:
            return None
        ws[-1][:, -1] = 0.0
    else:
        assert variant is None
    mean, std = normalisation(row.feeder)
    return P.MLPPolicy(ws, bs, activation=row.activation, head=row.head, obs_mean=mean, obs_std=std, compute=row.compute)


def reference(pol, obs, eps=None):
    """What the device is held against: forward_np for float64, the float64 evaluation of the float32-rounded operands for float32"""
    if pol.compute == "float32":
        return pol.forward_np(obs, eps, compute="float32", exact=True)
    return pol.forward_np(obs, eps)


def e_ref(pol, obs, eps=None):
    """tests/test_gpu_policy_f32.py's E_ref: float32 forward_np against the float64 evaluation of the same rounded operands"""
    return float(np.max(np.abs(pol.forward_np(obs, eps, compute="float32") - pol.forward_np(obs, eps, compute="float32", exact=True))))


def _sincos_turns(u):
    """(sin, cos) of 2 pi u for u in (0, 1), accurate RELATIVE to their own size: the quadrant comes from 4 u, which is exact, and
    the remainder (4 u - n) pi / 2 lies in [-pi / 4, pi / 4], where libm's sin and cos carry the argument's one rounding and no
    more.  math.cos(2 pi u) rounds 2 pi u first, an absolute 4e-16 on the angle: next to a zero crossing (|cos| < 0.01, one draw
    in a hundred) that is 1e-13 and more of the value -- measured up to 3e-12 on the draws of tests/test_gpu_policy_tiling.py, which
    hold the device to rtol 1e-13 on a quantity proportional to the draw.  csrc/fastmath.h's gs_sincos_turns reduces the same way."""
    q4 = 4.0 * u
    n = round(q4)
    x = (q4 - n) * (math.pi / 2.0)
    sn, cs = math.sin(x), math.cos(x)
    return ((sn, cs), (cs, -sn), (-sn, -cs), (-cs, sn))[n & 3]


def eps_of(seed, first_instance, T, B, A):
    """eps[t, b, a]: component a & 3 of the four normals of one Philox call keyed by seed, counter (global instance, t, a // 4,
    'PNOI'): Box-Muller cosine and sine on words (0, 1) and (2, 3), u = (r + 1/2) 2^-32 -- the recipe of oracle_np.rng_normal_quad
    and of tests/test_gpu_policy.py::_eps, with the sine and cosine of `_sincos_turns`"""
    out = np.empty((T, B, A))
    for t in range(T):
        for b in range(B):
            for q in range((A + 3) // 4):
                r = O.philox4x32(((first_instance + b) & 0xFFFFFFFF, t, q, 0x504E4F49), (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
                u = [(x + 0.5) * (1.0 / 4294967296.0) for x in r]
                ra, rb = math.sqrt(-2.0 * math.log(u[0])), math.sqrt(-2.0 * math.log(u[2]))
                (sa, ca), (sb, cb) = _sincos_turns(u[1]), _sincos_turns(u[3])
                z = (ra * ca, ra * sa, rb * cb, rb * sb)
                for k in range(4):
                    if 4 * q + k < A:
                        out[t, b, 4 * q + k] = z[k]
    return out


# ---- the head: noise only, and the log_std clamp -----------------------------------------------------------------------------------

HEAD_FEEDERS = ("star8_stacked", "star8")        # action_dim 12 (quads 0 .. 2, components 0 .. 3) and 5
CLAMP_LOG_STD = (-30.0, -20.0, 0.0, 2.0, 5.0, -20.3, -19.7, 1.9, 2.1, 3.3, -1.1, 0.7)      # below, at, inside, at, above; then off the float32 grid


def head_only_policy(name, log_std, compute, hidden=(17,)):
    """A Gaussian policy whose last layer has zero weights, mean bias 0 and log_std bias `log_std` [action_dim]: its stochastic
    action is tanh(exp(clip(log_std, -20, 2)) * eps) and nothing but the draw, one exp and one tanh enters.  float32 rounds the
    bias; returns (policy, the log_std the device holds)."""
    obs_dim, action_dim = WIDTHS[name]
    ws, bs = draw([obs_dim, *hidden, 2 * action_dim], 4)
    ws[-1][:] = 0.0
    bs[-1][:action_dim] = 0.0
    bs[-1][action_dim:] = np.asarray(log_std, dtype=np.float64)[:action_dim]
    mean, std = normalisation(name)
    pol = P.MLPPolicy(ws, bs, activation="relu", head="gaussian_tanh", obs_mean=mean, obs_std=std, compute=compute)
    held = bs[-1][action_dim:]
    return pol, (held.astype(np.float32).astype(np.float64) if compute == "float32" else held.copy())
