"""ctypes binding of libgridstep.so (include/gridstep.h).

This is the only place Python touches the device path.  There is no fallback of any kind:
if the shared library has not been built (``python -c "import __graft_entry__ as g; g.build()"``
or ``make -C grid_fed_rl_gym_amd/csrc``) loading raises, and if no GPU is visible
``gs_create`` fails with GS_E_NO_DEVICE and ``Handle`` raises PowerFlowError.
"""
from __future__ import annotations

import ctypes as C
import json
import os
import sys
from typing import Optional, Tuple

import numpy as np

from .components import PowerFlowError
from .feeders import FeederSpec

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libgridstep.so")

GS_ABI_VERSION = 2
GS_OK, GS_E_INVALID, GS_E_NO_DEVICE, GS_E_HIP, GS_E_TOPOLOGY, GS_E_STATE, GS_E_COMM, GS_E_NOMEM = 0, -1, -2, -3, -4, -5, -6, -7
JACOBIAN = {"as_coded": 0, "exact": 1}
ZERO_Z = {"open": 0, "epsilon": 1}
SOLVER = {"nr": 0, "newton_raphson": 0, "fbs": 1}
LINSOLVE = {"auto": 0, "tree": 1, "sparse_lu": 2, "dense_pivot": 3, "dense_mfma": 4, "sparse_lds": 5}
KERNEL_NAMES = ["unpack", "env_pre", "solve", "env_post", "pack"]

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int32)
_up = C.POINTER(C.c_uint8)


class gs_topology(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("n", C.c_int32), ("m", C.c_int32),
                ("from_bus", _ip), ("to_bus", _ip), ("r", _dp), ("x", _dp), ("rating", _dp),
                ("bus_type", _up), ("v_set", _dp),
                ("n_loads", C.c_int32), ("load_bus", _ip), ("load_base", _dp), ("load_pf", _dp),
                ("n_gens", C.c_int32), ("gen_bus", _ip), ("gen_kind", _ip), ("gen_cap", _dp),
                ("gen_p0", _dp), ("gen_p1", _dp), ("gen_p2", _dp),
                ("n_bats", C.c_int32), ("bat_bus", _ip), ("bat_cap", _dp), ("bat_rating", _dp), ("bat_eff", _dp),
                ("line_r_inst", _dp), ("line_x_inst", _dp), ("load_base_inst", _dp)]


class gs_config(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("solver_kind", C.c_int32), ("jacobian_mode", C.c_int32),
                ("zero_z_mode", C.c_int32), ("linear_solver", C.c_int32), ("max_iterations", C.c_int32),
                ("episode_length", C.c_int32), ("stochastic_loads", C.c_int32), ("weather_variation", C.c_int32),
                ("waves_per_group", C.c_int32), ("fbs_warm_start", C.c_int32),
                ("tolerance", C.c_double), ("acceleration_factor", C.c_double), ("timestep", C.c_double),
                ("v_min", C.c_double), ("v_max", C.c_double), ("f_min", C.c_double), ("f_max", C.c_double),
                ("safety_penalty", C.c_double), ("inertia_H", C.c_double), ("damping_D", C.c_double),
                ("f_nominal", C.c_double), ("power_base", C.c_double)]


class gs_solution_view(C.Structure):
    _fields_ = [("bus_voltages", _dp), ("bus_angles", _dp), ("line_flows", _dp), ("line_loadings", _dp),
                ("losses", _dp), ("max_mismatch", _dp), ("iterations", _ip), ("converged", _up), ("status", _ip)]


class gs_info_view(C.Structure):
    _fields_ = [("power_flow_converged", _up), ("max_voltage", _dp), ("min_voltage", _dp), ("total_losses", _dp),
                ("violations", _up), ("constraint_violations", _ip), ("current_step", _ip),
                ("episode_reward", _dp), ("iterations", _ip), ("status", _ip)]


class gs_rollout_view(C.Structure):
    _fields_ = [("observations", _dp), ("actions", _dp), ("rewards", _dp), ("next_observations", _dp), ("terminals", _up),
                ("final_observation", _dp), ("n_terminal", _ip)]


class gs_rollout_device(C.Structure):
    _fields_ = [("T", C.c_int32), ("B", C.c_int32), ("obs_dim", C.c_int32), ("action_dim", C.c_int32),
                ("obs_seq", C.c_void_p), ("actions", C.c_void_p), ("rewards", C.c_void_p), ("terminals", C.c_void_p),
                ("n_terminal", C.c_int32), ("reserved", C.c_int32), ("terminal_index", C.c_void_p), ("terminal_obs", C.c_void_p)]


class gs_rollout_source(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("dtype", C.c_int32), ("T", C.c_int32), ("chunk_rows", C.c_int32), ("flags", C.c_uint32),
                ("observations", C.c_void_p), ("actions", C.c_void_p), ("rewards", C.c_void_p), ("next_observations", C.c_void_p),
                ("terminals", _up), ("final_observation", C.c_void_p), ("log_probs", C.c_void_p)]


class gs_rollout_load_info(C.Structure):
    _fields_ = [("n", C.c_int64), ("n_terminal", C.c_int32), ("term_cap_needed", C.c_int32)]


class gs_rollout_continue_config(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("T", C.c_int32), ("keep", C.c_int32), ("policy", C.c_int32), ("policy_seed", C.c_uint64),
                ("t0", C.c_uint32), ("reserved", C.c_uint32), ("actions", _dp)]


class gs_rollout_window_info_out(C.Structure):
    _fields_ = [("T", C.c_int32), ("kept", C.c_int32), ("t0_next", C.c_uint32), ("T_cap", C.c_int32)]


POLICY = {"uploaded": 0, "random": 1, "mlp": 2}
ACTIVATION = {"relu": 0, "tanh": 1, "elu": 2}
HEAD = {"tanh": 0, "gaussian_tanh": 1}
GS_POLICY_MAX_LAYERS = 4


class gs_policy_mlp(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("n_layers", C.c_int32), ("dims", C.c_int32 * (GS_POLICY_MAX_LAYERS + 1)),
                ("activation", C.c_int32), ("head", C.c_int32), ("stochastic", C.c_int32),
                ("weights", _dp * GS_POLICY_MAX_LAYERS), ("biases", _dp * GS_POLICY_MAX_LAYERS)]


COMPUTE = {"float64": 0, "float32": 1}      # GS_COMPUTE_F64 / GS_COMPUTE_F32


class gs_policy_mlp_opts(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("compute", C.c_int32), ("obs_shift", _dp), ("obs_scale", _dp)]


GS_HEAD_LINEAR = 2          # gs_policy_mlp.head of a value network (gs_value_mlp_set)


class gs_gae_config(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("bootstrap_mask", C.c_int32), ("gamma", C.c_double), ("lam", C.c_double),
                ("reward_shift", C.c_double), ("reward_scale", C.c_double)]


class gs_rollout_onpolicy(C.Structure):
    _fields_ = [("T", C.c_int32), ("B", C.c_int32), ("n_terminal", C.c_int32), ("rows_per_tile", C.c_int32),
                ("log_probs", C.c_void_p), ("values", C.c_void_p), ("terminal_values", C.c_void_p), ("advantages", C.c_void_p),
                ("returns", C.c_void_p)]


class gs_rollout_onpolicy_host(C.Structure):
    _fields_ = [("log_probs", _dp), ("values", _dp), ("terminal_values", _dp), ("advantages", _dp), ("returns", _dp)]


ONPOLICY_KEYS = ("log_probs", "values", "terminal_values", "advantages", "returns")      # gs_rollout_onpolicy_host's fields, in order
BOOTSTRAP = {"terminated": 1, "truncated": 2}      # bits of gs_gae_config.bootstrap_mask


# constraint costs of a rollout (include/gridstep.h): channels, kinds and the structs of gs_rollout_costs / gs_rollout_evaluate_costs
COST_CHANNELS = ("voltage", "frequency", "thermal")      # GS_COST_VOLTAGE, GS_COST_FREQUENCY, GS_COST_THERMAL
COST_KIND = {"excess": 0, "indicator": 1, "count": 2}    # GS_COSTKIND_*
_d3, _vp3, _dp3 = C.c_double * 3, C.c_void_p * 3, _dp * 3


class gs_cost_config(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("kind", C.c_int32 * 3), ("voltage_limits", C.c_double * 2),
                ("frequency_limits", C.c_double * 2), ("line_loading_limit", C.c_double)]


class gs_cost_gae_config(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("bootstrap_mask", C.c_int32), ("gamma", _d3), ("lam", _d3), ("cost_shift", _d3),
                ("cost_scale", _d3)]


class gs_rollout_costs_dev(C.Structure):
    _fields_ = [("T", C.c_int32), ("B", C.c_int32), ("margins", C.c_void_p), ("counts", C.c_void_p), ("costs", C.c_void_p),
                ("n_violating", C.c_void_p), ("values", _vp3), ("terminal_values", _vp3), ("advantages", _vp3), ("returns", _vp3)]


class gs_rollout_costs_host(C.Structure):
    _fields_ = [("margins", _dp), ("counts", _ip), ("costs", _dp), ("n_violating", C.POINTER(C.c_int64)), ("values", _dp3),
                ("terminal_values", _dp3), ("advantages", _dp3), ("returns", _dp3)]


COST_CRITIC_KEYS = ("values", "terminal_values", "advantages", "returns")      # the per-channel fields of both structs, in order


def cost_config(limits=None, kinds="excess", struct_size=None) -> gs_cost_config:
    """gs_cost_config from ``limits`` -- anything with ``voltage``, ``frequency`` (lo, hi) and ``thermal`` -- and ``kinds``: one name
    of COST_KIND (or its number) for all channels, or three."""
    ks = [kinds] * 3 if isinstance(kinds, (str, int, np.integer)) else list(kinds)
    if len(ks) != 3:
        raise PowerFlowError(f"kinds: one kind or three, got {len(ks)}")
    ks = [COST_KIND[k] if isinstance(k, str) else int(k) for k in ks]
    c = gs_cost_config()
    c.struct_size = C.sizeof(gs_cost_config) if struct_size is None else int(struct_size)
    c.kind[:] = ks
    c.voltage_limits[:] = [float(x) for x in limits.voltage]
    c.frequency_limits[:] = [float(x) for x in limits.frequency]
    c.line_loading_limit = float(limits.thermal)
    return c


def _host_check(name: str, *args) -> Tuple[int, str]:
    """(return code, message) of ``name``, one of the library's checks that run on the host alone (no GPU, no handle)."""
    lib = load()
    rc = getattr(lib, name)(*args)
    return rc, ("" if rc == GS_OK else lib.gs_last_error(None).decode())


def _critic_shapes(T: int, B: int, n_terminal: int) -> dict:
    """The shapes of what a critic leaves over a rollout (COST_CRITIC_KEYS; ONPOLICY_KEYS without ``log_probs``)."""
    return dict(values=(T + 1, B), terminal_values=(n_terminal,), advantages=(T, B), returns=(T, B))


def cost_config_check(c: gs_cost_config) -> Tuple[int, str]:
    """gs_cost_config_check: (return code, message) -- the rules of a cost configuration on the host alone (no GPU)."""
    return _host_check("gs_cost_config_check", C.byref(c))


# episode accounting over rollouts (include/gridstep.h): start modes, the record flags' bits and the structs of gs_rollout_episodes
EPISODES_START = {"continue": 0, "fresh": 1, "unknown": 2}      # GS_EPISODES_*
GS_EPISODE_TERMINATED, GS_EPISODE_TRUNCATED, GS_EPISODE_PARTIAL = 1, 2, 4
_i64_3 = C.c_int64 * 3


class gs_episode_config(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("start", C.c_int32), ("with_costs", C.c_int32), ("reserved", C.c_int32),
                ("success_return", C.c_double)]


class gs_episode_stats(C.Structure):
    _fields_ = [("count", C.c_int64), ("count_partial", C.c_int64), ("return_mean", C.c_double), ("return_std", C.c_double),
                ("return_min", C.c_double), ("return_max", C.c_double), ("length_mean", C.c_double), ("length_min", C.c_double),
                ("length_max", C.c_double), ("cost_mean", _d3), ("violating", _i64_3), ("n_success", C.c_int64)]


# the list arrays and the carries of both structs, in order, with their dtypes; the last three of each group exist with costs only
EPISODE_LIST_KEYS = (("episode_index", np.int32), ("episode_return", np.float64), ("episode_length", np.int32), ("episode_ordinal", np.int32),
                     ("episode_flags", np.int32), ("episode_cost", np.float64), ("episode_violating", np.int32), ("episode_any_violating", np.int32))
EPISODE_CARRY_KEYS = (("ep_return", np.float64), ("ep_length", np.int32), ("ep_ordinal", np.int32), ("ep_partial", np.uint8),
                      ("ep_cost", np.float64), ("ep_violating", np.int32), ("ep_any_violating", np.int32))


class gs_rollout_episodes_dev(C.Structure):
    _fields_ = ([("n_episodes", C.c_int32), ("B", C.c_int32), ("with_costs", C.c_int32), ("cost_stride", C.c_int32)] +
                [(k, C.c_void_p) for k, _ in EPISODE_LIST_KEYS] + [("stats", C.c_void_p)] + [(k, C.c_void_p) for k, _ in EPISODE_CARRY_KEYS])


class gs_rollout_episodes_host(C.Structure):
    _fields_ = ([("n_episodes", C.c_void_p)] + [(k, C.c_void_p) for k, _ in EPISODE_LIST_KEYS] + [("stats", C.c_void_p)] +
                [(k, C.c_void_p) for k, _ in EPISODE_CARRY_KEYS])


def episode_config(start="continue", costs: bool = False, success_return: float = -1000.0, struct_size=None) -> gs_episode_config:
    """gs_episode_config; ``start``: a name of EPISODES_START or its number."""
    return gs_episode_config(C.sizeof(gs_episode_config) if struct_size is None else int(struct_size),
                             EPISODES_START[start] if isinstance(start, str) else int(start), int(bool(costs)), 0, float(success_return))


class gs_dataset_stats_view(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("rows_per_chunk", C.c_int32), ("n", C.c_int64), ("obs_dim", C.c_int32), ("action_dim", C.c_int32),
                ("obs_mean", _dp), ("obs_std", _dp), ("act_mean", _dp), ("act_std", _dp), ("reward_mean", _dp), ("reward_std", _dp)]


class gs_dataset_batch(C.Structure):
    _fields_ = [("observations", C.c_void_p), ("actions", C.c_void_p), ("rewards", C.c_void_p), ("next_observations", C.c_void_p),
                ("terminals", C.c_void_p)]


GS_DATASET_KEEP_STATS = 1
DATASET_KEYS = ("observations", "actions", "rewards", "next_observations", "terminals")      # gs_dataset_batch's fields, in order


# on-policy minibatch epochs (include/gridstep.h): advantage normalisations, the field bits and the structs of gs_onpolicy_*
ADV_NORM = {"none": 0, "rollout": 1, "minibatch": 2}      # GS_ADVNORM_*
# the fields of gs_onpolicy_batch_out, in order, with their GS_ONPOLICY_* bit
ONPOLICY_BATCH_FIELDS = (("observations", 1), ("actions", 2), ("log_probs", 4), ("advantages", 8), ("returns", 16), ("values", 32),
                         ("cost_advantages", 64), ("cost_returns", 128), ("indices", 256))
GS_ONPOLICY_ALL_FIELDS = 511


class gs_onpolicy_batch_config(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("adv_norm", C.c_int32), ("dtype", C.c_int32), ("fields", C.c_uint32), ("lam", _d3),
                ("adv_eps", C.c_double), ("obs_shift", _dp), ("obs_scale", _dp)]


class gs_onpolicy_stats_out(C.Structure):
    _fields_ = [("n", C.c_int64), ("adv_mean", C.c_double), ("adv_std", C.c_double)]


class gs_onpolicy_batch_out(C.Structure):
    _fields_ = [("observations", C.c_void_p), ("actions", C.c_void_p), ("log_probs", C.c_void_p), ("advantages", C.c_void_p),
                ("returns", C.c_void_p), ("values", C.c_void_p), ("cost_advantages", _vp3), ("cost_returns", _vp3),
                ("indices", C.c_void_p), ("adv_stats", C.c_void_p)]


def onpolicy_fields(fields) -> int:
    """The GS_ONPOLICY_* mask of ``fields``: None (all), the mask itself, or names of ONPOLICY_BATCH_FIELDS."""
    if fields is None:
        return GS_ONPOLICY_ALL_FIELDS
    if isinstance(fields, (int, np.integer)):
        return int(fields)
    bits = dict(ONPOLICY_BATCH_FIELDS)
    unknown = [k for k in fields if k not in bits]
    if unknown:
        raise PowerFlowError(f"on-policy batch: unknown field(s) {unknown}; any of {[k for k, _ in ONPOLICY_BATCH_FIELDS]}")
    return sum(bits[k] for k in set(fields))


# the learner (include/gridstep.h "the learner"): GS_LEARNER_*, and the structs of gs_learner_*
GS_LEARNER_POLICY, GS_LEARNER_VALUE, GS_LEARNER_COST_VALUE = 0, 1, 2
LEARNER_STATS = ("loss", "surrogate", "entropy", "approx_kl", "clip_fraction", "value_loss", "grad_norm", "step")


class gs_learner_config(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("reserved", C.c_int32), ("lr", C.c_double), ("beta1", C.c_double), ("beta2", C.c_double),
                ("eps", C.c_double), ("weight_decay", C.c_double), ("max_grad_norm", C.c_double), ("clip", C.c_double), ("ent_coef", C.c_double)]


class gs_learner_stats_out(C.Structure):
    _fields_ = [(k, C.c_double) for k in LEARNER_STATS]


class gs_learner_info_out(C.Structure):
    _fields_ = [("n_layers", C.c_int32), ("activation", C.c_int32), ("dims", C.c_int32 * 5), ("rows_per_segment", C.c_int32),
                ("param_count", C.c_int64), ("step", C.c_int64)]


class gs_learner_view_out(C.Structure):
    _fields_ = [("n", C.c_int32), ("reserved", C.c_int32), ("log_probs_new", C.c_void_p), ("ratio", C.c_void_p), ("clipped", C.c_void_p),
                ("loss_terms", C.c_void_p), ("entropy_terms", C.c_void_p)]


# the learner's loss (include/gridstep.h "the learner's loss"): GS_LOSS_* and the struct of gs_learner_set_loss / _get_loss
GS_LOSS_DEFAULT, GS_LOSS_AWR, GS_LOSS_EXPECTILE = 0, 1, 2
LOSS_KINDS = {"default": GS_LOSS_DEFAULT, "awr": GS_LOSS_AWR, "expectile": GS_LOSS_EXPECTILE}


class gs_learner_loss(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("kind", C.c_int32), ("temperature", C.c_double), ("weight_max", C.c_double),
                ("expectile", C.c_double)]


def learner_loss(kind="default", temperature=1.0, weight_max=20.0, expectile=0.7, struct_size=None) -> gs_learner_loss:
    """A ``gs_learner_loss``: ``kind`` a name of ``LOSS_KINDS`` or a GS_LOSS_* number."""
    if isinstance(kind, str):
        if kind not in LOSS_KINDS:
            raise ValueError(f"learner loss: unknown kind {kind!r}; one of {sorted(LOSS_KINDS)}")
        kind = LOSS_KINDS[kind]
    return gs_learner_loss(C.sizeof(gs_learner_loss) if struct_size is None else int(struct_size), int(kind), float(temperature),
                           float(weight_max), float(expectile))


# state-action critics (include/gridstep.h "state-action critics"): GS_LEARNER_Q, GS_SIGNAL_* and the structs of gs_rollout_*_q
GS_LEARNER_Q = 5            # + which
GS_SIGNAL_BATCH, GS_SIGNAL_Q = 0, 1
SIGNALS = {"batch": GS_SIGNAL_BATCH, "q": GS_SIGNAL_Q}
Q_NETS = ("q1", "q2")       # the names of GS_LEARNER_Q + 0 and + 1


class gs_q_eval_config(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("bootstrap_mask", C.c_int32), ("gamma", C.c_double), ("reward_shift", C.c_double),
                ("reward_scale", C.c_double)]


class gs_rollout_q(C.Structure):
    _fields_ = [("T", C.c_int32), ("B", C.c_int32), ("installed", C.c_int32), ("rows_per_tile", C.c_int32),
                ("q", (C.c_void_p * 2) * 2), ("q_min", C.c_void_p * 2), ("q_adv", C.c_void_p), ("td_target", C.c_void_p)]


class gs_rollout_q_host(C.Structure):
    _fields_ = [("q", (_dp * 2) * 2), ("q_min", _dp * 2), ("q_adv", _dp), ("td_target", _dp)]


Q_SOURCES = ("online", "target")      # the first index of gs_rollout_q.q and of q_min


def q_which(which) -> int:
    """0 or 1 from a twin's number or its name in ``Q_NETS``."""
    if which in Q_NETS:
        return Q_NETS.index(which)
    if isinstance(which, (int, np.integer)) and not isinstance(which, bool) and 0 <= int(which) <= 1:
        return int(which)
    raise ValueError(f"Q network: which = {which!r} must be 0, 1 or one of {Q_NETS}")


# the pathwise actor step (include/gridstep.h "the pathwise actor step"): the structs of gs_learner_step_pathwise / _pathwise_view
PATHWISE_NOISE_TAG = 0x50574E4F      # 'PWNO'


class gs_pathwise_config(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("stochastic", C.c_int32), ("alpha", C.c_double), ("bc_coef", C.c_double), ("seed", C.c_uint64),
                ("draw", C.c_uint32), ("reserved", C.c_uint32)]


class gs_pathwise_view_out(C.Structure):
    _fields_ = [("n", C.c_int32), ("action_dim", C.c_int32), ("installed", C.c_int32), ("pre_head_stride", C.c_int32), ("pre_head", C.c_void_p),
                ("actions", C.c_void_p),
                ("noise", C.c_void_p), ("log_probs", C.c_void_p), ("q", C.c_void_p * 2), ("q_min", C.c_void_p), ("bc_terms", C.c_void_p),
                ("loss_terms", C.c_void_p), ("which", C.c_void_p), ("dq_da", C.c_void_p * 2)]


def pathwise_config(alpha=0.0, bc_coef=0.0, stochastic=True, seed=0, draw=0, struct_size=None) -> gs_pathwise_config:
    return gs_pathwise_config(C.sizeof(gs_pathwise_config) if struct_size is None else int(struct_size), int(stochastic), float(alpha),
                              float(bc_coef), int(seed) & 0xFFFFFFFFFFFFFFFF, int(draw) & 0xFFFFFFFF, 0)


# the conservative critic step (include/gridstep.h "the conservative critic step"): the tags and the structs of
# gs_learner_step_conservative / _conservative_view
CQL_UNIFORM_TAG = 0x43514C55         # 'CQLU'
CQL_NOISE_TAG = 0x43514C4E           # 'CQLN'
CQL_MAX_N = (1 << 24) // 3


class gs_conservative_config(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("stochastic", C.c_int32), ("conservative_weight", C.c_double), ("seed", C.c_uint64),
                ("draw", C.c_uint32), ("reserved", C.c_uint32)]


class gs_conservative_view_out(C.Structure):
    _fields_ = [("net", C.c_int32), ("n", C.c_int32), ("action_dim", C.c_int32), ("pre_head_stride", C.c_int32), ("pre_head", C.c_void_p),
                ("random_actions", C.c_void_p), ("policy_actions", C.c_void_p), ("policy_noise", C.c_void_p), ("policy_log_probs", C.c_void_p),
                ("targets", C.c_void_p), ("q", C.c_void_p), ("weights", C.c_void_p), ("loss_terms", C.c_void_p), ("scalars", C.c_void_p)]


def conservative_config(conservative_weight=5.0, stochastic=True, seed=0, draw=0, struct_size=None) -> gs_conservative_config:
    return gs_conservative_config(C.sizeof(gs_conservative_config) if struct_size is None else int(struct_size), int(stochastic),
                                  float(conservative_weight), int(seed) & 0xFFFFFFFFFFFFFFFF, int(draw) & 0xFFFFFFFF, 0)


# policy-action TD targets (include/gridstep.h "policy-action TD targets"): GS_Q_TARGET_*, the noise tags and the structs of
# gs_rollout_evaluate_q_next / gs_rollout_q_next_*
GS_Q_TARGET_VALUE, GS_Q_TARGET_POLICY = 0, 1
Q_TARGETS = {"value": GS_Q_TARGET_VALUE, "policy": GS_Q_TARGET_POLICY}
Q_NEXT_ROLLOUT_TAG = 0x514E5854       # 'QNXT'
Q_NEXT_TERMINAL_TAG = 0x514E5445      # 'QNTE'
_fp = C.POINTER(C.c_float)


class gs_q_next_config(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("bootstrap_mask", C.c_int32), ("stochastic", C.c_int32), ("reserved", C.c_int32),
                ("gamma", C.c_double), ("alpha", C.c_double), ("reward_shift", C.c_double), ("reward_scale", C.c_double),
                ("seed", C.c_uint64), ("draw", C.c_uint32), ("reserved2", C.c_uint32)]


class gs_rollout_q_next(C.Structure):
    _fields_ = [("T", C.c_int32), ("B", C.c_int32), ("installed", C.c_int32), ("rows_per_tile", C.c_int32), ("action_dim", C.c_int32),
                ("terminal_capacity", C.c_int32), ("next_pre_head", C.c_void_p), ("next_actions", C.c_void_p), ("next_noise", C.c_void_p), ("next_log_probs", C.c_void_p),
                ("q_next", C.c_void_p * 2), ("q_next_min", C.c_void_p), ("td_target", C.c_void_p), ("term_pre_head", C.c_void_p),
                ("term_actions", C.c_void_p), ("term_noise", C.c_void_p), ("term_log_probs", C.c_void_p), ("term_q", C.c_void_p * 2), ("term_q_min", C.c_void_p),
                ("term_value", C.c_void_p)]


class gs_rollout_q_next_host(C.Structure):
    _fields_ = [("next_pre_head", _fp), ("next_actions", _dp), ("next_noise", _dp), ("next_log_probs", _dp), ("q_next", _dp * 2), ("q_next_min", _dp),
                ("td_target", _dp), ("term_pre_head", _fp), ("term_actions", _dp), ("term_noise", _dp), ("term_log_probs", _dp), ("term_q", _dp * 2),
                ("term_q_min", _dp), ("term_value", _dp)]


def q_next_config(gamma=0.99, alpha=0.0, bootstrap_mask=0, stochastic=True, seed=0, draw=0, reward_shift=0.0, reward_scale=1.0,
                  struct_size=None) -> gs_q_next_config:
    return gs_q_next_config(C.sizeof(gs_q_next_config) if struct_size is None else int(struct_size), int(bootstrap_mask), int(stochastic), 0,
                            float(gamma), float(alpha), float(reward_shift), float(reward_scale), int(seed) & 0xFFFFFFFFFFFFFFFF,
                            int(draw) & 0xFFFFFFFF, 0)


# per-minibatch targets (include/gridstep.h "per-minibatch targets"): the groups and the config of gs_learner_refresh
GS_REFRESH_TD_POLICY, GS_REFRESH_Q_TARGET, GS_REFRESH_TD_VALUE, GS_REFRESH_Q_ADV = 1, 2, 4, 8
REFRESH_GROUPS = {"td_policy": GS_REFRESH_TD_POLICY, "q_target": GS_REFRESH_Q_TARGET, "td_value": GS_REFRESH_TD_VALUE, "q_adv": GS_REFRESH_Q_ADV}


class gs_refresh_config(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("groups", C.c_int32), ("bootstrap_mask", C.c_int32), ("stochastic", C.c_int32),
                ("gamma", C.c_double), ("alpha", C.c_double), ("reward_shift", C.c_double), ("reward_scale", C.c_double),
                ("seed", C.c_uint64), ("draw", C.c_uint32), ("reserved", C.c_uint32), ("reserved2", C.c_uint64)]


def refresh_groups(groups) -> int:
    """GS_REFRESH_* bits from a name of ``REFRESH_GROUPS``, a sequence of names, or the number (an unknown bit is the library's to
    refuse)."""
    if isinstance(groups, str):
        groups = (groups,)
    if isinstance(groups, (bool, np.bool_)):
        raise ValueError(f"refresh: groups = {groups!r} is neither a name, a sequence of names nor the bits")
    if isinstance(groups, (int, np.integer)):
        return int(groups)
    bits = 0
    for g in groups:
        if g not in REFRESH_GROUPS:
            raise ValueError(f"refresh: unknown group {g!r}; one of {sorted(REFRESH_GROUPS)}")
        bits |= REFRESH_GROUPS[g]
    return bits


def refresh_config(groups, gamma=0.99, alpha=0.0, bootstrap_mask=0, stochastic=True, seed=0, draw=0, reward_shift=0.0, reward_scale=1.0,
                   struct_size=None) -> gs_refresh_config:
    return gs_refresh_config(C.sizeof(gs_refresh_config) if struct_size is None else int(struct_size), refresh_groups(groups), int(bootstrap_mask),
                             int(stochastic), float(gamma), float(alpha), float(reward_shift), float(reward_scale), int(seed) & 0xFFFFFFFFFFFFFFFF,
                             int(draw) & 0xFFFFFFFF, 0, 0)


def q_target_number(source) -> int:
    """GS_Q_TARGET_* from its name in ``Q_TARGETS`` or its number (an unknown number is the library's to refuse)."""
    if isinstance(source, str):
        if source not in Q_TARGETS:
            raise ValueError(f"Q target: unknown source {source!r}; one of {sorted(Q_TARGETS)}")
        return Q_TARGETS[source]
    return int(source)


# the federation (include/gridstep.h "the federation"): the structs of gs_fed_*
GS_FED_MAX_CLIENTS = 32
_FED = C.c_void_p


class gs_fed_info_out(C.Structure):
    _fields_ = [("n_clients", C.c_int32), ("net", C.c_int32), ("param_count", C.c_int64), ("rounds", C.c_int64), ("block_params", C.c_int32),
                ("reserved", C.c_int32)]


class gs_fed_round(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("n_participants", C.c_int32), ("participants", C.POINTER(C.c_int32)), ("weights", C.POINTER(C.c_double)),
                ("clip_norm", C.c_double), ("noise_std", C.c_double), ("server_lr", C.c_double), ("seed", C.c_uint64), ("round", C.c_uint32),
                ("reset_moments", C.c_int32)]


class gs_fed_stats_out(C.Structure):
    _fields_ = [("norm", C.c_double * GS_FED_MAX_CLIENTS), ("clip_scale", C.c_double * GS_FED_MAX_CLIENTS),
                ("coefficient", C.c_double * GS_FED_MAX_CLIENTS), ("noise_std", C.c_double), ("rounds", C.c_int64), ("round", C.c_uint32),
                ("n", C.c_int32)]


# parameter anchors (include/gridstep.h "parameter anchors"): GS_ANCHOR_* and the structs of gs_learner_anchor_* / gs_learner_fisher_*
GS_ANCHOR_PROX, GS_ANCHOR_EWC = 1, 2
ANCHOR_SLOTS = {"prox": GS_ANCHOR_PROX, "ewc": GS_ANCHOR_EWC, "both": GS_ANCHOR_PROX | GS_ANCHOR_EWC}
ANCHOR_ARRAYS = ("prox", "ewc_importance", "ewc_centre", "fisher_pending")      # gs_learner_anchor_download's, in argument order


class gs_learner_anchor_config(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("reserved", C.c_int32), ("prox_mu", C.c_double), ("ewc_lambda", C.c_double)]


class gs_fisher_config(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("reserved", C.c_int32), ("min_importance", C.c_double), ("decay", C.c_double)]


class gs_learner_anchor_stats_out(C.Structure):
    _fields_ = [("penalty_prox", C.c_double), ("penalty_ewc", C.c_double), ("grad_norm_loss", C.c_double), ("prox_mu", C.c_double),
                ("ewc_lambda", C.c_double), ("tasks", C.c_int64), ("fisher_samples", C.c_int64)]


def anchor_config(prox_mu=0.0, ewc_lambda=0.0, struct_size=None) -> gs_learner_anchor_config:
    return gs_learner_anchor_config(C.sizeof(gs_learner_anchor_config) if struct_size is None else int(struct_size), 0, float(prox_mu),
                                    float(ewc_lambda))


def fisher_config(min_importance=1e-3, decay=1.0, struct_size=None) -> gs_fisher_config:
    return gs_fisher_config(C.sizeof(gs_fisher_config) if struct_size is None else int(struct_size), 0, float(min_importance), float(decay))


def anchor_check(c: Optional[gs_learner_anchor_config]) -> Tuple[int, str]:
    """gs_learner_anchor_check: (return code, message) -- the value rules of the anchors' coefficients on the host alone (no GPU)."""
    return _host_check("gs_learner_anchor_check", None if c is None else C.byref(c))


def learner_net(net) -> int:
    """The GS_LEARNER_* number of ``net``: "policy", "value", a cost channel's name (``COST_CHANNELS``), a twin Q network's name
    (``Q_NETS``), or the number itself for the policy and the state critics (the Q networks go by name)."""
    if isinstance(net, (int, np.integer)) and not isinstance(net, bool):
        if not 0 <= int(net) < 2 + len(COST_CHANNELS):
            raise ValueError(f"learner: net {int(net)} outside 0 .. {1 + len(COST_CHANNELS)}")
        return int(net)
    if net == "policy":
        return GS_LEARNER_POLICY
    if net == "value":
        return GS_LEARNER_VALUE
    if net in COST_CHANNELS:
        return GS_LEARNER_COST_VALUE + COST_CHANNELS.index(net)
    if net in Q_NETS:
        return GS_LEARNER_Q + Q_NETS.index(net)
    raise ValueError(f"learner: unknown network {net!r}; 'policy', 'value' or one of {COST_CHANNELS + Q_NETS}")


def _net_number(net) -> int:
    """``learner_net`` for the ``Handle``'s methods, which also take the numbers ``learner_net`` gave for the Q networks' names"""
    if isinstance(net, (int, np.integer)) and not isinstance(net, bool) and GS_LEARNER_Q <= int(net) < GS_LEARNER_Q + len(Q_NETS):
        return int(net)
    return learner_net(net)


def learner_config(lr=3e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, clip=0.2, ent_coef=0.0, max_grad_norm=0.0,
                   struct_size=None) -> gs_learner_config:
    return gs_learner_config(C.sizeof(gs_learner_config) if struct_size is None else int(struct_size), 0, float(lr), float(betas[0]),
                             float(betas[1]), float(eps), float(weight_decay), float(max_grad_norm), float(clip), float(ent_coef))


# every symbol include/gridstep.h declares: (name, restype, argtypes)
_H = C.c_void_p
SYMBOLS = [
    ("gs_version", C.c_int, []),
    ("gs_build_experiments", C.c_int, []),
    ("gs_device_count", C.c_int, []),
    ("gs_last_error", C.c_char_p, [_H]),
    ("gs_create", C.c_int, [C.POINTER(gs_topology), C.POINTER(gs_config), C.c_int32, C.c_int32, C.c_int64, C.POINTER(_H)]),
    ("gs_destroy", None, [_H]),
    ("gs_dims", C.c_int, [_H, _ip, _ip, _ip, _ip, _ip, _ip]),
    ("gs_describe", C.c_int, [_H, C.c_char_p, C.c_int32]),
    ("gs_plan_describe", C.c_int, [C.POINTER(gs_topology), C.POINTER(gs_config), C.c_int32, C.c_int32, C.c_char_p, C.c_int32]),
    ("gs_synchronize", C.c_int, [_H]),
    ("gs_solve", C.c_int, [_H, _dp, _dp, C.POINTER(gs_solution_view)]),
    ("gs_upload_injections", C.c_int, [_H, _dp, _dp]),
    ("gs_solve_device", C.c_int, [_H]),
    ("gs_download_solution", C.c_int, [_H, C.POINTER(gs_solution_view)]),
    ("gs_reset", C.c_int, [_H, C.POINTER(C.c_uint64), _up, _dp]),
    ("gs_step", C.c_int, [_H, _dp, _dp, _dp, _up, _up, C.POINTER(gs_info_view)]),
    ("gs_upload_actions", C.c_int, [_H, _dp, C.c_int32]),
    ("gs_step_device", C.c_int, [_H, C.c_int32]),
    ("gs_download_step", C.c_int, [_H, _dp, _dp, _up, _up, C.POINTER(gs_info_view)]),
    ("gs_step_f32", C.c_int, [_H, _dp, C.POINTER(C.c_float), _dp, _up, _up, C.POINTER(gs_info_view)]),
    ("gs_download_step_f32", C.c_int, [_H, C.POINTER(C.c_float), _dp, _up, _up, C.POINTER(gs_info_view)]),
    ("gs_rollout", C.c_int, [_H, C.c_int32, C.c_int32, C.c_uint64, _dp]),
    ("gs_rollout_download", C.c_int, [_H, C.POINTER(gs_rollout_view)]),
    ("gs_rollout_device_view", C.c_int, [_H, C.POINTER(gs_rollout_device)]),
    ("gs_rollout_load_check", C.c_int, [C.POINTER(gs_rollout_source), C.c_int32, C.c_int32, C.c_int32, C.POINTER(gs_rollout_load_info)]),
    ("gs_rollout_load", C.c_int, [_H, C.POINTER(gs_rollout_source)]),
    ("gs_rollout_continue", C.c_int, [_H, C.POINTER(gs_rollout_continue_config)]),
    ("gs_rollout_window_info", C.c_int, [_H, C.POINTER(gs_rollout_window_info_out)]),
    ("gs_dataset_build", C.c_int, [_H, C.c_uint32]),
    ("gs_dataset_stats", C.c_int, [_H, C.POINTER(gs_dataset_stats_view)]),
    ("gs_dataset_set_stats", C.c_int, [_H, C.POINTER(gs_dataset_stats_view)]),
    ("gs_dataset_sample", C.c_int, [_H, C.c_int32, C.POINTER(C.c_int64), C.c_uint64, C.c_uint64, C.c_int32, C.c_int32,
                                    C.POINTER(gs_dataset_batch), C.c_void_p]),
    ("gs_get_state", C.c_int, [_H, _dp]),
    ("gs_set_state", C.c_int, [_H, _dp]),
    ("gs_comm_unique_id", C.c_int, [_up]),
    ("gs_comm_init", C.c_int, [_H, _up, C.c_int32, C.c_int32]),
    ("gs_allgather_obs", C.c_int, [_H, _dp]),
    ("gs_comm_destroy", C.c_int, [_H]),
    ("gs_comm_info", C.c_int, [_H, C.c_void_p]),
    ("gs_host_obs_bind", C.c_int, [_H, _dp]),
    ("gs_host_obs_unbind", C.c_int, [_H, _dp]),
    ("gs_flat_newton_map_dump", C.c_int, [C.c_void_p, C.c_int32, _dp]),
    ("gs_mesh_schedule_dump_packed", C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _ip, _ip, _ip, _dp, _ip]),
    ("gs_mesh_schedule_dump", C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _ip, C.c_char_p, C.c_int32,
                                        C.c_void_p, _ip, _ip, _dp]),
    ("gs_comm_init_loopback", C.c_int, [C.POINTER(_H), C.c_int32]),
    ("gs_allgather_obs_shards", C.c_int, [C.POINTER(_H), C.c_int32, _dp]),
    ("gs_allgather_obs_view", C.c_int, [_H, C.c_void_p, C.c_void_p]),
    ("gs_allgather_obs_download", C.c_int, [_H, _dp]),
    ("gs_timing_enable", C.c_int, [_H, C.c_int32]),
    ("gs_timing_read", C.c_int, [_H, _dp, C.POINTER(C.c_int64)]),
    ("gs_step_device_ptr", C.c_int, [_H, C.c_void_p, C.c_void_p]),
    ("gs_step_device_view", C.c_int, [_H, C.c_void_p, C.c_void_p]),
    ("gs_host_alloc", C.c_int, [C.POINTER(C.c_void_p), C.c_size_t]),
    ("gs_host_free", C.c_int, [C.c_void_p]),
    ("gs_debug_stamps", C.c_int, [_H, C.POINTER(C.c_uint64), C.c_int32]),
    ("gs_debug_block_times", C.c_int, [_H, C.POINTER(C.c_uint64), C.c_int32]),
    ("gs_debug_write_rows", C.c_int, [_H, C.c_int32, _dp]),
    ("gs_debug_read_rows", C.c_int, [_H, C.c_int32, _dp]),
    ("gs_debug_fastmath", C.c_int, [C.c_int32, C.c_int64, _dp, _dp, _dp]),
    ("gs_fallback_linear", C.c_int, [_H, _dp, _dp, _dp, _dp, _up, _up, C.POINTER(C.c_int32)]),
    ("gs_set_line_impedances", C.c_int, [_H, _dp, _dp, _up]),
    ("gs_get_line_impedances", C.c_int, [_H, _dp, _dp]),
    ("gs_set_load_powers", C.c_int, [_H, _dp, _up]),
    ("gs_get_load_powers", C.c_int, [_H, _dp]),
    ("gs_policy_mlp_check", C.c_int, [C.POINTER(gs_policy_mlp), C.c_int32, C.c_int32]),
    ("gs_policy_mlp_set", C.c_int, [_H, C.POINTER(gs_policy_mlp)]),
    ("gs_policy_mlp_eval", C.c_int, [_H, C.c_uint64, C.c_int32, _dp]),
    ("gs_policy_mlp_check_opts", C.c_int, [C.POINTER(gs_policy_mlp), C.POINTER(gs_policy_mlp_opts), C.c_int32, C.c_int32]),
    ("gs_policy_mlp_set_opts", C.c_int, [_H, C.POINTER(gs_policy_mlp), C.POINTER(gs_policy_mlp_opts)]),
    ("gs_rollout_set_log_probs", C.c_int, [_H, C.c_int32]),
    ("gs_value_mlp_check", C.c_int, [C.POINTER(gs_policy_mlp), C.POINTER(gs_policy_mlp_opts), C.c_int32]),
    ("gs_value_mlp_set", C.c_int, [_H, C.POINTER(gs_policy_mlp), C.POINTER(gs_policy_mlp_opts)]),
    ("gs_value_mlp_eval", C.c_int, [_H, _dp]),
    ("gs_rollout_evaluate", C.c_int, [_H, C.POINTER(gs_gae_config)]),
    ("gs_rollout_onpolicy_view", C.c_int, [_H, C.POINTER(gs_rollout_onpolicy), C.c_void_p]),
    ("gs_rollout_onpolicy_download", C.c_int, [_H, C.POINTER(gs_rollout_onpolicy_host)]),
    ("gs_cost_config_default", C.c_int, [_H, C.POINTER(gs_cost_config)]),
    ("gs_cost_config_check", C.c_int, [C.POINTER(gs_cost_config)]),
    ("gs_rollout_costs", C.c_int, [_H, C.POINTER(gs_cost_config)]),
    ("gs_costs_eval", C.c_int, [_H, C.POINTER(gs_cost_config), _dp, C.c_int32, _dp, _ip, _dp]),
    ("gs_cost_value_mlp_set", C.c_int, [_H, C.c_int32, C.POINTER(gs_policy_mlp), C.POINTER(gs_policy_mlp_opts)]),
    ("gs_rollout_evaluate_costs", C.c_int, [_H, C.POINTER(gs_cost_gae_config)]),
    ("gs_rollout_costs_view", C.c_int, [_H, C.POINTER(gs_rollout_costs_dev), C.c_void_p]),
    ("gs_rollout_costs_download", C.c_int, [_H, C.POINTER(gs_rollout_costs_host)]),
    ("gs_rollout_episodes", C.c_int, [_H, C.POINTER(gs_episode_config)]),
    ("gs_rollout_episodes_view", C.c_int, [_H, C.POINTER(gs_rollout_episodes_dev), C.c_void_p]),
    ("gs_rollout_episodes_download", C.c_int, [_H, C.POINTER(gs_rollout_episodes_host)]),
    ("gs_episodes_clear", C.c_int, [_H]),
    ("gs_onpolicy_prepare", C.c_int, [_H, C.POINTER(gs_onpolicy_batch_config)]),
    ("gs_onpolicy_stats", C.c_int, [_H, C.POINTER(gs_onpolicy_stats_out)]),
    ("gs_onpolicy_batch", C.c_int, [_H, C.c_uint64, C.c_uint32, C.c_int64, C.c_int32, C.POINTER(gs_onpolicy_batch_out), C.c_void_p]),
    ("gs_learner_create", C.c_int, [_H, C.c_int32, C.POINTER(gs_learner_config)]),
    ("gs_learner_step", C.c_int, [_H, C.c_int32, C.POINTER(gs_onpolicy_batch_out), C.c_int32, C.c_void_p]),
    ("gs_learner_stats", C.c_int, [_H, C.c_int32, C.POINTER(gs_learner_stats_out)]),
    ("gs_learner_info", C.c_int, [_H, C.c_int32, C.POINTER(gs_learner_info_out)]),
    ("gs_learner_download", C.c_int, [_H, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("gs_learner_view", C.c_int, [_H, C.c_int32, C.POINTER(gs_learner_view_out), C.c_void_p]),
    ("gs_learner_set_loss", C.c_int, [_H, C.c_int32, C.POINTER(gs_learner_loss)]),
    ("gs_learner_get_loss", C.c_int, [_H, C.c_int32, C.POINTER(gs_learner_loss)]),
    ("gs_q_mlp_check", C.c_int, [C.POINTER(gs_policy_mlp), C.POINTER(gs_policy_mlp_opts), C.c_int32, C.c_int32]),
    ("gs_q_mlp_set", C.c_int, [_H, C.c_int32, C.POINTER(gs_policy_mlp), C.POINTER(gs_policy_mlp_opts)]),
    ("gs_rollout_evaluate_q", C.c_int, [_H, C.POINTER(gs_q_eval_config)]),
    ("gs_rollout_q_view", C.c_int, [_H, C.POINTER(gs_rollout_q), C.c_void_p]),
    ("gs_rollout_q_download", C.c_int, [_H, C.POINTER(gs_rollout_q_host)]),
    ("gs_learner_set_signal", C.c_int, [_H, C.c_int32, C.c_int32]),
    ("gs_learner_get_signal", C.c_int, [_H, C.c_int32, C.POINTER(C.c_int32)]),
    ("gs_q_target_update", C.c_int, [_H, C.c_double]),
    ("gs_q_target_download", C.c_int, [_H, C.c_int32, C.c_void_p]),
    ("gs_rollout_evaluate_q_next", C.c_int, [_H, C.POINTER(gs_q_next_config)]),
    ("gs_rollout_q_next_view", C.c_int, [_H, C.POINTER(gs_rollout_q_next), C.c_void_p]),
    ("gs_rollout_q_next_download", C.c_int, [_H, C.POINTER(gs_rollout_q_next_host)]),
    ("gs_q_set_target_source", C.c_int, [_H, C.c_int32]),
    ("gs_q_get_target_source", C.c_int, [_H, C.POINTER(C.c_int32)]),
    ("gs_learner_step_pathwise", C.c_int, [_H, C.POINTER(gs_onpolicy_batch_out), C.c_int32, C.POINTER(gs_pathwise_config), C.c_void_p]),
    ("gs_learner_pathwise_view", C.c_int, [_H, C.POINTER(gs_pathwise_view_out), C.c_void_p]),
    ("gs_learner_step_conservative", C.c_int, [_H, C.c_int32, C.POINTER(gs_onpolicy_batch_out), C.c_int32, C.POINTER(gs_conservative_config), C.c_void_p]),
    ("gs_learner_conservative_view", C.c_int, [_H, C.POINTER(gs_conservative_view_out), C.c_void_p]),
    ("gs_learner_refresh", C.c_int, [_H, C.POINTER(gs_onpolicy_batch_out), C.c_int32, C.POINTER(gs_refresh_config), C.c_void_p]),
    ("gs_fed_create", C.c_int, [C.POINTER(_H), C.c_int32, C.c_int32, C.POINTER(_FED)]),
    ("gs_fed_destroy", C.c_int, [_FED]),
    ("gs_fed_info", C.c_int, [_FED, C.POINTER(gs_fed_info_out)]),
    ("gs_fed_set_global", C.c_int, [_FED, C.c_void_p]),
    ("gs_fed_measure", C.c_int, [_FED, C.POINTER(C.c_int32), C.c_int32, C.POINTER(C.c_double)]),
    ("gs_fed_aggregate", C.c_int, [_FED, C.POINTER(gs_fed_round)]),
    ("gs_fed_stats", C.c_int, [_FED, C.POINTER(gs_fed_stats_out)]),
    ("gs_fed_download", C.c_int, [_FED, C.c_void_p]),
    ("gs_learner_anchor_check", C.c_int, [C.POINTER(gs_learner_anchor_config)]),
    ("gs_learner_anchor_here", C.c_int, [_H, C.c_int32, C.c_void_p]),
    ("gs_learner_anchor_set", C.c_int, [_H, C.c_int32, C.POINTER(gs_learner_anchor_config)]),
    ("gs_learner_anchor_get", C.c_int, [_H, C.c_int32, C.POINTER(gs_learner_anchor_config)]),
    ("gs_learner_fisher_begin", C.c_int, [_H, C.c_int32]),
    ("gs_learner_fisher_accumulate", C.c_int, [_H, C.c_int32, C.POINTER(gs_onpolicy_batch_out), C.c_int32, C.c_void_p]),
    ("gs_learner_fisher_commit", C.c_int, [_H, C.c_int32, C.POINTER(gs_fisher_config)]),
    ("gs_learner_anchor_clear", C.c_int, [_H, C.c_int32, C.c_int32]),
    ("gs_learner_anchor_stats", C.c_int, [_H, C.c_int32, C.POINTER(gs_learner_anchor_stats_out)]),
    ("gs_learner_anchor_download", C.c_int, [_H, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
]
# the gs3_* entry points (three-phase solver) are bound in unbalanced.py


_lib: Optional[C.CDLL] = None


def load() -> C.CDLL:
    """Load libgridstep.so and bind every declared symbol; raises if the library is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise PowerFlowError(
            f"{LIB_PATH} not found: the HIP extension has not been built "
            "(run __graft_entry__.build() or `make -C grid_fed_rl_gym_amd/csrc`). There is no CPU fallback.")
    lib = C.CDLL(LIB_PATH)
    for name, res, args in SYMBOLS:
        fn = getattr(lib, name)       # AttributeError if the .so lacks a declared symbol
        fn.restype = res
        fn.argtypes = args
    if lib.gs_version() != GS_ABI_VERSION:
        raise PowerFlowError(f"libgridstep ABI {lib.gs_version()} != binding {GS_ABI_VERSION}")
    _lib = lib
    return lib


def experiments() -> bool:
    """True if libgridstep.so was built with ``make EXPERIMENTS=1`` (gs_build_experiments)."""
    return bool(load().gs_build_experiments())


def _f64(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float64)


def _i32(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.int32)


def _ptr(a: Optional[np.ndarray], typ):
    return None if a is None else a.ctypes.data_as(typ)


def rollout_source(B: int, obs_dim: int, action_dim: int, observations, actions, rewards, next_observations, terminals,
                   final_observation=None, log_probs=None, chunk_rows: int = 0):
    """(gs_rollout_source, the arrays it points into) for ``Handle.rollout_load`` and ``rollout_load_check``: shapes checked against
    ``[T, B, ...]``, one floating dtype (float64 or float32) for all, nothing copied that is C-contiguous already."""
    obs = np.asarray(observations)
    if obs.dtype not in (np.float64, np.float32):
        raise PowerFlowError(f"rollout_load: observations are {obs.dtype}; float64 or float32 (convert other types yourself: the loader does not guess)")
    if obs.ndim != 3 or obs.shape[1:] != (B, obs_dim) or obs.shape[0] < 1:
        raise PowerFlowError(f"rollout_load: observations shape {obs.shape} != (T, {B}, {obs_dim})")
    T = int(obs.shape[0])
    want = dict(observations=(obs, (T, B, obs_dim)), next_observations=(next_observations, (T, B, obs_dim)), rewards=(rewards, (T, B)),
                actions=(actions, (T, B, action_dim)), final_observation=(final_observation, (B, obs_dim)), log_probs=(log_probs, (T, B)))
    keep = {}
    for k, (a, shape) in want.items():
        if a is None:
            if k in ("final_observation", "log_probs") or (k == "actions" and action_dim == 0):
                continue
            raise PowerFlowError(f"rollout_load: {k} is None")
        a = np.asarray(a)
        if a.dtype != obs.dtype:
            raise PowerFlowError(f"rollout_load: {k} is {a.dtype}, observations are {obs.dtype}: the floating arrays share one dtype, float64 or float32")
        if a.shape != shape:
            raise PowerFlowError(f"rollout_load: {k} shape {a.shape} != {shape}")
        keep[k] = np.ascontiguousarray(a)
    term = np.asarray(terminals)
    if term.dtype == np.bool_:
        term = term.astype(np.uint8)          # (True: bit 0, terminated)
    if term.dtype != np.uint8:
        raise PowerFlowError(f"rollout_load: terminals are {term.dtype}; uint8 flags (bit 0 terminated, bit 1 truncated) or bool")
    if term.shape != (T, B):
        raise PowerFlowError(f"rollout_load: terminals shape {term.shape} != ({T}, {B})")
    keep["terminals"] = np.ascontiguousarray(term)
    vp = lambda k: None if k not in keep else keep[k].ctypes.data_as(C.c_void_p)
    src = gs_rollout_source(C.sizeof(gs_rollout_source), COMPUTE["float64" if obs.dtype == np.float64 else "float32"], T, int(chunk_rows), 0,
                            vp("observations"), vp("actions"), vp("rewards"), vp("next_observations"), _ptr(keep["terminals"], _up),
                            vp("final_observation"), vp("log_probs"))
    return src, keep


def rollout_load_check(src: gs_rollout_source, B: int, obs_dim: int, action_dim: int) -> dict:
    """gs_rollout_load_check: the host checks of ``gs_rollout_load`` without a handle or a device; ``n``, ``n_terminal`` and
    ``term_cap_needed`` of a source that passes, PowerFlowError with the library's message otherwise."""
    lib = load()
    info = gs_rollout_load_info()
    rc = lib.gs_rollout_load_check(None if src is None else C.byref(src), int(B), int(obs_dim), int(action_dim), C.byref(info))
    if rc != GS_OK:
        raise PowerFlowError(f"libgridstep error {rc}: {lib.gs_last_error(None).decode()}")
    return dict(n=int(info.n), n_terminal=int(info.n_terminal), term_cap_needed=int(info.term_cap_needed))


def make_config(**kw) -> gs_config:
    """gs_config with the reference's constructor defaults (power_flow.py:79-84,
    grid_env.py:161-173, dynamics.py:233-238)."""
    cfg = gs_config()
    cfg.struct_size = C.sizeof(gs_config)
    d = dict(solver_kind=0, jacobian_mode=0, zero_z_mode=0, linear_solver=0, max_iterations=50,
             episode_length=86400, stochastic_loads=0, weather_variation=0, waves_per_group=0, fbs_warm_start=0,
             tolerance=1e-6, acceleration_factor=1.0, timestep=1.0, v_min=0.95, v_max=1.05, f_min=59.5,
             f_max=60.5, safety_penalty=100.0, inertia_H=5.0, damping_D=1.0, f_nominal=60.0, power_base=1.0)
    for k, v in kw.items():
        if k not in d:
            raise TypeError(f"unknown config field {k!r}")
        d[k] = v
    for k, v in d.items():
        setattr(cfg, k, v)
    return cfg


class gs_comm_info_t(C.Structure):
    _fields_ = [("transport", C.c_int32), ("nranks", C.c_int32), ("rank", C.c_int32), ("device", C.c_int32),
                ("comm_device", C.c_int32), ("rccl_version", C.c_int32), ("reserved0", C.c_int32), ("reserved1", C.c_int32),
                ("device_uuid", C.c_uint8 * 16)]


class gs_gathered_obs(C.Structure):
    _fields_ = [("observations", C.c_void_p), ("rows", C.c_int64), ("obs_dim", C.c_int32), ("rank", C.c_int32),
                ("world", C.c_int32), ("reserved", C.c_int32)]


class gs_step_device_out(C.Structure):
    _fields_ = [("observations", C.c_void_p), ("reward", C.c_void_p), ("terminated", C.c_void_p), ("truncated", C.c_void_p),
                ("B", C.c_int32), ("obs_dim", C.c_int32)]


class DeviceArray:
    """A view of device memory owned by a handle: address, shape, dtype, exposed through ``__cuda_array_interface__`` (which
    PyTorch-ROCm and CuPy read as well) so that a consumer on the GPU wraps it without a copy."""

    def __init__(self, ptr: int, shape, typestr: str) -> None:
        self.ptr, self.shape, self.typestr = int(ptr or 0), tuple(int(x) for x in shape), typestr

    @property
    def __cuda_array_interface__(self) -> dict:
        return {"shape": self.shape, "typestr": self.typestr, "data": (self.ptr, False), "version": 3, "strides": None}

    def __repr__(self) -> str:
        return f"DeviceArray(0x{self.ptr:x}, shape={self.shape}, typestr={self.typestr!r})"

    def to_host(self) -> np.ndarray:
        """A host copy (a plain ``hipMemcpy``, which waits for it): for looking at a batch or a view without a GPU framework.  The
        caller orders it behind the producer (a call made without a consumer stream has returned complete)."""
        out = np.empty(self.shape, dtype=np.dtype(self.typestr))
        if out.nbytes:
            rc = _hip_runtime().hipMemcpy(C.c_void_p(out.ctypes.data), C.c_void_p(self.ptr), C.c_size_t(out.nbytes), 2)   # hipMemcpyDeviceToHost
            if rc != 0:
                raise PowerFlowError(f"hipMemcpy of {self!r} failed: hipError {rc}")
        return out


_hip: Optional[C.CDLL] = None


def _hip_runtime() -> C.CDLL:
    """The HIP runtime libgridstep.so is linked against (already in the process once the library is loaded)."""
    global _hip
    if _hip is None:
        load()
        last = None
        for name in ("libamdhip64.so", "libamdhip64.so.7", "libamdhip64.so.6", "/opt/rocm/lib/libamdhip64.so"):
            try:
                _hip = C.CDLL(name)
                break
            except OSError as e:
                last = e
        if _hip is None:
            raise PowerFlowError(f"the HIP runtime could not be loaded: {last}")
        _hip.hipMemcpy.restype = C.c_int
        _hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    return _hip


def _stream_arg(stream):
    """A consumer's / producer's ``hipStream_t`` for the C ABI: ``None`` = no stream (the caller synchronises itself); an
    integer handle otherwise.  Handle 0 is the LEGACY DEFAULT stream -- what ``torch.cuda.current_stream().cuda_stream`` is
    unless the caller made a stream of its own -- and goes over as ``hipStreamLegacy`` (1), since NULL means "no stream" at
    the boundary.  (Round 3: 0 used to be taken for "no stream", which left a step free to read its actions before the
    default stream had written them.)"""
    if stream is None:
        return None
    return C.c_void_p(int(stream) if int(stream) != 0 else 1)


def _device_address(x, shape) -> int:
    """Device address of a float64 C-contiguous array of ``shape`` given as an int, a torch tensor or anything with
    ``__cuda_array_interface__``."""
    if isinstance(x, int):
        return x
    if hasattr(x, "data_ptr"):                      # torch
        if tuple(x.shape) != tuple(shape) or str(x.dtype) not in ("torch.float64",) or not x.is_contiguous():
            raise PowerFlowError(f"device actions must be a contiguous float64 tensor of shape {tuple(shape)}, got {tuple(x.shape)} {x.dtype}")
        return int(x.data_ptr())
    cai = getattr(x, "__cuda_array_interface__", None)
    if cai is None:
        raise PowerFlowError("device actions: an address, a torch tensor or an object with __cuda_array_interface__")
    if tuple(cai["shape"]) != tuple(shape) or cai["typestr"] not in ("<f8", "=f8") or cai.get("strides") not in (None,):
        raise PowerFlowError(f"device actions must be C-contiguous float64 of shape {tuple(shape)}")
    return int(cai["data"][0])


def _device_address_of(x, shape, dtype) -> int:
    """``_device_address`` for a C-contiguous array of ``dtype`` (float64 / float32): a torch tensor or anything with
    ``__cuda_array_interface__``."""
    dt = np.dtype(dtype)
    if hasattr(x, "data_ptr"):                      # torch
        if tuple(x.shape) != tuple(shape) or str(x.dtype) != f"torch.{dt.name}" or not x.is_contiguous() or not getattr(x, "is_cuda", True):
            raise PowerFlowError(f"expected a contiguous {dt.name} device tensor of shape {tuple(shape)}, got {tuple(x.shape)} {x.dtype}")
        return int(x.data_ptr())
    cai = getattr(x, "__cuda_array_interface__", None)
    if cai is None:
        raise PowerFlowError("expected a torch tensor or an object with __cuda_array_interface__")
    if tuple(cai["shape"]) != tuple(shape) or np.dtype(cai["typestr"]) != dt or cai.get("strides") not in (None,):
        raise PowerFlowError(f"expected a C-contiguous {dt.name} device array of shape {tuple(shape)}")
    return int(cai["data"][0])


def check_line_impedances(spec: FeederSpec, r, x, rows: int) -> Tuple[np.ndarray, np.ndarray]:
    """Per-instance line impedances ``r``, ``x`` of shape [rows, m] as C-contiguous float64, checked against the rules of
    gs_topology::line_r_inst (include/gridstep.h): finite, r >= 0, a line of zero nominal impedance keeps its nominal r and x in
    every instance, every other line keeps hypot(r, x) > 1e-12.  Raises ValueError."""
    r = np.ascontiguousarray(r, dtype=np.float64)
    x = np.ascontiguousarray(x, dtype=np.float64)
    shape = (int(rows), int(spec.m))
    if r.shape != shape or x.shape != shape:
        raise ValueError(f"line impedances: r and x must have shape {shape}, got {r.shape} and {x.shape}")
    if not (np.isfinite(r).all() and np.isfinite(x).all()):
        raise ValueError("line impedances: every value must be finite")
    if (r < 0).any():
        raise ValueError("line impedances: r must be >= 0")
    zero = ~(np.hypot(np.asarray(spec.r, dtype=np.float64), np.asarray(spec.x, dtype=np.float64)) > 1e-12)
    if zero.any() and not (np.array_equal(r[:, zero], np.broadcast_to(np.asarray(spec.r)[zero], (shape[0], int(zero.sum())))) and
                           np.array_equal(x[:, zero], np.broadcast_to(np.asarray(spec.x)[zero], (shape[0], int(zero.sum()))))):
        raise ValueError("line impedances: a line of zero nominal impedance keeps its nominal r and x in every instance")
    if not (np.hypot(r[:, ~zero], x[:, ~zero]) > 1e-12).all():
        raise ValueError("line impedances: a line of non-zero nominal impedance cannot have zero impedance")
    return r, x


def check_load_powers(spec: FeederSpec, load_powers, rows: int) -> np.ndarray:
    """Per-instance load powers of shape [rows, n_loads] (watts) as C-contiguous float64, checked against the rules of
    gs_topology::load_base_inst (include/gridstep.h): the feeder has loads, every value finite and >= 0.  Raises ValueError."""
    if int(spec.n_loads) == 0:
        raise ValueError("load powers: the feeder has no loads")
    pl = np.ascontiguousarray(load_powers, dtype=np.float64)
    shape = (int(rows), int(spec.n_loads))
    if pl.shape != shape:
        raise ValueError(f"load powers must have shape {shape}, got {pl.shape}")
    if not np.isfinite(pl).all():
        raise ValueError("load powers: every value must be finite")
    if (pl < 0).any():
        raise ValueError("load powers must be >= 0")
    return pl


def _topology_of(spec: FeederSpec, line_impedances=None, load_powers=None):
    """gs_topology of a FeederSpec and the arrays it points into (keep them alive while the struct is in use).
    ``line_impedances``: None or (r, x), C-contiguous float64 [batch, m] (gs_topology::line_r_inst / line_x_inst);
    ``load_powers``: None or C-contiguous float64 [batch, n_loads] (gs_topology::load_base_inst)."""
    keep = dict(frm=_i32(spec.frm), to=_i32(spec.to), r=_f64(spec.r), x=_f64(spec.x), rating=_f64(spec.rating),
                bus_type=np.ascontiguousarray(spec.bus_type, dtype=np.uint8), v_set=_f64(spec.v_set),
                load_bus=_i32(spec.load_bus), load_base=_f64(spec.load_base), load_pf=_f64(spec.load_pf),
                gen_bus=_i32(spec.gen_bus), gen_kind=_i32(spec.gen_kind), gen_cap=_f64(spec.gen_cap),
                gen_p0=_f64(spec.gen_p0), gen_p1=_f64(spec.gen_p1), gen_p2=_f64(spec.gen_p2),
                bat_bus=_i32(spec.bat_bus), bat_cap=_f64(spec.bat_cap), bat_rating=_f64(spec.bat_rating),
                bat_eff=_f64(spec.bat_eff))
    t = gs_topology()
    t.struct_size = C.sizeof(gs_topology)
    t.n, t.m = spec.n, spec.m
    t.from_bus, t.to_bus = _ptr(keep["frm"], _ip), _ptr(keep["to"], _ip)
    t.r, t.x, t.rating = _ptr(keep["r"], _dp), _ptr(keep["x"], _dp), _ptr(keep["rating"], _dp)
    t.bus_type, t.v_set = _ptr(keep["bus_type"], _up), _ptr(keep["v_set"], _dp)
    t.n_loads = spec.n_loads
    t.load_bus, t.load_base, t.load_pf = _ptr(keep["load_bus"], _ip), _ptr(keep["load_base"], _dp), _ptr(keep["load_pf"], _dp)
    t.n_gens = spec.n_gens
    t.gen_bus, t.gen_kind, t.gen_cap = _ptr(keep["gen_bus"], _ip), _ptr(keep["gen_kind"], _ip), _ptr(keep["gen_cap"], _dp)
    t.gen_p0, t.gen_p1, t.gen_p2 = _ptr(keep["gen_p0"], _dp), _ptr(keep["gen_p1"], _dp), _ptr(keep["gen_p2"], _dp)
    t.n_bats = spec.n_bats
    t.bat_bus, t.bat_cap = _ptr(keep["bat_bus"], _ip), _ptr(keep["bat_cap"], _dp)
    t.bat_rating, t.bat_eff = _ptr(keep["bat_rating"], _dp), _ptr(keep["bat_eff"], _dp)
    if line_impedances is not None:
        keep["r_inst"], keep["x_inst"] = _f64(line_impedances[0]), _f64(line_impedances[1])
        t.line_r_inst, t.line_x_inst = _ptr(keep["r_inst"], _dp), _ptr(keep["x_inst"], _dp)
    if load_powers is not None:
        keep["load_inst"] = _f64(load_powers)
        t.load_base_inst = _ptr(keep["load_inst"], _dp)
    return t, keep


def policy_struct(weights, biases, activation="relu", head="gaussian_tanh", stochastic=False, n_layers=None):
    """gs_policy_mlp of per-layer ``weights`` ([out, in], torch's Linear.weight layout) and ``biases`` and the arrays it points
    into (keep them alive while the struct is in use).  ``n_layers`` overrides the count (the refusal tests pass 0 and 5); ``head`` may be a
    raw GS_HEAD_* value (GS_HEAD_LINEAR: a value network)."""
    keep = {"w": [_f64(w) for w in weights], "b": [_f64(b) for b in biases]}
    p = gs_policy_mlp()
    p.struct_size = C.sizeof(gs_policy_mlp)
    p.n_layers = len(keep["w"]) if n_layers is None else int(n_layers)
    p.activation, p.head, p.stochastic = ACTIVATION[activation], HEAD[head] if isinstance(head, str) else int(head), int(bool(stochastic))
    for l, (w, b) in enumerate(zip(keep["w"][:GS_POLICY_MAX_LAYERS], keep["b"])):
        if w.ndim != 2 or b.shape != (w.shape[0],):
            raise ValueError(f"layer {l}: weights must be [out, in] and biases [out], got {w.shape} and {b.shape}")
        if l and w.shape[1] != keep["w"][l - 1].shape[0]:
            raise ValueError(f"layer {l} takes {w.shape[1]} inputs, layer {l - 1} gives {keep['w'][l - 1].shape[0]}")
        p.dims[l], p.dims[l + 1] = w.shape[1], w.shape[0]
        p.weights[l], p.biases[l] = _ptr(w, _dp), _ptr(b, _dp)
    return p, keep


def policy_check(p: gs_policy_mlp, obs_dim: int, action_dim: int) -> Tuple[int, str]:
    """gs_policy_mlp_check: (return code, message) -- the rules of gs_policy_mlp on the host alone (no GPU)."""
    return _host_check("gs_policy_mlp_check", C.byref(p), int(obs_dim), int(action_dim))


def policy_opts(compute="float64", obs_shift=None, obs_scale=None, struct_size=None):
    """gs_policy_mlp_opts and the arrays it points into.  ``compute``: "float64" | "float32" or a raw GS_COMPUTE_* value;
    ``struct_size`` overrides the size (the refusal tests pass a wrong one)."""
    keep = {"shift": None if obs_shift is None else _f64(obs_shift).reshape(-1),
            "scale": None if obs_scale is None else _f64(obs_scale).reshape(-1)}
    o = gs_policy_mlp_opts()
    o.struct_size = C.sizeof(gs_policy_mlp_opts) if struct_size is None else int(struct_size)
    o.compute = COMPUTE[compute] if isinstance(compute, str) else int(compute)
    if keep["shift"] is not None:
        o.obs_shift = _ptr(keep["shift"], _dp)
    if keep["scale"] is not None:
        o.obs_scale = _ptr(keep["scale"], _dp)
    return o, keep


def policy_check_opts(p: gs_policy_mlp, o: Optional[gs_policy_mlp_opts], obs_dim: int, action_dim: int) -> Tuple[int, str]:
    """gs_policy_mlp_check_opts: (return code, message) -- the rules of gs_policy_mlp and its options on the host alone."""
    return _host_check("gs_policy_mlp_check_opts", C.byref(p), None if o is None else C.byref(o), int(obs_dim), int(action_dim))


def q_check(p: gs_policy_mlp, o: Optional[gs_policy_mlp_opts], obs_dim: int, action_dim: int) -> Tuple[int, str]:
    """(return code, message) of gs_q_mlp_check: the rules of ``gs_q_mlp_set`` on the host alone."""
    return _host_check("gs_q_mlp_check", C.byref(p), None if o is None else C.byref(o), int(obs_dim), int(action_dim))


def value_check(p: gs_policy_mlp, o: Optional[gs_policy_mlp_opts], obs_dim: int) -> Tuple[int, str]:
    """gs_value_mlp_check: (return code, message) -- the rules of a value network on the host alone (no GPU)."""
    return _host_check("gs_value_mlp_check", C.byref(p), None if o is None else C.byref(o), int(obs_dim))


MESH_ITEM_DTYPE = np.dtype([("vk_off", "<i4"), ("vj_off", "<i4"), ("xk_off", "<i4"), ("xj_off", "<i4"), ("flags", "<i4"), ("cq_off", "<i4"),
                            ("adj_ptr", "<i4"), ("bus", "<i4"), ("ykj_g", "<f8"), ("ykj_b", "<f8"), ("ykk_g", "<f8"), ("ykk_b", "<f8"),
                            ("mout", "<i4", (8,)), ("cq_in", "<i4", (4,)), ("rw_in", "<i4", (4,)), ("cl_in", "<i4", (4,)),
                            ("nbr", "<i4"), ("pos", "<i4"), ("pad", "<i4", (10,))])      # GsMeshItem, csrc/gs_internal.h


def flat_newton_map(spec, zero_z="open") -> np.ndarray:
    """gs_flat_newton_map_dump: W [2 (n - 1), n] with x = W [P_spec (non-slack buses, bus order); 1] -- the first Newton step from the flat
    start as the meshed step kernel takes it (host arithmetic, no GPU)."""
    lib = load()
    t, keep = _topology_of(spec)
    out = np.zeros((2 * (spec.n - 1), spec.n))
    rc = lib.gs_flat_newton_map_dump(C.byref(t), ZERO_Z[zero_z], _ptr(out, _dp))
    if rc != GS_OK:
        raise PowerFlowError(f"gs_flat_newton_map_dump failed ({rc}): {lib.gs_last_error(None).decode()}")
    return out


def plan_describe(spec: FeederSpec, cfg: gs_config, batch: int, cus: int = 256, line_impedances=None, load_powers=None) -> dict:
    """gs_plan_describe: what Handle(spec, cfg, batch).describe() returns on a device with ``cus`` compute units, planned on the host
    (no device needed).  ``line_impedances``: None or per-instance (r, x), [batch, m] each; ``load_powers``: None or per-instance
    load powers, [batch, n_loads]."""
    lib = load()
    t, keep = _topology_of(spec, line_impedances, load_powers)
    buf = C.create_string_buffer(4096)
    rc = lib.gs_plan_describe(C.byref(t), C.byref(cfg), int(batch), int(cus), buf, 4096)
    if rc != GS_OK:
        raise PowerFlowError(f"gs_plan_describe failed ({rc}): {lib.gs_last_error(None).decode()}")
    return json.loads(buf.value.decode())


def mesh_schedule(spec: FeederSpec, nw: int = 4, ni: int = 10, acc_cap: int = 4, region_base: int = 0, slot_bytes: int = 144,
                  zero_z: str = "open", unit_budget: int = 0) -> dict:
    """gs_mesh_schedule_dump: the host-side schedule of the meshed Newton-Raphson step kernel for ``spec`` (no device needed).
    Returns the header fields, ``why`` (when not eligible) and the tables as NumPy arrays (items: MESH_ITEM_DTYPE)."""
    lib = load()
    t, keep = _topology_of(spec)
    hd = np.zeros(16, dtype=np.int32)
    why = C.create_string_buffer(256)
    args = (C.byref(t), ZERO_Z[zero_z], int(nw), int(ni), int(acc_cap), int(unit_budget), int(region_base), int(slot_bytes))
    rc = lib.gs_mesh_schedule_dump(*args, _ptr(hd, _ip), why, 256, None, None, None, None)
    if rc != GS_OK:
        raise PowerFlowError(f"gs_mesh_schedule_dump failed ({rc}): {lib.gs_last_error(None).decode()}")
    names = ("ok", "n_levels", "n_rows", "max_rows_per_wave", "n_pivots", "msg_units", "n_messages", "n_accumulators", "max_degree",
             "unit_bytes", "zero_off", "dummy_off", "body_off", "region_bytes", "item_bytes", "n_adj")
    out = {k: int(v) for k, v in zip(names, hd)}
    out["why"] = why.value.decode(); out["nw"], out["ni"] = int(nw), int(ni)
    if not out["ok"]:
        return out
    if out["item_bytes"] != MESH_ITEM_DTYPE.itemsize:
        raise PowerFlowError(f"GsMeshItem is {out['item_bytes']} bytes in the library, {MESH_ITEM_DTYPE.itemsize} here")
    items = np.zeros(nw * ni * 8, dtype=MESH_ITEM_DTYPE)
    rowinfo = np.zeros((nw * ni, 4), dtype=np.int32)
    adj_off = np.zeros(max(out["n_adj"], 1), dtype=np.int32)
    adj_y = np.zeros((max(out["n_adj"], 1), 2))
    rc = lib.gs_mesh_schedule_dump(*args, _ptr(hd, _ip), why, 256, items.ctypes.data_as(C.c_void_p), _ptr(rowinfo, _ip),
                                   _ptr(adj_off, _ip), _ptr(adj_y, _dp))
    if rc != GS_OK:
        raise PowerFlowError(f"gs_mesh_schedule_dump failed ({rc}): {lib.gs_last_error(None).decode()}")
    out.update(items=items.reshape(nw, ni, 8), rowinfo=rowinfo.reshape(nw, ni, 4), adj_off=adj_off, adj_y=adj_y)
    # the packed form the kernel reads
    cnt = np.zeros(4, dtype=np.int32)
    rc = lib.gs_mesh_schedule_dump_packed(*args, _ptr(cnt, _ip), None, None, None, None)
    if rc != GS_OK:
        raise PowerFlowError(f"gs_mesh_schedule_dump_packed failed ({rc}): {lib.gs_last_error(None).decode()}")
    packed = np.zeros((nw * ni * 8, int(cnt[3])), dtype=np.int32)
    rowinfo_p = np.zeros((nw * ni, 4), dtype=np.int32)
    ytab = np.zeros((int(cnt[1]) // 2, 2))
    adj_ent = np.zeros(int(cnt[2]), dtype=np.int32)
    rc = lib.gs_mesh_schedule_dump_packed(*args, _ptr(cnt, _ip), _ptr(packed, _ip), _ptr(rowinfo_p, _ip), _ptr(ytab, _dp), _ptr(adj_ent, _ip))
    if rc != GS_OK:
        raise PowerFlowError(f"gs_mesh_schedule_dump_packed failed ({rc}): {lib.gs_last_error(None).decode()}")
    out.update(n_pairs=int(cnt[0]), packed=packed.reshape(nw, ni, 8, -1), rowinfo_packed=rowinfo_p.reshape(nw, ni, 4), ytab=ytab, adj_ent=adj_ent)
    return out


class Handle:
    """Owns one gs_handle (one GPU, one stream).  All array arguments are NumPy, batch-major."""

    def __init__(self, spec: FeederSpec, cfg: gs_config, batch: int, device: int = 0, first_instance: int = 0, line_impedances=None,
                 load_powers=None):
        self._lib = load()
        self._h = _H()
        self.spec = spec
        self.B = int(batch)
        self.obs_dtype = np.dtype(np.float64)      # np.float32: step() / download_step() hand out the block rounded on the device (gs_step_f32)
        t, keep = _topology_of(spec, line_impedances, load_powers)
        self._pz = line_impedances is not None
        self._pl = load_powers is not None
        rc = self._lib.gs_create(C.byref(t), C.byref(cfg), self.B, int(device), int(first_instance), C.byref(self._h))
        if rc != GS_OK:
            self._h = _H()
            raise PowerFlowError(f"gs_create failed ({rc}): {self._lib.gs_last_error(None).decode()}")
        dims = [C.c_int32() for _ in range(6)]
        self._check(self._lib.gs_dims(self._h, *[C.byref(d) for d in dims]))
        self.n, self.m, self.obs_dim, self.action_dim, self.state_dim, _ = [d.value for d in dims]

    # -- plumbing -------------------------------------------------------------------------
    def _check(self, rc: int) -> None:
        if rc != GS_OK:
            raise PowerFlowError(f"libgridstep error {rc}: {self._lib.gs_last_error(self._h).decode()}")

    def close(self) -> None:
        if getattr(self, "_h", None) and self._h.value:
            for child in list(getattr(self, "_children", [])):     # objects bound to this handle (safety.PostStepChecks) go first
                child.close()
            self._lib.gs_destroy(self._h)
            self._h = _H()
            self._free_pinned()

    def last_error(self) -> str:
        return self._lib.gs_last_error(self._h).decode()

    def _instance_mask(self, mask) -> Optional[np.ndarray]:
        """``mask`` (None: every instance) as the uint8 [B] array the per-instance setters pass on."""
        if mask is None:
            return None
        mk = np.ascontiguousarray(mask, dtype=np.uint8)
        if mk.shape != (self.B,):
            raise PowerFlowError(f"mask must have shape ({self.B},)")
        return mk

    # -- per-instance line impedances (gs_set_line_impedances / gs_get_line_impedances) --------------------------------------
    def set_line_impedances(self, r: np.ndarray, x: np.ndarray, mask: Optional[np.ndarray] = None) -> None:
        r, x = _f64(r), _f64(x)
        if r.shape != (self.B, self.m) or x.shape != (self.B, self.m):
            raise PowerFlowError(f"line impedances must have shape {(self.B, self.m)}")
        mk = self._instance_mask(mask)
        self._check(self._lib.gs_set_line_impedances(self._h, _ptr(r, _dp), _ptr(x, _dp), None if mk is None else _ptr(mk, _up)))

    def get_line_impedances(self) -> Tuple[np.ndarray, np.ndarray]:
        r = np.empty((self.B, self.m)); x = np.empty((self.B, self.m))
        self._check(self._lib.gs_get_line_impedances(self._h, _ptr(r, _dp), _ptr(x, _dp)))
        return r, x

    # -- per-instance load powers (gs_set_load_powers / gs_get_load_powers) ---------------------------------------------------
    def set_load_powers(self, load_powers: np.ndarray, mask: Optional[np.ndarray] = None) -> None:
        pl = _f64(load_powers)
        if pl.shape != (self.B, int(self.spec.n_loads)):
            raise PowerFlowError(f"load powers must have shape {(self.B, int(self.spec.n_loads))}")
        mk = self._instance_mask(mask)
        self._check(self._lib.gs_set_load_powers(self._h, _ptr(pl, _dp), None if mk is None else _ptr(mk, _up)))

    def get_load_powers(self) -> np.ndarray:
        pl = np.empty((self.B, int(self.spec.n_loads)))
        self._check(self._lib.gs_get_load_powers(self._h, _ptr(pl, _dp)))
        return pl

    def _adopt(self, child) -> None:
        if not hasattr(self, "_children"):
            self._children = []
        self._children.append(child)

    def _release(self, child) -> None:
        if child in getattr(self, "_children", []):
            self._children.remove(child)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def describe(self) -> dict:
        buf = C.create_string_buffer(4096)
        self._check(self._lib.gs_describe(self._h, buf, 4096))
        return json.loads(buf.value.decode())

    def synchronize(self) -> None:
        self._check(self._lib.gs_synchronize(self._h))

    # -- solver ---------------------------------------------------------------------------
    def _solution_buffers(self):
        B, n, m = self.B, self.n, self.m
        out = dict(bus_voltages=np.empty((B, n)), bus_angles=np.empty((B, n)), line_flows=np.empty((B, m)),
                   line_loadings=np.empty((B, m)), losses=np.empty(B), max_mismatch=np.empty(B),
                   iterations=np.empty(B, dtype=np.int32), converged=np.empty(B, dtype=np.uint8),
                   status=np.empty(B, dtype=np.int32))
        v = gs_solution_view(_ptr(out["bus_voltages"], _dp), _ptr(out["bus_angles"], _dp), _ptr(out["line_flows"], _dp),
                             _ptr(out["line_loadings"], _dp), _ptr(out["losses"], _dp), _ptr(out["max_mismatch"], _dp),
                             _ptr(out["iterations"], _ip), _ptr(out["converged"], _up), _ptr(out["status"], _ip))
        return out, v

    def _pq(self, P, Q):
        P = _f64(P)
        if P.shape != (self.B, self.n):
            raise PowerFlowError(f"P_spec shape {P.shape} != ({self.B}, {self.n})")
        if Q is not None:
            Q = _f64(Q)
            if Q.shape != P.shape:
                raise PowerFlowError(f"Q_spec shape {Q.shape} != {P.shape}")
        return P, Q

    def solve(self, P, Q=None) -> dict:
        P, Q = self._pq(P, Q)
        out, v = self._solution_buffers()
        self._check(self._lib.gs_solve(self._h, _ptr(P, _dp), _ptr(Q, _dp), C.byref(v)))
        return out

    def fallback_linear(self, load_w=None, gen_w=None, total_load=None, total_gen=None, mask=None) -> np.ndarray:
        """gs_fallback_linear: replace the solution of the masked (default: non-converged) instances by the reference's
        linear approximation (robust_power_flow.py:336-398); returns the boolean [B] array of replaced instances.
        Without load_w / gen_w the per-bus totals come from the environment state on the device."""
        def arr(a, shape):
            if a is None:
                return None
            a = _f64(a)
            if a.shape != shape:
                raise PowerFlowError(f"expected shape {shape}, got {a.shape}")
            return a
        lw, gw = arr(load_w, (self.B, self.n)), arr(gen_w, (self.B, self.n))
        tl, tg = arr(total_load, (self.B,)), arr(total_gen, (self.B,))
        mk = None if mask is None else np.ascontiguousarray(np.asarray(mask).astype(np.uint8).reshape(self.B))
        applied = np.zeros(self.B, dtype=np.uint8)
        cnt = C.c_int32(0)
        self._check(self._lib.gs_fallback_linear(self._h, _ptr(lw, _dp), _ptr(gw, _dp), _ptr(tl, _dp), _ptr(tg, _dp), _ptr(mk, _up),
                                                 _ptr(applied, _up), C.byref(cnt)))
        return applied.astype(bool)

    def upload_injections(self, P, Q=None) -> None:
        P, Q = self._pq(P, Q)
        self._check(self._lib.gs_upload_injections(self._h, _ptr(P, _dp), _ptr(Q, _dp)))

    def solve_device(self) -> None:
        self._check(self._lib.gs_solve_device(self._h))

    def download_solution(self) -> dict:
        out, v = self._solution_buffers()
        self._check(self._lib.gs_download_solution(self._h, C.byref(v)))
        return out

    # -- env ------------------------------------------------------------------------------
    def reset(self, seeds=None, mask=None, want_obs: bool = True):
        s = None if seeds is None else np.ascontiguousarray(seeds, dtype=np.uint64)
        k = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8)
        if s is not None and s.shape != (self.B,):
            raise PowerFlowError(f"seeds shape {s.shape} != ({self.B},)")
        if k is not None and k.shape != (self.B,):
            raise PowerFlowError(f"mask shape {k.shape} != ({self.B},)")
        obs = np.empty((self.B, self.obs_dim)) if want_obs else None
        self._check(self._lib.gs_reset(self._h, _ptr(s, C.POINTER(C.c_uint64)), _ptr(k, _up), _ptr(obs, _dp)))
        return obs

    # -- page-locked output buffers (opt-in) ----------------------------------------------------
    def use_pinned_outputs(self, sets: int = 2) -> None:
        """From now on step() / download_step() return arrays that live in ``sets`` rotating sets of page-locked host
        buffers (gs_host_alloc): the device-to-host copy runs at the link's rate and no 45 MB array is page-faulted in
        per step.  The price is the reference's "fresh arrays every step": what step() returned is overwritten ``sets``
        steps later -- copy what has to live longer (a replay buffer does that anyway)."""
        if getattr(self, "_pinned", None):
            return
        self._pinned, self._pinned_ptrs, self._pinned_turn = [], [], 0
        for _ in range(max(2, int(sets))):
            self._pinned.append(self._alloc_step_set(self._pinned_array))

    def _pinned_array(self, shape, dtype=np.float64):
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        p = C.c_void_p()
        rc = self._lib.gs_host_alloc(C.byref(p), max(n, 8))
        if rc != GS_OK:
            raise PowerFlowError(f"gs_host_alloc({n}) failed ({rc}): {self._lib.gs_last_error(None).decode()}")
        self._pinned_ptrs.append(p)
        return np.frombuffer((C.c_char * max(n, 8)).from_address(p.value), dtype=dtype, count=int(np.prod(shape))).reshape(shape)

    def _alloc_step_set(self, new, want_obs=True):
        B = self.B
        return dict(obs=new((B, self.obs_dim), self.obs_dtype) if want_obs else None, reward=new((B,)),
                    terminated=new((B,), np.uint8), truncated=new((B,), np.uint8),
                    power_flow_converged=new((B,), np.uint8), max_voltage=new((B,)), min_voltage=new((B,)),
                    total_losses=new((B,)), violations=new((B, 4), np.uint8),
                    constraint_violations=new((B,), np.int32), current_step=new((B,), np.int32),
                    episode_reward=new((B,)), iterations=new((B,), np.int32), status=new((B,), np.int32))

    def _free_pinned(self) -> None:
        self._pinned = None
        rec = getattr(self, "_recycle", None)
        if rec and getattr(self, "_h", None) and self._h.value:
            for st in rec["sets"]:
                self._unbind_obs(st)
        self._recycle = None
        keep = set()
        if rec:       # a set the caller still holds arrays of is not freed: those arrays stay valid (the memory goes with the process)
            for st in rec["sets"]:
                if not self._set_is_free(st):
                    keep.update(st["ptrs"])
        for p in getattr(self, "_pinned_ptrs", []):
            if p.value not in keep:
                self._lib.gs_host_free(p)
        self._pinned_ptrs = []

    # -- recycled output buffers (what BatchedGridEnvironment uses by default) -------------------------
    def use_recycled_outputs(self, max_sets: int = 4) -> None:
        """step() / download_step() return arrays that are views of page-locked buffer sets owned by the handle, and a set is
        taken again only once NOTHING the caller got from it is alive any more (the reference counts of its root arrays: every
        view, slice or reshape of a returned array holds one).  So the contract stays the reference's -- what step() returned is
        never overwritten behind the caller's back -- while the usual loop (consume the observation, drop it, step again) neither
        page-faults a fresh 45 MB array per step nor copies through pageable memory: 1.9 M -> ~7 M env-steps/s at B = 8192.
        A caller that keeps everything makes the pool grow to ``max_sets`` sets and then gets fresh pageable arrays as before."""
        if getattr(self, "_recycle", None) or getattr(self, "_pinned", None):
            return
        if not hasattr(self, "_pinned_ptrs"):
            self._pinned_ptrs = []
        self._recycle = {"sets": [], "max": max(1, int(max_sets))}

    @staticmethod
    def _anchor_counts(st):
        return [sys.getrefcount(a) for a in st["anchors"]]

    def _set_is_free(self, st) -> bool:
        # (NumPy collapses the base of a view of a view to the first array of the chain: the anchors are those first arrays --
        # what every view, slice and reshape of a returned array keeps alive; counted the same way as the baseline was)
        return all(c <= b for c, b in zip(self._anchor_counts(st), st["base"]))

    def _recycled_set(self, want_obs):
        rec = self._recycle
        for st in rec["sets"]:
            if st["want_obs"] == want_obs and self._set_is_free(st):
                return st
        if len(rec["sets"]) >= rec["max"]:
            return None
        # Only the observation block is page-locked and recycled: it is the 45 MB whose page faults and staged copy the sets exist to
        # avoid.  The dozen per-instance arrays (half a megabyte together) are fresh pageable arrays every step, so a caller that keeps an
        # `info` array does not keep a 45 MB block from being taken again -- the pool's bound is max_sets x B x obs_dim x 8 bytes of
        # page-locked memory, reached only by a caller that keeps max_sets observation arrays alive.
        before = len(self._pinned_ptrs)
        try:
            roots = {"obs": self._pinned_array((self.B, self.obs_dim), self.obs_dtype)}
        except PowerFlowError:                        # no page-locked memory to be had: an ordinary array, still reused
            for p in self._pinned_ptrs[before:]:
                self._lib.gs_host_free(p)
            del self._pinned_ptrs[before:]
            roots = {"obs": np.empty((self.B, self.obs_dim), dtype=self.obs_dtype)}
        st = {"roots": roots, "want_obs": want_obs, "ptrs": {p.value for p in self._pinned_ptrs[before:]}, "anchors": [], "base": []}
        def first_array(a):
            while isinstance(a.base, np.ndarray):
                a = a.base
            return a
        st["anchors"] = [first_array(r) for r in roots.values() if r is not None]
        st["base"] = self._anchor_counts(st)                                      # no views alive yet
        rec["sets"].append(st)
        return st

    # -- constant observation columns of a recycled / pinned set: written once (gs_host_obs_bind), not moved again ------------
    def _const_block(self):
        s = self.spec
        c0 = 2 * s.n + 2 * s.m + 1
        return c0, c0 + 2 * s.n_loads

    def _bind_obs(self, st) -> None:
        """Called once a set's observation array holds a whole observation: from now on downloads into it move the changing
        columns only.  A caller that edits returned arrays IN PLACE would spoil the constant columns for the set's next use: a
        sample of them is checked before every reuse (``_obs_intact``), and a spoilt set is bound again."""
        obs = st["roots"].get("obs") if st else None
        c0, c1 = self._const_block()
        if obs is None or c1 <= c0 or obs.dtype != np.float64:      # (a float32 block is converted and copied whole)
            return
        if self._lib.gs_host_obs_bind(self._h, _ptr(obs, _dp)) != GS_OK:
            return
        rng = np.random.default_rng(12345)
        k = min(128, obs.shape[0] * (c1 - c0))
        rows, cols = rng.integers(0, obs.shape[0], k), rng.integers(c0, c1, k)
        st["probe"] = (rows, cols, obs[rows, cols].copy())

    def _obs_intact(self, st) -> bool:
        pr = st.get("probe")
        if pr is None:
            return True
        rows, cols, vals = pr
        return bool(np.array_equal(st["roots"]["obs"][rows, cols], vals))

    def _unbind_obs(self, st) -> None:
        if st.pop("probe", None) is not None:
            self._lib.gs_host_obs_unbind(self._h, _ptr(st["roots"]["obs"], _dp))

    def _step_buffers(self, want_obs=True):
        st = self._recycled_set(want_obs) if (getattr(self, "_recycle", None) and want_obs) else None
        self._cur_set = st
        if st is not None and not self._obs_intact(st):
            self._unbind_obs(st)                   # (this download writes whole rows again; bound anew behind it)
        if getattr(self, "_pinned", None):
            out = dict(self._pinned[self._pinned_turn])
            self._pinned_turn = (self._pinned_turn + 1) % len(self._pinned)
            if not want_obs:
                out["obs"] = None
        elif st is not None:
            out = self._alloc_step_set(lambda shape, dtype=np.float64: np.empty(shape, dtype=dtype), False)
            out["obs"] = st["roots"]["obs"].view()
        else:
            out = self._alloc_step_set(lambda shape, dtype=np.float64: np.empty(shape, dtype=dtype), want_obs)
        info = gs_info_view(_ptr(out["power_flow_converged"], _up), _ptr(out["max_voltage"], _dp),
                            _ptr(out["min_voltage"], _dp), _ptr(out["total_losses"], _dp), _ptr(out["violations"], _up),
                            _ptr(out["constraint_violations"], _ip), _ptr(out["current_step"], _ip),
                            _ptr(out["episode_reward"], _dp), _ptr(out["iterations"], _ip), _ptr(out["status"], _ip))
        return out, info

    def step(self, actions) -> dict:
        a = _f64(actions)
        if a.shape != (self.B, self.action_dim):
            raise PowerFlowError(f"actions shape {a.shape} != ({self.B}, {self.action_dim})")
        out, info = self._step_buffers()
        if self.obs_dtype == np.float32:
            self._check(self._lib.gs_step_f32(self._h, _ptr(a, _dp), _ptr(out["obs"], C.POINTER(C.c_float)), _ptr(out["reward"], _dp),
                                              _ptr(out["terminated"], _up), _ptr(out["truncated"], _up), C.byref(info)))
            return out
        self._check(self._lib.gs_step(self._h, _ptr(a, _dp), _ptr(out["obs"], _dp), _ptr(out["reward"], _dp),
                                      _ptr(out["terminated"], _up), _ptr(out["truncated"], _up), C.byref(info)))
        self._after_download()
        return out

    def _after_download(self) -> None:
        st = getattr(self, "_cur_set", None)
        if st is not None and st["roots"].get("obs") is not None and "probe" not in st and st["ptrs"]:
            self._bind_obs(st)

    def upload_actions(self, actions) -> None:
        a = _f64(actions)
        if a.ndim != 3 or a.shape[1:] != (self.B, self.action_dim):
            raise PowerFlowError(f"actions shape {a.shape} != (K, {self.B}, {self.action_dim})")
        self._check(self._lib.gs_upload_actions(self._h, _ptr(a, _dp), a.shape[0]))

    def step_device(self, k: int) -> None:
        self._check(self._lib.gs_step_device(self._h, int(k)))

    # -- a consumer on the same GPU: device pointers in, device pointers out -------------------------
    def step_device_ptr(self, actions, stream=None) -> None:
        """gs_step_device_ptr: one step with ``actions`` [B, action_dim] float64 in DEVICE memory -- an integer address, or
        any object with ``__cuda_array_interface__`` / ``data_ptr()`` (a torch tensor on this GPU).  ``stream``: the
        producer's ``hipStream_t`` as an integer (torch: ``torch.cuda.current_stream().cuda_stream``); the step then waits
        on the device for what is queued there.  None: the caller has synchronised."""
        self._check(self._lib.gs_step_device_ptr(self._h, C.c_void_p(_device_address(actions, (self.B, self.action_dim))),
                                                 _stream_arg(stream)))

    def step_device_view(self, stream=None) -> dict:
        """gs_step_device_view: the last step's observation block, rewards and flags as ``DeviceArray`` objects (zero-copy:
        ``torch.as_tensor(x, device="cuda")`` / ``cupy.asarray(x)``).  ``stream``: the consumer's stream, made to wait on the
        device for the step; None: the call returns when the step has finished.  The observation block is one of the handle's
        two buffers (valid until the next-but-one step), the other arrays are refreshed by every call."""
        out = gs_step_device_out()
        self._check(self._lib.gs_step_device_view(self._h, C.byref(out), _stream_arg(stream)))
        B = int(out.B)
        return dict(obs=DeviceArray(out.observations, (B, int(out.obs_dim)), "<f8"), reward=DeviceArray(out.reward, (B,), "<f8"),
                    terminated=DeviceArray(out.terminated, (B,), "|u1"), truncated=DeviceArray(out.truncated, (B,), "|u1"))

    def download_step(self, want_obs: bool = True) -> dict:
        out, info = self._step_buffers(want_obs)
        if want_obs and self.obs_dtype == np.float32:
            self._check(self._lib.gs_download_step_f32(self._h, _ptr(out["obs"], C.POINTER(C.c_float)), _ptr(out["reward"], _dp),
                                                       _ptr(out["terminated"], _up), _ptr(out["truncated"], _up), C.byref(info)))
            return out
        self._check(self._lib.gs_download_step(self._h, _ptr(out["obs"], _dp), _ptr(out["reward"], _dp),
                                               _ptr(out["terminated"], _up), _ptr(out["truncated"], _up), C.byref(info)))
        if want_obs:
            self._after_download()
        return out

    # -- rollout collection ------------------------------------------------------------------
    def set_policy(self, p: Optional[gs_policy_mlp], opts: Optional[gs_policy_mlp_opts] = None) -> None:
        """gs_policy_mlp_set / gs_policy_mlp_set_opts (with ``opts``): install (a copy of) the policy on the device; None
        removes it."""
        if opts is None:
            self._check(self._lib.gs_policy_mlp_set(self._h, None if p is None else C.byref(p)))
        else:
            self._check(self._lib.gs_policy_mlp_set_opts(self._h, None if p is None else C.byref(p), C.byref(opts)))

    def policy_eval(self, seed: int = 0, t: int = 0) -> np.ndarray:
        """gs_policy_mlp_eval: the installed policy's actions [B, action_dim] on the observation the environment stands at."""
        a = np.empty((self.B, self.action_dim))
        self._check(self._lib.gs_policy_mlp_eval(self._h, C.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF), int(t), _ptr(a, _dp)))
        return a

    def rollout(self, T: int, policy: str = "random", seed: int = 0, actions=None) -> None:
        """gs_rollout: T env steps back to back on the device (asynchronous).  policy "random": uniform actions in
        (-1, 1) drawn on the device from ``seed``; "uploaded": ``actions`` [T, B, A]; "mlp": the policy of ``set_policy``
        acts on every observation (``seed``: its noise)."""
        a = None
        if policy == "uploaded":
            a = _f64(actions)
            if a.shape != (int(T), self.B, self.action_dim):
                raise PowerFlowError(f"actions shape {a.shape} != ({T}, {self.B}, {self.action_dim})")
        self._check(self._lib.gs_rollout(self._h, int(T), POLICY[policy], C.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF), _ptr(a, _dp)))
        self._rollout_T = int(T)

    def rollout_download(self, want=("observations", "actions", "rewards", "next_observations", "terminals")) -> dict:
        """Host copies of the last rollout, [T, B, ...] each (gs_rollout_download); ``terminals`` is the raw uint8 flag
        array (bit 0 terminated, bit 1 truncated)."""
        T, B = self._rollout_T, self.B
        out = {}
        if "observations" in want: out["observations"] = np.empty((T, B, self.obs_dim))
        if "actions" in want: out["actions"] = np.empty((T, B, self.action_dim))
        if "rewards" in want: out["rewards"] = np.empty((T, B))
        if "next_observations" in want: out["next_observations"] = np.empty((T, B, self.obs_dim))
        if "terminals" in want: out["terminals"] = np.empty((T, B), dtype=np.uint8)
        if "final_observation" in want: out["final_observation"] = np.empty((B, self.obs_dim))
        n = C.c_int32(0)
        v = gs_rollout_view(_ptr(out.get("observations"), _dp), _ptr(out.get("actions"), _dp), _ptr(out.get("rewards"), _dp),
                            _ptr(out.get("next_observations"), _dp), _ptr(out.get("terminals"), _up),
                            _ptr(out.get("final_observation"), _dp), C.pointer(n))
        self._check(self._lib.gs_rollout_download(self._h, C.byref(v)))
        out["n_terminal"] = int(n.value)
        return out

    def rollout_load(self, observations, actions, rewards, next_observations, terminals, final_observation=None, log_probs=None,
                     chunk_rows: int = 0) -> None:
        """gs_rollout_load: these host arrays become the handle's rollout, as if ``rollout`` had produced them (the inverse of
        ``rollout_download``).  ``observations`` / ``next_observations`` [T, B, obs_dim], ``actions`` [T, B, action_dim], ``rewards``
        [T, B], ``terminals`` [T, B] uint8 (bit 0 terminated, bit 1 truncated), optionally ``final_observation`` [B, obs_dim] (None:
        ``next_observations[T - 1]``) and ``log_probs`` [T, B] (None: the rollout recorded none).  The floating arrays are all float64
        or all float32 (widened once, exactly, on the device); C-contiguous arrays are not copied.  A live transition's next
        observation must equal, by bits, the observation that follows it: GS_E_INVALID names the first that does not, and the handle
        then holds no rollout.  The environment is not touched.  ``chunk_rows``: rows of ``next_observations`` per staging chunk (0: the
        library's choice).  Returns when the arrays are on the device."""
        src, keep = rollout_source(self.B, self.obs_dim, self.action_dim, observations, actions, rewards, next_observations, terminals,
                                   final_observation, log_probs, chunk_rows)
        self._check(self._lib.gs_rollout_load(self._h, C.byref(src)))
        del keep
        self._rollout_T = int(src.T)

    def rollout_continue(self, T: int, keep: int, policy: str = "random", seed: int = 0, actions=None, t0: Optional[int] = None) -> None:
        """gs_rollout_continue (asynchronous): the last ``keep`` steps of the handle's rollout move to the front on the device and ``T``
        new steps are collected behind them; the rollout then has ``keep + T`` steps.  ``policy`` / ``seed`` / ``actions`` ([T, B, A], the
        new steps only) as ``rollout``; ``t0``: the step index the first new step draws with (None: where the last collection's draws
        ended, ``rollout_window_info()["t0_next"]``)."""
        a = None
        if policy == "uploaded":
            a = _f64(actions)
            if a.shape != (int(T), self.B, self.action_dim):
                raise PowerFlowError(f"actions shape {a.shape} != ({T}, {self.B}, {self.action_dim})")
        if t0 is None:
            t0 = self.rollout_window_info()["t0_next"]
        cfg = gs_rollout_continue_config(C.sizeof(gs_rollout_continue_config), int(T), int(keep), POLICY[policy], int(seed) & 0xFFFFFFFFFFFFFFFF,
                                         int(t0) & 0xFFFFFFFF, 0, _ptr(a, _dp))
        self._check(self._lib.gs_rollout_continue(self._h, C.byref(cfg)))
        self._rollout_T = int(keep) + int(T)

    def rollout_window_info(self) -> dict:
        """gs_rollout_window_info (host state, no wait): ``T`` steps of the handle's rollout, ``kept`` of them from before the last
        ``rollout_continue``, ``t0_next`` the draw index the next continue goes on with, ``T_cap`` the steps the buffers hold."""
        o = gs_rollout_window_info_out()
        self._check(self._lib.gs_rollout_window_info(self._h, C.byref(o)))
        return dict(T=int(o.T), kept=int(o.kept), t0_next=int(o.t0_next), T_cap=int(o.T_cap))

    # -- on-policy rollouts: log-probabilities, the value network, advantages and returns (include/gridstep.h) -------------------
    def rollout_log_probs(self, on: bool = True) -> None:
        """gs_rollout_set_log_probs: whether rollouts under a stochastic policy record the log-probabilities of their actions."""
        self._check(self._lib.gs_rollout_set_log_probs(self._h, int(bool(on))))

    def set_value(self, p: Optional[gs_policy_mlp], opts: Optional[gs_policy_mlp_opts] = None) -> None:
        """gs_value_mlp_set: install (a copy of) the value network on the device; None removes it."""
        self._check(self._lib.gs_value_mlp_set(self._h, None if p is None else C.byref(p), None if opts is None else C.byref(opts)))

    def value_eval(self) -> np.ndarray:
        """gs_value_mlp_eval: the value network's estimates [B] on the observation the environment stands at."""
        v = np.empty(self.B)
        self._check(self._lib.gs_value_mlp_eval(self._h, _ptr(v, _dp)))
        return v

    def rollout_evaluate(self, gamma: float = 0.99, lam: float = 0.95, bootstrap_mask: int = 0, reward_shift: float = 0.0,
                         reward_scale: float = 1.0) -> None:
        """gs_rollout_evaluate (asynchronous): values, terminal values, advantages and returns of the last rollout."""
        cfg = gs_gae_config(C.sizeof(gs_gae_config), int(bootstrap_mask), float(gamma), float(lam), float(reward_shift), float(reward_scale))
        self._check(self._lib.gs_rollout_evaluate(self._h, C.byref(cfg)))

    def rollout_onpolicy_view(self, stream=None) -> gs_rollout_onpolicy:
        """Device pointers of the last rollout's on-policy arrays (gs_rollout_onpolicy_view)."""
        v = gs_rollout_onpolicy()
        self._check(self._lib.gs_rollout_onpolicy_view(self._h, C.byref(v), _stream_arg(stream)))
        return v

    def rollout_onpolicy_arrays(self, stream=None) -> dict:
        """The same as zero-copy ``DeviceArray`` views: ``log_probs`` [T, B] (None if the rollout recorded none), ``values`` [T + 1, B],
        ``terminal_values`` [n_terminal], ``advantages`` and ``returns`` [T, B]; plus ``rows_per_tile``.  Valid until the next rollout."""
        v = self.rollout_onpolicy_view(stream)
        T, B, n = int(v.T), int(v.B), int(v.n_terminal)
        return dict(log_probs=DeviceArray(v.log_probs, (T, B), "<f8") if v.log_probs else None, values=DeviceArray(v.values, (T + 1, B), "<f8"),
                    terminal_values=DeviceArray(v.terminal_values, (n,), "<f8"), advantages=DeviceArray(v.advantages, (T, B), "<f8"),
                    returns=DeviceArray(v.returns, (T, B), "<f8"), rows_per_tile=int(v.rows_per_tile))

    def rollout_onpolicy_download(self, want=ONPOLICY_KEYS, n_terminal: Optional[int] = None) -> dict:
        """Host copies (gs_rollout_onpolicy_download) of the arrays named in ``want``; ``terminal_values`` needs ``n_terminal`` (what
        ``rollout_download`` reported) or asks for it."""
        T, B = getattr(self, "_rollout_T", 0), self.B
        for k in want:
            if k not in ONPOLICY_KEYS:
                raise PowerFlowError(f"rollout_onpolicy_download: unknown array {k!r}")
        if "terminal_values" in want and n_terminal is None:
            n_terminal = int(self.rollout_device_view().n_terminal)
        shapes = dict(_critic_shapes(T, B, n_terminal), log_probs=(T, B))
        out = {k: np.empty(shapes[k]) for k in want}
        v = gs_rollout_onpolicy_host(*[_ptr(out.get(k), _dp) for k in ONPOLICY_KEYS])
        self._check(self._lib.gs_rollout_onpolicy_download(self._h, C.byref(v)))
        return out

    # -- constraint costs of the last rollout: margins, counts, costs, cost critics and cost advantages (include/gridstep.h) ----
    def cost_config_default(self) -> gs_cost_config:
        """gs_cost_config_default: the handle's own voltage and frequency limits, 0.8 and the excess kind."""
        c = gs_cost_config()
        self._check(self._lib.gs_cost_config_default(self._h, C.byref(c)))
        return c

    def rollout_costs(self, cfg: Optional[gs_cost_config] = None) -> None:
        """gs_rollout_costs (asynchronous): margins, counts and costs of every transition of the last rollout; None: the defaults."""
        self._check(self._lib.gs_rollout_costs(self._h, None if cfg is None else C.byref(cfg)))

    def costs_eval(self, observations, cfg: Optional[gs_cost_config] = None, want=("margins", "counts", "costs")) -> dict:
        """gs_costs_eval: the same three results, [rows, 3] each, for ``observations`` [rows, obs_dim] on the host."""
        obs = _f64(observations)
        if obs.ndim != 2 or obs.shape[1] != self.obs_dim:
            raise PowerFlowError(f"observations shape {obs.shape} != (rows, {self.obs_dim})")
        rows = obs.shape[0]
        out = {k: np.empty((rows, 3), dtype=np.int32 if k == "counts" else np.float64) for k in want}
        self._check(self._lib.gs_costs_eval(self._h, None if cfg is None else C.byref(cfg), _ptr(obs, _dp) if rows else None, rows,
                                            _ptr(out.get("margins"), _dp), _ptr(out.get("counts"), _ip), _ptr(out.get("costs"), _dp)))
        return out

    def set_cost_value(self, channel: int, p: Optional[gs_policy_mlp], opts: Optional[gs_policy_mlp_opts] = None) -> None:
        """gs_cost_value_mlp_set: install (a copy of) a value network as the cost critic of ``channel``; None removes it."""
        self._check(self._lib.gs_cost_value_mlp_set(self._h, int(channel), None if p is None else C.byref(p), None if opts is None else C.byref(opts)))

    def rollout_evaluate_costs(self, gamma=0.99, lam=0.95, bootstrap_mask: int = 0, cost_shift=0.0, cost_scale=1.0, struct_size=None) -> None:
        """gs_rollout_evaluate_costs (asynchronous): values, terminal values, cost advantages and cost returns of every channel that
        has a critic.  ``gamma``, ``lam``, ``cost_shift``, ``cost_scale``: a scalar for all channels or three."""
        three = lambda x: _d3(*[float(v) for v in np.broadcast_to(np.asarray(x, dtype=np.float64), (3,))])
        cfg = gs_cost_gae_config(C.sizeof(gs_cost_gae_config) if struct_size is None else int(struct_size), int(bootstrap_mask), three(gamma),
                                 three(lam), three(cost_shift), three(cost_scale))
        self._check(self._lib.gs_rollout_evaluate_costs(self._h, C.byref(cfg)))

    def rollout_costs_view(self, stream=None) -> gs_rollout_costs_dev:
        """Device pointers of the last rollout's constraint arrays (gs_rollout_costs_view)."""
        v = gs_rollout_costs_dev()
        self._check(self._lib.gs_rollout_costs_view(self._h, C.byref(v), _stream_arg(stream)))
        return v

    def rollout_costs_arrays(self, stream=None) -> dict:
        """The same as zero-copy ``DeviceArray`` views: ``margins``, ``costs`` (float64) and ``counts`` (int32) [3, T, B], ``n_violating``
        [3] int64, and per channel c ``values[c]`` [T + 1, B], ``terminal_values[c]`` [n_terminal], ``advantages[c]``, ``returns[c]``
        [T, B] -- None where the channel had no critic at the last evaluation.  Valid until the next rollout."""
        v = self.rollout_costs_view(stream)
        T, B = int(v.T), int(v.B)
        n = int(self.rollout_device_view().n_terminal)
        shapes = _critic_shapes(T, B, n)
        out = dict(margins=DeviceArray(v.margins, (3, T, B), "<f8"), counts=DeviceArray(v.counts, (3, T, B), "<i4"),
                   costs=DeviceArray(v.costs, (3, T, B), "<f8"), n_violating=DeviceArray(v.n_violating, (3,), "<i8"))
        for k in COST_CRITIC_KEYS:
            out[k] = [DeviceArray(getattr(v, k)[c], shapes[k], "<f8") if getattr(v, k)[c] else None for c in range(3)]
        return out

    def rollout_costs_download(self, want=("margins", "counts", "costs", "n_violating"), channels=(), n_terminal: Optional[int] = None) -> dict:
        """Host copies (gs_rollout_costs_download) of the arrays named in ``want``; the per-channel arrays (``values``,
        ``terminal_values``, ``advantages``, ``returns``) come as lists of three with None outside ``channels``."""
        T, B = getattr(self, "_rollout_T", 0), self.B
        out = {}
        dtypes = dict(margins=np.float64, counts=np.int32, costs=np.float64)
        v = gs_rollout_costs_host()
        for k in want:
            if k in dtypes:
                out[k] = np.empty((3, T, B), dtype=dtypes[k])
                setattr(v, k, _ptr(out[k], _ip if k == "counts" else _dp))
            elif k == "n_violating":
                out[k] = np.empty(3, dtype=np.int64)
                v.n_violating = out[k].ctypes.data_as(C.POINTER(C.c_int64))
            elif k in COST_CRITIC_KEYS:
                if k == "terminal_values" and n_terminal is None:
                    n_terminal = int(self.rollout_device_view().n_terminal)
                out[k] = [np.empty(_critic_shapes(T, B, n_terminal)[k]) if c in channels else None for c in range(3)]
                for c in channels:
                    getattr(v, k)[c] = _ptr(out[k][c], _dp)
            else:
                raise PowerFlowError(f"rollout_costs_download: unknown array {k!r}")
        self._check(self._lib.gs_rollout_costs_download(self._h, C.byref(v)))
        return out

    # -- episode accounting: the episodes the last rollout finished and the carries of the open ones (include/gridstep.h) ---------
    def rollout_episodes(self, cfg: Optional[gs_episode_config] = None) -> None:
        """gs_rollout_episodes (asynchronous): the episode list, the statistics and the carries over the last rollout; None:
        continue, no costs, -1000."""
        self._check(self._lib.gs_rollout_episodes(self._h, None if cfg is None else C.byref(cfg)))

    def episodes_clear(self) -> None:
        """gs_episodes_clear: drop the episode track."""
        self._check(self._lib.gs_episodes_clear(self._h))

    def rollout_episodes_view(self, stream=None) -> gs_rollout_episodes_dev:
        """Device pointers of what gs_rollout_episodes left (gs_rollout_episodes_view)."""
        v = gs_rollout_episodes_dev()
        self._check(self._lib.gs_rollout_episodes_view(self._h, C.byref(v), _stream_arg(stream)))
        return v

    def rollout_episodes_arrays(self, stream=None) -> dict:
        """The same as zero-copy ``DeviceArray`` views: the list arrays of EPISODE_LIST_KEYS ([n_episodes]; ``episode_index``
        [n_episodes, 2]; ``episode_cost`` / ``episode_violating`` lists of three [n_episodes], one per channel), the carries of
        EPISODE_CARRY_KEYS ([B]; ``ep_cost`` / ``ep_violating`` [3, B]) -- the cost arrays None without costs -- and ``n_episodes``."""
        v = self.rollout_episodes_view(stream)
        n, B, stride = int(v.n_episodes), int(v.B), int(v.cost_stride)
        out = dict(n_episodes=n, with_costs=bool(v.with_costs))
        for k, dt in EPISODE_LIST_KEYS:
            ptr, ts, size = getattr(v, k), np.dtype(dt).str, np.dtype(dt).itemsize
            if not ptr:
                out[k] = None
            elif k in ("episode_cost", "episode_violating"):
                out[k] = [DeviceArray(ptr + c * stride * size, (n,), ts) for c in range(3)]
            else:
                out[k] = DeviceArray(ptr, (n, 2) if k == "episode_index" else (n,), ts)
        for k, dt in EPISODE_CARRY_KEYS:
            ptr = getattr(v, k)
            out[k] = DeviceArray(ptr, (3, B) if k in ("ep_cost", "ep_violating") else (B,), np.dtype(dt).str) if ptr else None
        return out

    def rollout_episodes_download(self, want=None, n_episodes: Optional[int] = None) -> dict:
        """Host copies (gs_rollout_episodes_download) of the arrays named in ``want`` (None: every list array and carry the last
        accounting made, and ``stats``): names of EPISODE_LIST_KEYS / EPISODE_CARRY_KEYS and "stats" (a ``gs_episode_stats``).
        Always carries ``n_episodes``."""
        if n_episodes is None:
            n_episodes = int(self.rollout_device_view().n_terminal)
        n, B = int(n_episodes), self.B
        cost_keys = ("episode_cost", "episode_violating", "episode_any_violating", "ep_cost", "ep_violating", "ep_any_violating")
        if want is None:
            with_costs = bool(self.rollout_episodes_view().with_costs)
            want = [k for k, _ in EPISODE_LIST_KEYS + EPISODE_CARRY_KEYS if with_costs or k not in cost_keys] + ["stats"]
        shapes = dict(episode_index=(n, 2), episode_cost=(3, n), episode_violating=(3, n), ep_cost=(3, B), ep_violating=(3, B))
        dtypes = dict(EPISODE_LIST_KEYS + EPISODE_CARRY_KEYS)
        v = gs_rollout_episodes_host()
        out = {}
        for k in want:
            if k == "stats":
                out[k] = gs_episode_stats()
                v.stats = C.addressof(out[k])
            elif k in dtypes:
                out[k] = np.empty(shapes.get(k, (n,) if k.startswith("episode_") else (B,)), dtype=dtypes[k])
                setattr(v, k, out[k].ctypes.data)
            else:
                raise PowerFlowError(f"rollout_episodes_download: unknown array {k!r}")
        cnt = C.c_int32(0)
        v.n_episodes = C.addressof(cnt)
        self._check(self._lib.gs_rollout_episodes_download(self._h, C.byref(v)))
        if int(cnt.value) != n:
            raise PowerFlowError(f"rollout_episodes_download: the rollout finished {cnt.value} episodes, not {n}")
        out["n_episodes"] = n
        return out

    # -- on-policy minibatch epochs over the last rollout (gs_onpolicy_*) --------------------------------------------------------
    def onpolicy_prepare(self, adv_norm="rollout", dtype=np.float32, fields=None, lambdas=(0.0, 0.0, 0.0), adv_eps: float = 1e-8,
                         obs_shift=None, obs_scale=None, struct_size=None) -> None:
        """gs_onpolicy_prepare (asynchronous): the combined advantage of the last rollout and its statistics, and the observation
        normalisation ``(x - obs_shift) * obs_scale`` of the minibatches.  ``adv_norm``: a name of ADV_NORM or its number; ``dtype``:
        float64 / float32 (or the GS_COMPUTE_* number); ``fields``: ``onpolicy_fields``; ``lambdas``: one multiplier per channel."""
        if isinstance(dtype, (int, np.integer)):
            compute = int(dtype)
        else:
            dt = np.dtype(dtype)
            if dt not in (np.dtype(np.float64), np.dtype(np.float32)):
                raise PowerFlowError(f"onpolicy_prepare: dtype {dt} (float64 or float32)")
            compute = 1 if dt == np.dtype(np.float32) else 0
        shift = None if obs_shift is None else _f64(obs_shift).reshape(-1)
        scale = None if obs_scale is None else _f64(obs_scale).reshape(-1)
        for v in (shift, scale):
            if v is not None and v.shape != (self.obs_dim,):
                raise PowerFlowError(f"onpolicy_prepare: obs_shift / obs_scale shape {v.shape} != ({self.obs_dim},)")
        cfg = gs_onpolicy_batch_config(C.sizeof(gs_onpolicy_batch_config) if struct_size is None else int(struct_size),
                                       ADV_NORM[adv_norm] if isinstance(adv_norm, str) else int(adv_norm), compute, onpolicy_fields(fields),
                                       _d3(*[float(x) for x in lambdas]), float(adv_eps), _ptr(shift, _dp), _ptr(scale, _dp))
        self._check(self._lib.gs_onpolicy_prepare(self._h, C.byref(cfg)))
        self._opb = (compute, int(cfg.fields))

    def onpolicy_stats(self) -> dict:
        """gs_onpolicy_stats: ``n`` and the combined advantage's ``adv_mean`` and raw ``adv_std`` over the rollout (waits for the prepare)."""
        o = gs_onpolicy_stats_out()
        self._check(self._lib.gs_onpolicy_stats(self._h, C.byref(o)))
        return dict(n=int(o.n), adv_mean=float(o.adv_mean), adv_std=float(o.adv_std))

    def onpolicy_batch(self, seed: int, epoch: int, first: int, n: int, out=None, stream=None) -> dict:
        """gs_onpolicy_batch: positions ``first .. first + n - 1`` of the epoch's permutation as zero-copy ``DeviceArray`` views keyed
        by the prepared fields (``cost_advantages`` / ``cost_returns``: lists of three, None for a channel that is not gathered), plus
        ``adv_stats`` [2] float64 with the advantages.  ``out``: the caller's device arrays per key (lists of three for the cost
        fields), the handle's own buffers -- valid until the next call -- for the rest; ``stream``: the consumer's stream."""
        compute, fields = getattr(self, "_opb", (1, 0))
        dt = np.dtype(np.float32 if compute == 1 else np.float64)
        n = int(n)
        shapes = dict(observations=(n, self.obs_dim), actions=(n, self.action_dim))
        types = dict(indices=np.dtype(np.int32), adv_stats=np.dtype(np.float64))
        shape = lambda k: (2,) if k == "adv_stats" else shapes.get(k, (n,))
        b = gs_onpolicy_batch_out()
        for k, x in (out or {}).items():
            if k in ("cost_advantages", "cost_returns"):
                for c in range(3):
                    if x[c] is not None:
                        getattr(b, k)[c] = _device_address_of(x[c], (n,), dt)
            elif k in dict(ONPOLICY_BATCH_FIELDS) or k == "adv_stats":
                setattr(b, k, _device_address_of(x, shape(k), types.get(k, dt)))
            else:
                raise PowerFlowError(f"onpolicy_batch: unknown output {k!r}")
        self._check(self._lib.gs_onpolicy_batch(self._h, C.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF), C.c_uint32(int(epoch) & 0xFFFFFFFF),
                                                int(first), n, C.byref(b), _stream_arg(stream)))
        res = {}
        for k, bit in ONPOLICY_BATCH_FIELDS:
            if not fields & bit:
                continue
            if k in ("cost_advantages", "cost_returns"):
                res[k] = [DeviceArray(getattr(b, k)[c], (n,), dt.str) if getattr(b, k)[c] else None for c in range(3)]
            else:
                res[k] = DeviceArray(getattr(b, k), shape(k), types.get(k, dt).str)
        if fields & 8:
            res["adv_stats"] = DeviceArray(b.adv_stats, (2,), "<f8")
        return res

    # -- the learner (gs_learner_*) ----------------------------------------------------------------------------------------------
    def learner_create(self, net, cfg: gs_learner_config) -> None:
        """gs_learner_create: the installed network ``net`` (``learner_net``) becomes trainable; Adam starts from zero."""
        self._check(self._lib.gs_learner_create(self._h, _net_number(net), C.byref(cfg)))

    def learner_step(self, net, batch: dict, n: Optional[int] = None, stream=None) -> None:
        """gs_learner_step (asynchronous): one update of ``net`` on ``batch``, a dict of ``onpolicy_batch``'s (device arrays or
        addresses per key; the cost fields lists of three).  ``n``: the samples, by default the length of ``observations``."""
        b = gs_onpolicy_batch_out()
        addr = lambda x: None if x is None else int(x) if isinstance(x, (int, np.integer)) else int(x.__cuda_array_interface__["data"][0]) if hasattr(x, "__cuda_array_interface__") else int(x.data_ptr())
        for k, x in batch.items():
            if k in ("cost_advantages", "cost_returns"):
                for c in range(3):
                    getattr(b, k)[c] = addr(x[c])
            elif k in dict(ONPOLICY_BATCH_FIELDS) or k == "adv_stats":
                setattr(b, k, addr(x))
        if n is None:
            obs = batch.get("observations")
            n = int(obs.shape[0]) if hasattr(obs, "shape") else 0
        self._check(self._lib.gs_learner_step(self._h, _net_number(net), C.byref(b), int(n), _stream_arg(stream)))

    def learner_step_pathwise(self, batch: dict, n: Optional[int] = None, cfg: Optional[gs_pathwise_config] = None, stream=None) -> None:
        """gs_learner_step_pathwise (asynchronous): one pathwise actor update of the policy on ``batch`` (as ``learner_step``'s) under
        ``cfg`` (``pathwise_config``)."""
        b = gs_onpolicy_batch_out()
        addr = lambda x: None if x is None else int(x) if isinstance(x, (int, np.integer)) else int(x.__cuda_array_interface__["data"][0]) if hasattr(x, "__cuda_array_interface__") else int(x.data_ptr())
        for k in ("observations", "indices"):
            if batch.get(k) is not None:
                setattr(b, k, addr(batch[k]))
        if n is None:
            obs = batch.get("observations")
            n = int(obs.shape[0]) if hasattr(obs, "shape") else 0
        cfg = pathwise_config() if cfg is None else cfg
        self._check(self._lib.gs_learner_step_pathwise(self._h, C.byref(b), int(n), C.byref(cfg), _stream_arg(stream)))

    def learner_pathwise_view(self, stream=None) -> dict:
        """gs_learner_pathwise_view: the last pathwise step's arrays as zero-copy ``DeviceArray`` views -- ``actions``, ``noise`` [n, A],
        ``log_probs``, ``q_min``, ``bc_terms``, ``loss_terms`` [n] (float64), ``which`` [n] (int32), and per twin ``q`` [n] (float64)
        and ``dq_da`` [n, A] (float32), None for a twin that was not installed; plus ``installed`` (the twins' numbers)."""
        o = gs_pathwise_view_out()
        self._check(self._lib.gs_learner_pathwise_view(self._h, C.byref(o), _stream_arg(stream)))
        n, A = int(o.n), int(o.action_dim)
        arr = lambda p, shape, ts: DeviceArray(p, shape, ts) if p else None
        # (pre_head: the policy's float32 pre-head rows, in the learners' shared scratch: flat from the first row's start, row i at
        # i * pre_head_stride, its first 2 A values mean | log_std; valid until the next step of any learner)
        flat = (n - 1) * int(o.pre_head_stride) + 2 * A
        return dict(pre_head=arr(o.pre_head, (flat,), "<f4"), pre_head_stride=int(o.pre_head_stride), actions=arr(o.actions, (n, A), "<f8"), noise=arr(o.noise, (n, A), "<f8"), log_probs=arr(o.log_probs, (n,), "<f8"),
                    q=[arr(o.q[w], (n,), "<f8") for w in range(2)], q_min=arr(o.q_min, (n,), "<f8"), bc_terms=arr(o.bc_terms, (n,), "<f8"),
                    loss_terms=arr(o.loss_terms, (n,), "<f8"), which=arr(o.which, (n,), "<i4"),
                    dq_da=[arr(o.dq_da[w], (n, A), "<f4") for w in range(2)], installed=tuple(w for w in range(2) if o.installed >> w & 1))

    def learner_step_conservative(self, net, batch: dict, n: Optional[int] = None, cfg: Optional[gs_conservative_config] = None, stream=None) -> None:
        """gs_learner_step_conservative (asynchronous): one conservative critic update of twin ``net`` ("q1" / "q2") on ``batch`` (as
        ``learner_step``'s) under ``cfg`` (``conservative_config``)."""
        b = gs_onpolicy_batch_out()
        addr = lambda x: None if x is None else int(x) if isinstance(x, (int, np.integer)) else int(x.__cuda_array_interface__["data"][0]) if hasattr(x, "__cuda_array_interface__") else int(x.data_ptr())
        for k in ("observations", "indices"):
            if batch.get(k) is not None:
                setattr(b, k, addr(batch[k]))
        if n is None:
            obs = batch.get("observations")
            n = int(obs.shape[0]) if hasattr(obs, "shape") else 0
        cfg = conservative_config() if cfg is None else cfg
        self._check(self._lib.gs_learner_step_conservative(self._h, _net_number(net), C.byref(b), int(n), C.byref(cfg), _stream_arg(stream)))

    def learner_refresh(self, batch: dict, cfg: gs_refresh_config, n: Optional[int] = None, stream=None) -> None:
        """gs_learner_refresh (asynchronous): the groups of ``cfg`` (``refresh_config``) re-evaluated for the transitions
        ``batch["indices"]`` names (a device int32 array, as ``learner_step``'s) under the images as they are now, written into the
        arrays of ``rollout_evaluate_q_next`` / ``rollout_evaluate_q`` at those transitions."""
        b = gs_onpolicy_batch_out()
        addr = lambda x: None if x is None else int(x) if isinstance(x, (int, np.integer)) else int(x.__cuda_array_interface__["data"][0]) if hasattr(x, "__cuda_array_interface__") else int(x.data_ptr())
        idx = batch.get("indices")
        if idx is not None:
            b.indices = addr(idx)
        if n is None:
            n = int(idx.shape[0]) if hasattr(idx, "shape") else 0
        self._check(self._lib.gs_learner_refresh(self._h, C.byref(b), int(n), C.byref(cfg), _stream_arg(stream)))

    def learner_conservative_view(self, stream=None) -> dict:
        """gs_learner_conservative_view: the last conservative step's arrays as zero-copy ``DeviceArray`` views -- ``random_actions``,
        ``policy_actions``, ``policy_noise`` [n, A], ``policy_log_probs``, ``loss_terms`` [n], ``q``, ``weights`` [3 n], ``scalars``
        [4] (m, S, lse, qbar) (float64), ``targets`` [n] (float32), ``pre_head`` / ``pre_head_stride`` as ``learner_pathwise_view``'s;
        plus ``net`` (the twin's learner number), ``n`` and ``action_dim``."""
        o = gs_conservative_view_out()
        self._check(self._lib.gs_learner_conservative_view(self._h, C.byref(o), _stream_arg(stream)))
        n, A = int(o.n), int(o.action_dim)
        flat = (n - 1) * int(o.pre_head_stride) + 2 * A
        return dict(net=int(o.net), n=n, action_dim=A, pre_head=DeviceArray(o.pre_head, (flat,), "<f4"), pre_head_stride=int(o.pre_head_stride),
                    random_actions=DeviceArray(o.random_actions, (n, A), "<f8"), policy_actions=DeviceArray(o.policy_actions, (n, A), "<f8"),
                    policy_noise=DeviceArray(o.policy_noise, (n, A), "<f8"), policy_log_probs=DeviceArray(o.policy_log_probs, (n,), "<f8"),
                    targets=DeviceArray(o.targets, (n,), "<f4"), q=DeviceArray(o.q, (3 * n,), "<f8"), weights=DeviceArray(o.weights, (3 * n,), "<f8"),
                    loss_terms=DeviceArray(o.loss_terms, (n,), "<f8"), scalars=DeviceArray(o.scalars, (4,), "<f8"))

    def learner_stats(self, net) -> dict:
        """gs_learner_stats: the last step's ``LEARNER_STATS`` as floats (waits for the step); ``step`` an int."""
        o = gs_learner_stats_out()
        self._check(self._lib.gs_learner_stats(self._h, _net_number(net), C.byref(o)))
        out = {k: float(getattr(o, k)) for k in LEARNER_STATS}
        out["step"] = int(o.step)
        return out

    def learner_info(self, net) -> dict:
        """gs_learner_info: ``dims`` (the layers' widths), ``activation`` (its name), ``param_count``, ``step``, ``rows_per_segment``."""
        o = gs_learner_info_out()
        self._check(self._lib.gs_learner_info(self._h, _net_number(net), C.byref(o)))
        names = {v: k for k, v in ACTIVATION.items()}
        return dict(dims=[int(o.dims[l]) for l in range(o.n_layers + 1)], activation=names[int(o.activation)], param_count=int(o.param_count),
                    step=int(o.step), rows_per_segment=int(o.rows_per_segment))

    def learner_download(self, net, want=("params", "grads", "m", "v")) -> dict:
        """gs_learner_download: flat float32 host copies [param_count], in torch order, of the arrays named in ``want``."""
        P = self.learner_info(net)["param_count"]
        out = {k: np.empty(P, dtype=np.float32) for k in want}
        unknown = set(out) - {"params", "grads", "m", "v"}
        if unknown:
            raise PowerFlowError(f"learner_download: unknown array(s) {sorted(unknown)}")
        ptr = lambda k: out[k].ctypes.data if k in out else None
        self._check(self._lib.gs_learner_download(self._h, _net_number(net), ptr("params"), ptr("grads"), ptr("m"), ptr("v")))
        return out

    # -- parameter anchors (gs_learner_anchor_*, gs_learner_fisher_*) -----------------------------------------------------------------
    def learner_anchor_here(self, net, params=None) -> None:
        """gs_learner_anchor_here: the PROX centre of ``net`` becomes ``params`` (flat float32 [param_count] in torch order), or a
        device copy of the learner's current master parameters."""
        ptr = None
        if params is not None:
            params = np.ascontiguousarray(params, dtype=np.float32).reshape(-1)
            P = self.learner_info(net)["param_count"]
            if params.size != P:
                raise PowerFlowError(f"learner_anchor_here: {params.size} values for {P} parameters")
            ptr = params.ctypes.data
        self._check(self._lib.gs_learner_anchor_here(self._h, _net_number(net), ptr))

    def learner_anchor_set(self, net, cfg: gs_learner_anchor_config) -> None:
        """gs_learner_anchor_set: the coefficients of ``cfg`` (``anchor_config``) apply from the next step of ``net``."""
        self._check(self._lib.gs_learner_anchor_set(self._h, _net_number(net), C.byref(cfg)))

    def learner_anchor_get(self, net) -> dict:
        """gs_learner_anchor_get: ``prox_mu`` and ``ewc_lambda`` in force."""
        o = gs_learner_anchor_config()
        self._check(self._lib.gs_learner_anchor_get(self._h, _net_number(net), C.byref(o)))
        return dict(prox_mu=float(o.prox_mu), ewc_lambda=float(o.ewc_lambda))

    def learner_fisher_begin(self, net) -> None:
        """gs_learner_fisher_begin: a task opens for ``net``: the pending Fisher sum and its sample count are zeroed."""
        self._check(self._lib.gs_learner_fisher_begin(self._h, _net_number(net)))

    def learner_fisher_accumulate(self, net, batch: dict, n: Optional[int] = None, stream=None) -> None:
        """gs_learner_fisher_accumulate (asynchronous): the per-sample squared gradients of ``net``'s loss on ``batch`` (as
        ``learner_step``'s) join the open task's pending sum; no parameter, moment or statistic changes."""
        b = gs_onpolicy_batch_out()
        addr = lambda x: None if x is None else int(x) if isinstance(x, (int, np.integer)) else int(x.__cuda_array_interface__["data"][0]) if hasattr(x, "__cuda_array_interface__") else int(x.data_ptr())
        for k, x in batch.items():
            if k in ("cost_advantages", "cost_returns"):
                for c in range(3):
                    getattr(b, k)[c] = addr(x[c])
            elif k in dict(ONPOLICY_BATCH_FIELDS) or k == "adv_stats":
                setattr(b, k, addr(x))
        if n is None:
            obs = batch.get("observations")
            n = int(obs.shape[0]) if hasattr(obs, "shape") else 0
        self._check(self._lib.gs_learner_fisher_accumulate(self._h, _net_number(net), C.byref(b), int(n), _stream_arg(stream)))

    def learner_fisher_commit(self, net, cfg: gs_fisher_config) -> None:
        """gs_learner_fisher_commit (asynchronous): the open task ends at the current master parameters and is merged into the EWC
        slot under ``cfg`` (``fisher_config``)."""
        self._check(self._lib.gs_learner_fisher_commit(self._h, _net_number(net), C.byref(cfg)))

    def learner_anchor_clear(self, net, which="both") -> None:
        """gs_learner_anchor_clear: ``which`` a name of ``ANCHOR_SLOTS`` or the GS_ANCHOR_* bits."""
        if isinstance(which, str):
            if which not in ANCHOR_SLOTS:
                raise ValueError(f"learner anchor: unknown slot {which!r}; one of {sorted(ANCHOR_SLOTS)}")
            which = ANCHOR_SLOTS[which]
        self._check(self._lib.gs_learner_anchor_clear(self._h, _net_number(net), int(which)))

    def learner_anchor_stats(self, net) -> dict:
        """gs_learner_anchor_stats: ``penalty_prox``, ``penalty_ewc``, ``grad_norm_loss``, ``prox_mu``, ``ewc_lambda`` (floats) and
        ``tasks``, ``fisher_samples`` (ints) of the last step taken with a non-zero coefficient (waits for it)."""
        o = gs_learner_anchor_stats_out()
        self._check(self._lib.gs_learner_anchor_stats(self._h, _net_number(net), C.byref(o)))
        return dict(penalty_prox=float(o.penalty_prox), penalty_ewc=float(o.penalty_ewc), grad_norm_loss=float(o.grad_norm_loss),
                    prox_mu=float(o.prox_mu), ewc_lambda=float(o.ewc_lambda), tasks=int(o.tasks), fisher_samples=int(o.fisher_samples))

    def learner_anchor_download(self, net, want=ANCHOR_ARRAYS) -> dict:
        """gs_learner_anchor_download: flat host copies [param_count], in torch order, of the arrays named in ``want``
        (``ANCHOR_ARRAYS``: float32 but ``fisher_pending``, which is float64)."""
        P = self.learner_info(net)["param_count"]
        unknown = set(want) - set(ANCHOR_ARRAYS)
        if unknown:
            raise PowerFlowError(f"learner_anchor_download: unknown array(s) {sorted(unknown)}")
        out = {k: np.empty(P, dtype=np.float64 if k == "fisher_pending" else np.float32) for k in want}
        ptr = lambda k: out[k].ctypes.data if k in out else None
        self._check(self._lib.gs_learner_anchor_download(self._h, _net_number(net), *[ptr(k) for k in ANCHOR_ARRAYS]))
        return out

    def learner_view(self, net, stream=None) -> dict:
        """gs_learner_view: the last step's per-sample arrays as zero-copy ``DeviceArray`` views (None where ``net`` has none)."""
        o = gs_learner_view_out()
        self._check(self._lib.gs_learner_view(self._h, _net_number(net), C.byref(o), _stream_arg(stream)))
        n = int(o.n)
        arr = lambda p, ts: DeviceArray(p, (n,), ts) if p else None
        return dict(log_probs_new=arr(o.log_probs_new, "<f8"), ratio=arr(o.ratio, "<f8"), clipped=arr(o.clipped, "<i4"),
                    loss_terms=arr(o.loss_terms, "<f8"), entropy_terms=arr(o.entropy_terms, "<f8"))

    def learner_set_loss(self, net, loss: gs_learner_loss) -> None:
        """gs_learner_set_loss: ``loss`` (``learner_loss``) applies from the next step of ``net``; Adam's state stays."""
        self._check(self._lib.gs_learner_set_loss(self._h, _net_number(net), C.byref(loss)))

    def learner_get_loss(self, net) -> dict:
        """gs_learner_get_loss: ``kind`` (a name of ``LOSS_KINDS``), ``temperature``, ``weight_max`` and ``expectile`` in force."""
        o = gs_learner_loss()
        self._check(self._lib.gs_learner_get_loss(self._h, _net_number(net), C.byref(o)))
        names = {v: k for k, v in LOSS_KINDS.items()}
        return dict(kind=names[int(o.kind)], temperature=float(o.temperature), weight_max=float(o.weight_max), expectile=float(o.expectile))

    # -- state-action critics (gs_q_*, gs_rollout_*_q, gs_learner_*_signal) ---------------------------------------------------------
    def set_q(self, which, p: Optional[gs_policy_mlp], opts: Optional[gs_policy_mlp_opts] = None) -> None:
        """gs_q_mlp_set: install (a copy of) twin ``which`` (0 / 1 / "q1" / "q2") and its target image; None removes it."""
        self._check(self._lib.gs_q_mlp_set(self._h, q_which(which), None if p is None else C.byref(p), None if opts is None else C.byref(opts)))

    def rollout_evaluate_q(self, gamma: float = 0.99, bootstrap_mask: int = 0, reward_shift: float = 0.0, reward_scale: float = 1.0,
                           struct_size=None) -> None:
        """gs_rollout_evaluate_q (asynchronous): the twins' values under both images, their minimum, q_adv and td_target."""
        cfg = gs_q_eval_config(C.sizeof(gs_q_eval_config) if struct_size is None else int(struct_size), int(bootstrap_mask), float(gamma),
                               float(reward_shift), float(reward_scale))
        self._check(self._lib.gs_rollout_evaluate_q(self._h, C.byref(cfg)))

    def rollout_q_arrays(self, stream=None) -> dict:
        """gs_rollout_q_view as zero-copy ``DeviceArray`` views, [T, B] float64 each: ``q`` {"online" / "target": [twin 0, twin 1]}
        (None for a twin that is not installed), ``q_min`` {"online" / "target"}, ``q_adv``, ``td_target``; plus ``installed`` (a
        tuple of the installed twins' numbers) and ``rows_per_tile``.  Valid until the next rollout."""
        v = gs_rollout_q()
        self._check(self._lib.gs_rollout_q_view(self._h, C.byref(v), _stream_arg(stream)))
        T, B = int(v.T), int(v.B)
        arr = lambda p: DeviceArray(p, (T, B), "<f8") if p else None
        return dict(q={name: [arr(v.q[s][w]) for w in range(2)] for s, name in enumerate(Q_SOURCES)},
                    q_min={name: arr(v.q_min[s]) for s, name in enumerate(Q_SOURCES)}, q_adv=arr(v.q_adv), td_target=arr(v.td_target),
                    installed=tuple(w for w in range(2) if v.installed >> w & 1), rows_per_tile=int(v.rows_per_tile))

    def rollout_q_download(self, want=("q", "q_min", "q_adv", "td_target")) -> dict:
        """gs_rollout_q_download: host copies [T, B] of what ``want`` names -- ``q`` and ``q_min`` as dicts like ``rollout_q_arrays``'s
        (``q`` holds both twins' arrays; a twin that is not installed is left as NaN)."""
        T, B = getattr(self, "_rollout_T", 0), self.B
        unknown = set(want) - {"q", "q_min", "q_adv", "td_target"}
        if unknown:
            raise PowerFlowError(f"rollout_q_download: unknown array(s) {sorted(unknown)}")
        o = gs_rollout_q_host()
        out: dict = {}
        if "q" in want:
            out["q"] = {name: [np.full((T, B), np.nan) for _ in range(2)] for name in Q_SOURCES}
            for s, name in enumerate(Q_SOURCES):
                for w in range(2):
                    o.q[s][w] = _ptr(out["q"][name][w], _dp)
        if "q_min" in want:
            out["q_min"] = {name: np.empty((T, B)) for name in Q_SOURCES}
            for s, name in enumerate(Q_SOURCES):
                o.q_min[s] = _ptr(out["q_min"][name], _dp)
        for k in ("q_adv", "td_target"):
            if k in want:
                out[k] = np.empty((T, B))
                setattr(o, k, _ptr(out[k], _dp))
        self._check(self._lib.gs_rollout_q_download(self._h, C.byref(o)))
        return out

    def learner_set_signal(self, net, signal) -> None:
        """gs_learner_set_signal: "batch" or "q" (``SIGNALS``, or the number) from the next step of ``net``."""
        if isinstance(signal, str):
            if signal not in SIGNALS:
                raise ValueError(f"learner signal: unknown signal {signal!r}; one of {sorted(SIGNALS)}")
            signal = SIGNALS[signal]
        self._check(self._lib.gs_learner_set_signal(self._h, _net_number(net), int(signal)))

    def learner_get_signal(self, net) -> str:
        """gs_learner_get_signal: the name of the signal in force."""
        o = C.c_int32(0)
        self._check(self._lib.gs_learner_get_signal(self._h, _net_number(net), C.byref(o)))
        return {v: k for k, v in SIGNALS.items()}[int(o.value)]

    def q_target_update(self, tau: float = 0.005) -> None:
        """gs_q_target_update (asynchronous): every installed twin's target image moves by ``tau`` towards its online image."""
        self._check(self._lib.gs_q_target_update(self._h, float(tau)))

    def q_target_download(self, which, param_count: int) -> np.ndarray:
        """gs_q_target_download: the target's parameters, float32 [param_count], flat in torch order."""
        out = np.empty(int(param_count), dtype=np.float32)
        self._check(self._lib.gs_q_target_download(self._h, q_which(which), out.ctypes.data))
        return out

    # -- policy-action TD targets (gs_rollout_evaluate_q_next, gs_rollout_q_next_*, gs_q_*_target_source) ---------------------------
    def rollout_evaluate_q_next(self, cfg: Optional[gs_q_next_config] = None) -> None:
        """gs_rollout_evaluate_q_next (asynchronous): the installed policy's action and log-probability at every next state, the
        target twins' values of it, their minimum and the Bellman target ``r' + gamma (min Q_target - alpha log pi)``."""
        cfg = q_next_config() if cfg is None else cfg
        self._check(self._lib.gs_rollout_evaluate_q_next(self._h, C.byref(cfg)))

    def rollout_q_next_arrays(self, stream=None) -> dict:
        """gs_rollout_q_next_view as zero-copy ``DeviceArray`` views: ``next_pre_head`` [T, B, 2 A] float32, ``next_actions``
        / ``next_noise`` [T, B, A], ``next_log_probs`` / ``q_next_min`` / ``td_target`` [T, B], ``q_next`` [twin 0, twin 1] (None for a twin that is
        not installed); under a bootstrap mask the terminal list's ``term_*`` arrays over its first ``n_terminal`` entries (None
        otherwise); plus ``installed`` and ``rows_per_tile``.  Valid until the next rollout."""
        v = gs_rollout_q_next()
        self._check(self._lib.gs_rollout_q_next_view(self._h, C.byref(v), _stream_arg(stream)))
        T, B, A = int(v.T), int(v.B), int(v.action_dim)
        n = int(self.rollout_device_view().n_terminal) if v.term_log_probs else 0
        arr = lambda p, shape, dt="<f8": DeviceArray(p, shape, dt) if p else None
        return dict(next_pre_head=arr(v.next_pre_head, (T, B, 2 * A), "<f4"), next_actions=arr(v.next_actions, (T, B, A)), next_noise=arr(v.next_noise, (T, B, A)),
                    next_log_probs=arr(v.next_log_probs, (T, B)), q_next=[arr(v.q_next[w], (T, B)) for w in range(2)],
                    q_next_min=arr(v.q_next_min, (T, B)), td_target=arr(v.td_target, (T, B)),
                    term_pre_head=arr(v.term_pre_head, (n, 2 * A), "<f4"), term_actions=arr(v.term_actions, (n, A)), term_noise=arr(v.term_noise, (n, A)),
                    term_log_probs=arr(v.term_log_probs, (n,)), term_q=[arr(v.term_q[w], (n,)) for w in range(2)],
                    term_q_min=arr(v.term_q_min, (n,)), term_value=arr(v.term_value, (n,)),
                    installed=tuple(w for w in range(2) if v.installed >> w & 1), rows_per_tile=int(v.rows_per_tile), n_terminal=n)

    Q_NEXT_KEYS = ("next_pre_head", "next_actions", "next_noise", "next_log_probs", "q_next", "q_next_min", "td_target", "term_pre_head", "term_actions",
                   "term_noise", "term_log_probs", "term_q", "term_q_min", "term_value")

    def rollout_q_next_download(self, want=Q_NEXT_KEYS, n_terminal: Optional[int] = None) -> dict:
        """gs_rollout_q_next_download: host copies of what ``want`` names, shaped as ``rollout_q_next_arrays``'s (``q_next`` and
        ``term_q`` hold both twins' arrays; a twin that is not installed, and every terminal array when the last evaluation ran
        under mask 0, is left as NaN).  The terminal arrays need ``n_terminal`` (read from the device when not given)."""
        unknown = set(want) - set(self.Q_NEXT_KEYS)
        if unknown:
            raise PowerFlowError(f"rollout_q_next_download: unknown array(s) {sorted(unknown)}")
        T, B, A = getattr(self, "_rollout_T", 0), self.B, self.action_dim
        if n_terminal is None and any(k.startswith("term_") for k in want):
            n_terminal = int(self.rollout_device_view().n_terminal)
        n = int(n_terminal or 0)
        shapes = dict(next_pre_head=(T, B, 2 * A), next_actions=(T, B, A), next_noise=(T, B, A), next_log_probs=(T, B), q_next_min=(T, B), td_target=(T, B),
                      term_pre_head=(n, 2 * A), term_actions=(n, A), term_noise=(n, A), term_log_probs=(n,), term_q_min=(n,), term_value=(n,))
        o = gs_rollout_q_next_host()
        out: dict = {}
        for k in want:
            if k in ("q_next", "term_q"):
                out[k] = [np.full((T, B) if k == "q_next" else (n,), np.nan) for _ in range(2)]
                for w in range(2):
                    getattr(o, k)[w] = _ptr(out[k][w], _dp)
            else:
                f32 = k.endswith("pre_head")
                out[k] = np.full(shapes[k], np.nan, dtype=np.float32 if f32 else np.float64)
                setattr(o, k, _ptr(out[k], _fp if f32 else _dp))
        self._check(self._lib.gs_rollout_q_next_download(self._h, C.byref(o)))
        return out

    def q_set_target_source(self, source) -> None:
        """gs_q_set_target_source: "value" (gs_rollout_evaluate_q's td_target) or "policy" (gs_rollout_evaluate_q_next's) from the
        next step of a Q learner (``Q_TARGETS``, or the number)."""
        self._check(self._lib.gs_q_set_target_source(self._h, q_target_number(source)))

    def q_get_target_source(self) -> str:
        """gs_q_get_target_source: the name of the source in force."""
        o = C.c_int32(0)
        self._check(self._lib.gs_q_get_target_source(self._h, C.byref(o)))
        return {v: k for k, v in Q_TARGETS.items()}[int(o.value)]

    def rollout_device_view(self) -> gs_rollout_device:
        """Device pointers of the last rollout (gs_rollout_device_view) for a consumer that stays on the GPU."""
        v = gs_rollout_device()
        self._check(self._lib.gs_rollout_device_view(self._h, C.byref(v)))
        return v

    def rollout_device_arrays(self) -> dict:
        """The last rollout as zero-copy ``DeviceArray`` views (``torch.as_tensor(x, device="cuda")``): ``obs_seq`` [T + 1, B, obs_dim]
        (slot t = what step t started from; ``obs_seq[1:]`` are the next observations except where an episode ended),
        ``actions`` [T, B, A], ``rewards`` [T, B], ``terminals`` [T, B] uint8 (bit 0 terminated, bit 1 truncated), and for the
        transitions that ended an episode ``terminal_index`` [n, 2] int32 (t, b) with their ``terminal_obs`` [n, obs_dim].
        Valid until the next rollout on the handle."""
        v = self.rollout_device_view()
        T, B, D, A, n = int(v.T), int(v.B), int(v.obs_dim), int(v.action_dim), int(v.n_terminal)
        return dict(obs_seq=DeviceArray(v.obs_seq, (T + 1, B, D), "<f8"), actions=DeviceArray(v.actions, (T, B, A), "<f8"),
                    rewards=DeviceArray(v.rewards, (T, B), "<f8"), terminals=DeviceArray(v.terminals, (T, B), "|u1"),
                    terminal_index=DeviceArray(v.terminal_index, (n, 2), "<i4"), terminal_obs=DeviceArray(v.terminal_obs, (n, D), "<f8"))

    # -- the device-resident dataset over the last rollout (gs_dataset_*) ---------------------------------------------------
    def dataset_build(self, keep_stats: bool = False) -> None:
        """gs_dataset_build (asynchronous): statistics and terminal map of the last rollout; ``keep_stats``: the map only."""
        self._check(self._lib.gs_dataset_build(self._h, GS_DATASET_KEEP_STATS if keep_stats else 0))

    def dataset_stats(self) -> dict:
        """gs_dataset_stats: ``n``, ``rows_per_chunk`` and the raw statistics (standard deviations WITHOUT the + 1e-6)."""
        out = dict(obs_mean=np.empty(self.obs_dim), obs_std=np.empty(self.obs_dim), act_mean=np.empty(self.action_dim),
                   act_std=np.empty(self.action_dim), reward_mean=np.empty(1), reward_std=np.empty(1))
        v = gs_dataset_stats_view(C.sizeof(gs_dataset_stats_view), 0, 0, 0, 0, *[_ptr(out[k], _dp) for k in
                                  ("obs_mean", "obs_std", "act_mean", "act_std", "reward_mean", "reward_std")])
        self._check(self._lib.gs_dataset_stats(self._h, C.byref(v)))
        out["reward_mean"], out["reward_std"] = float(out["reward_mean"][0]), float(out["reward_std"][0])
        out["n"], out["rows_per_chunk"] = int(v.n), int(v.rows_per_chunk)
        return out

    def dataset_set_stats(self, obs_mean, obs_std, act_mean, act_std, reward_mean, reward_std) -> None:
        """gs_dataset_set_stats: install raw statistics (standard deviations WITHOUT the + 1e-6) in place of the computed ones."""
        a = [_f64(np.atleast_1d(x)) for x in (obs_mean, obs_std, act_mean, act_std, reward_mean, reward_std)]
        if a[0].shape != a[1].shape or a[2].shape != a[3].shape or a[0].ndim != 1 or a[2].ndim != 1 or a[4].shape != (1,) or a[5].shape != (1,):
            raise PowerFlowError("dataset statistics: mean and std of a kind must be vectors of one length, the reward pair scalars")
        v = gs_dataset_stats_view(C.sizeof(gs_dataset_stats_view), 0, 0, a[0].shape[0], a[2].shape[0], *[_ptr(x, _dp) for x in a])
        self._check(self._lib.gs_dataset_set_stats(self._h, C.byref(v)))

    def dataset_sample(self, n: int, indices=None, seed: int = 0, draw: int = 0, dtype=np.float64, normalize: bool = True, out=None,
                       stream=None) -> dict:
        """gs_dataset_sample: one minibatch as ``DeviceArray`` views keyed like ``GridDataset.sample_batch``.  ``indices``: int64 [n]
        (host) or None (drawn on the device from ``seed`` / ``draw``); ``out``: dict of the caller's device arrays (torch tensors or
        anything ``_device_address`` takes) for some or all keys, the handle's own buffers (valid until the next call) for the rest;
        ``stream``: the consumer's stream (``_stream_arg``), None = the call returns when the batch is complete."""
        dt = np.dtype(dtype)
        if dt not in (np.dtype(np.float64), np.dtype(np.float32)):
            raise PowerFlowError(f"dataset_sample: dtype {dt} (float64 or float32)")
        n = int(n)
        idx = None
        if indices is not None:
            idx = np.ascontiguousarray(indices, dtype=np.int64)
            if idx.shape != (n,):
                raise PowerFlowError(f"dataset_sample: indices shape {idx.shape} != ({n},)")
        shapes = dict(observations=(n, self.obs_dim), actions=(n, self.action_dim), rewards=(n,), next_observations=(n, self.obs_dim),
                      terminals=(n,))
        b = gs_dataset_batch()
        for k, x in (out or {}).items():
            if k not in shapes:
                raise PowerFlowError(f"dataset_sample: unknown output {k!r}")
            setattr(b, k, _device_address_of(x, shapes[k], dt))
        self._check(self._lib.gs_dataset_sample(self._h, n, None if idx is None else idx.ctypes.data_as(C.POINTER(C.c_int64)),
                                                C.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF), C.c_uint64(int(draw) & 0xFFFFFFFFFFFFFFFF),
                                                1 if dt == np.dtype(np.float32) else 0, int(bool(normalize)), C.byref(b), _stream_arg(stream)))
        return {k: DeviceArray(getattr(b, k), shapes[k], dt.str) for k in DATASET_KEYS}

    def get_state(self) -> np.ndarray:
        st = np.empty((self.B, self.state_dim))
        self._check(self._lib.gs_get_state(self._h, _ptr(st, _dp)))
        return st

    def set_state(self, state) -> None:
        st = _f64(state)
        if st.shape != (self.B, self.state_dim):
            raise PowerFlowError(f"state shape {st.shape} != ({self.B}, {self.state_dim})")
        self._check(self._lib.gs_set_state(self._h, _ptr(st, _dp)))

    # -- multi-GPU ------------------------------------------------------------------------
    @staticmethod
    def comm_unique_id() -> bytes:
        lib = load()
        buf = (C.c_uint8 * 128)()
        rc = lib.gs_comm_unique_id(buf)
        if rc != GS_OK:
            raise PowerFlowError(f"gs_comm_unique_id failed ({rc}): {lib.gs_last_error(None).decode()}")
        return bytes(buf)

    def comm_init(self, uid: bytes, rank: int, world: int) -> None:
        buf = (C.c_uint8 * 128).from_buffer_copy(uid)
        self._check(self._lib.gs_comm_init(self._h, buf, int(rank), int(world)))
        self.world = int(world)

    def allgather_obs(self, to_host: bool = False):
        full = np.empty((self.world * self.B, self.obs_dim)) if to_host else None
        self._check(self._lib.gs_allgather_obs(self._h, _ptr(full, _dp)))
        return full

    def comm_destroy(self) -> None:
        self._check(self._lib.gs_comm_destroy(self._h))

    def comm_info(self) -> dict:
        """gs_comm_info: what the communicator itself reports about this member (RCCL's rank count, rank, device and version;
        -1 where the library lacks the entry point) and the HIP device's UUID."""
        v = gs_comm_info_t()
        self._check(self._lib.gs_comm_info(self._h, C.byref(v)))
        return {"transport": {1: "rccl", 2: "loopback"}.get(v.transport, "?"), "nranks": int(v.nranks), "rank": int(v.rank),
                "device": int(v.device), "comm_device": int(v.comm_device), "rccl_version": int(v.rccl_version),
                "device_uuid": bytes(v.device_uuid).hex()}

    @staticmethod
    def comm_init_loopback(handles) -> None:
        """gs_comm_init_loopback: the handles of this process (shard r built with first_instance = r * B) become ranks
        0 .. len - 1 of an in-process communicator whose all-gather moves the blocks by device-to-device copies."""
        lib = load()
        arr = (_H * len(handles))(*[h._h for h in handles])
        rc = lib.gs_comm_init_loopback(arr, len(handles))
        if rc != GS_OK:
            raise PowerFlowError(f"gs_comm_init_loopback failed ({rc}): {lib.gs_last_error(None).decode()}")
        for h in handles:
            h.world = len(handles)

    @staticmethod
    def allgather_obs_shards(handles, to_host: bool = False):
        """gs_allgather_obs_shards: one gather for every member; returns the [world * B, obs_dim] block (to_host) or None."""
        lib = load()
        arr = (_H * len(handles))(*[h._h for h in handles])
        full = np.empty((len(handles) * handles[0].B, handles[0].obs_dim)) if to_host else None
        rc = lib.gs_allgather_obs_shards(arr, len(handles), _ptr(full, _dp))
        if rc != GS_OK:
            raise PowerFlowError(f"gs_allgather_obs_shards failed ({rc}): {lib.gs_last_error(None).decode()} / {handles[0].last_error()}")
        return full

    def allgather_obs_view(self, stream=None) -> "DeviceArray":
        """gs_allgather_obs_view: this member's gathered block [world * B, obs_dim] as a zero-copy ``DeviceArray``."""
        v = gs_gathered_obs()
        self._check(self._lib.gs_allgather_obs_view(self._h, C.byref(v), _stream_arg(stream)))
        return DeviceArray(v.observations, (int(v.rows), int(v.obs_dim)), "<f8")

    def allgather_obs_download(self) -> np.ndarray:
        full = np.empty((self.world * self.B, self.obs_dim))
        self._check(self._lib.gs_allgather_obs_download(self._h, _ptr(full, _dp)))
        return full

    # -- measurement ----------------------------------------------------------------------
    def timing_enable(self, on: bool = True, span: bool = False) -> None:
        """Per-launch HIP event pairs (on), or one pair around the whole region up to the next timing_read() (span)."""
        self._check(self._lib.gs_timing_enable(self._h, (2 if span else 1) if on else 0))

    STAMP_NAMES = ["prologue_inject", "init", "mismatch", "bottom_up", "flag", "top_down", "final_mismatch", "epilogue_pack",
                   "prologue_scalars_rng", "prologue_chains", "epi_buses", "epi_lines", "epi_reduce", "epi_scalars", "nr_apply", "startup"]

    def debug_stamps(self) -> dict:
        buf = (C.c_uint64 * 16)()
        self._check(self._lib.gs_debug_stamps(self._h, buf, 16))
        return {n: int(buf[k]) for k, n in enumerate(self.STAMP_NAMES)}

    def debug_block_times(self, n_blocks: int) -> np.ndarray:
        """[n_blocks, 2] (start, end) of the workgroups of the last step launch, 100 MHz ticks (gs_debug_block_times)."""
        out = np.zeros((int(n_blocks), 2), dtype=np.uint64)
        self._check(self._lib.gs_debug_block_times(self._h, out.ctypes.data_as(C.POINTER(C.c_uint64)), int(n_blocks)))
        return out

    ROW_FAMILIES = {"VM": 0, "LOAD": 1, "ENVLOAD": 2, "FLOW": 3, "FREQ": 4, "CONV": 5, "ITERS": 6, "MAXMIS": 7, "LOADP": 8}

    def debug_read_rows(self, name: str) -> np.ndarray:
        """Test aid (gs_debug_read_rows): one family of device rows as a [B, width] array."""
        width = {"VM": self.n, "LOAD": self.m, "ENVLOAD": self.m, "FLOW": self.m, "LOADP": self.spec.n_loads}.get(name, 1)
        out = np.empty((self.B, width))
        if width:
            self._check(self._lib.gs_debug_read_rows(self._h, self.ROW_FAMILIES[name], out.ctypes.data_as(_dp)))
        return out

    def debug_write_rows(self, rows: dict) -> None:
        """Test aid (gs_debug_write_rows): overwrite families of device rows with [B, width] arrays; None entries are skipped."""
        for name, val in rows.items():
            if val is None:
                continue
            a = np.ascontiguousarray(np.asarray(val, dtype=np.float64).reshape(self.B, -1))
            self._check(self._lib.gs_debug_write_rows(self._h, self.ROW_FAMILIES[name], a.ctypes.data_as(_dp)))

    def timing_read(self) -> dict:
        ms = (C.c_double * 5)()
        cnt = (C.c_int64 * 5)()
        self._check(self._lib.gs_timing_read(self._h, ms, cnt))
        return {KERNEL_NAMES[k]: {"total_ms": ms[k], "launches": int(cnt[k])} for k in range(5)}
