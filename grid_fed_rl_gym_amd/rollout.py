"""Batched rollout collection -- the immediate consumer of env.step().

Mirrors the reference's ``collect_random_data(env, num_steps)`` and ``GridDataset``
(reference algorithms/base.py:268-298, 180-266): same dictionary keys, same normalisation
arithmetic.  The loop itself runs on the device (``gs_rollout``, include/gridstep.h): ``num_steps``
fused step kernels back to back, each writing its observation block straight into the next slot of a
``[T + 1, B, obs_dim]`` device buffer, random actions drawn on the device, finished instances reset in
place where the reference calls ``env.reset()`` (base.py:289-290) -- one host copy at the end, or none
(``rollout_device``).  NumPy only -- the learner side (torch) is out of scope.

``DeviceGridDataset`` is ``GridDataset`` where the collection lies: statistics reduced on the device, minibatches gathered and
normalised there (``gs_dataset_*``, include/gridstep.h), nothing copied to the host but the statistics.

``evaluate_rollout`` / ``collect_onpolicy_data`` add what a policy-gradient learner needs from a stochastic rollout -- the
log-probabilities the policy kernels recorded, a value network's estimates over every row, advantages and returns
(``gs_rollout_evaluate``); ``gae_np`` restates the device's recurrence.

``rollout_costs`` / ``evaluate_rollout_costs`` / ``collect_constrained_data`` add what a CONSTRAINED learner needs (the reference's
algorithms/safe.py): per transition and per channel (voltage, frequency, thermal) the constraint margin, the violation count and a
cost, cost critics and cost advantages (``gs_rollout_costs``, ``gs_rollout_evaluate_costs``); ``costs_np`` and
``rollout_costs_np`` restate the contract.

``rollout_episodes`` / ``EpisodeMonitor`` / ``evaluate_policy`` keep the books per EPISODE (``gs_rollout_episodes``; DESIGN.md section
17): the returns, lengths and episodic costs of the episodes a rollout finished, with per-instance carries on the device so that an
episode that straddles rollouts is one episode; ``episodes_np`` restates the contract.

``OnPolicyBatches`` turns the evaluated rollout into EPOCHS of minibatches for a clipped-surrogate learner (``gs_onpolicy_*``; DESIGN.md
section 18): a keyed permutation evaluated on the device, one gather per minibatch with the observations in the policy's
normalisation and the (Lagrangian) advantage normalised; ``permutation_np`` and ``onpolicy_batch_np`` restate the contract.

``load_rollout_data`` / ``load_rollout`` install a RECORDED dataset as the environment's rollout (``gs_rollout_load``; DESIGN.md
section 29), the inverse of ``Handle.rollout_download``: everything above then runs on it unchanged.  The rules: the arrays are
[T, B, ...] (or flat time-major), float64 or float32, one dtype for all; a finished transition's next observation goes to the
terminal list, which is in ascending ``t * B + b`` order; a LIVE transition's next observation must equal, by bits (a NaN equals the
same NaN), the observation one step later, or ``final_observation`` at the last step when one is given -- ``GS_E_INVALID`` names the
number of offenders and the first one's (t, b), and the environment then holds no rollout; log-probabilities count as recorded only
when given; everything computed over the previous rollout is stale; the environment itself is not touched and need not have been
reset; the simulator's next rollout puts the constant observation columns back.  ``transitions_to_rollout`` /
``rollout_to_transitions`` lay a flat recorded trajectory out in columns and back, marking its breaks as truncations;
``concat_rollouts`` joins consecutive rollouts; ``save_rollout`` writes the arrays with ``np.savez``.

``continue_rollout`` / ``ReplayWindow`` slide a WINDOW over consecutive rollouts (``gs_rollout_continue``): the
last ``keep`` steps of the environment's rollout move to the front on the device and ``num_steps`` fresh ones are collected behind
them, so the off-policy learners train on recent experience with no transition crossing the host; ``rollout_window_np`` restates
the result.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from types import SimpleNamespace
from typing import Dict, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from .components import PowerFlowError
from .env import BatchedGridEnvironment


def collect_random_data(env: BatchedGridEnvironment, num_steps: int, seed: int = 0,
                        actions: Optional[np.ndarray] = None, reset: bool = True) -> Dict[str, np.ndarray]:
    """``num_steps`` batched steps with uniform random actions in (-1, 1) (the reference samples
    ``env.action_space``, base.py:280) -> ``num_steps * B`` transitions, time-major
    (transition index = t * B + b).  ``actions`` ([num_steps, B, A]) overrides the sampling.
    ``reset=False`` continues from where the environment stands (the reference always resets first, base.py:277)."""
    rollout_device(env, num_steps, seed=seed, actions=actions, reset=reset)
    d = env.handle.rollout_download()
    T, B = int(num_steps), env.num_envs
    out = {k: d[k].reshape((T * B,) + d[k].shape[2:]) for k in ("observations", "actions", "rewards", "next_observations")}
    out["terminals"] = d["terminals"].reshape(T * B) != 0
    return out


def collect_policy_data(env: BatchedGridEnvironment, policy, num_steps: int, stochastic: bool = False, seed: int = 0,
                        reset: bool = True) -> Dict[str, np.ndarray]:
    """``collect_random_data`` under ``policy`` (an ``MLPPolicy``) instead of random actions: before every step one kernel
    evaluates the policy on the observation block where it lies (``gs_rollout`` with ``GS_POLICY_MLP``), an instance that
    finished being shown its fresh observation after the reset, as the reference calls ``env.reset()`` and then the policy.
    Same dictionary, same transition order.  ``stochastic``: sample the Gaussian head (noise from ``seed``)."""
    rollout_device(env, num_steps, seed=seed, reset=reset, policy=policy, stochastic=stochastic)
    d = env.handle.rollout_download()
    T, B = int(num_steps), env.num_envs
    out = {k: d[k].reshape((T * B,) + d[k].shape[2:]) for k in ("observations", "actions", "rewards", "next_observations")}
    out["terminals"] = d["terminals"].reshape(T * B) != 0
    return out


def rollout_device(env: BatchedGridEnvironment, num_steps: int, seed: int = 0, actions: Optional[np.ndarray] = None,
                   reset: bool = True, policy=None, stochastic: bool = False):
    """The same collection left on the GPU: returns the ``gs_rollout_device`` view (device pointers to
    ``obs_seq[T + 1, B, obs_dim]``, actions, rewards, done flags and the list of terminal observations) for a learner
    that consumes it there.  Valid until the next rollout on the environment.  ``policy``: an ``MLPPolicy`` to install
    and act with (``stochastic``: sample its Gaussian head), or True to act with the policy ``env.set_policy`` installed."""
    if policy is not None and actions is not None:
        raise ValueError("rollout_device: either actions or a policy")
    if reset or env._needs_reset:
        env.reset(seed=seed)
    if policy is not None:
        if policy is not True:
            env.set_policy(policy, stochastic=stochastic)
        env.handle.rollout(int(num_steps), "mlp", seed=seed)
    elif actions is None:
        env.handle.rollout(int(num_steps), "random", seed=seed)
    else:
        env.handle.rollout(int(num_steps), "uploaded", actions=np.asarray(actions, dtype=np.float64))
    return env.handle.rollout_device_view()


def gae_np(rewards, values, terminals, terminal_values, terminal_index, gamma: float = 0.99, lam: float = 0.95, bootstrap_mask: int = 0,
           reward_shift: float = 0.0, reward_scale: float = 1.0):
    """(advantages, returns), [T, B] each: the recurrence of ``gs_rollout_evaluate`` (include/gridstep.h) restated in NumPy, every
    operation IEEE float64 in the device's order.  ``rewards`` [T, B], ``values`` [T + 1, B], ``terminals`` [T, B] uint8 done flags
    (bit 0 terminated, bit 1 truncated), ``terminal_values`` [n] the values of the terminal observations of the transitions
    ``terminal_index`` [n, 2] (t, b).  ``bootstrap_mask``: the flag bits whose episode end bootstraps from its terminal value
    (0: none, the reference's ``1 - terminals``).  The tail of an unfinished episode bootstraps from ``values[T]``."""
    rewards, values = np.asarray(rewards, dtype=np.float64), np.asarray(values, dtype=np.float64)
    terminals = np.asarray(terminals).astype(np.uint8)
    T, B = rewards.shape
    term_v = np.zeros((T, B))
    idx = np.asarray(terminal_index, dtype=np.int64).reshape(-1, 2)
    term_v[idx[:, 0], idx[:, 1]] = np.asarray(terminal_values, dtype=np.float64)[:len(idx)]
    gamma, lam, mask = float(gamma), float(lam), int(bootstrap_mask)
    gl = gamma * lam
    adv, ret = np.empty((T, B)), np.empty((T, B))
    adv_next = np.zeros(B)
    for t in range(T - 1, -1, -1):
        done = terminals[t] != 0
        vnext = np.where(done, np.where((terminals[t] & mask) != 0, term_v[t], 0.0), values[t + 1])
        r = (rewards[t] - float(reward_shift)) * float(reward_scale)
        delta = (r + gamma * vnext) - values[t]
        adv[t] = np.where(done, delta, delta + gl * adv_next)
        ret[t] = adv[t] + values[t]
        adv_next = adv[t]
    return adv, ret


def _bootstrap_mask(bootstrap) -> int:
    if isinstance(bootstrap, (int, np.integer)):
        return int(bootstrap)
    names = {bootstrap} if isinstance(bootstrap, str) else set(bootstrap)
    unknown = names - set(_lib.BOOTSTRAP)
    if unknown:
        raise ValueError(f"bootstrap: unknown episode end(s) {sorted(unknown)}; any of {sorted(_lib.BOOTSTRAP)}, or the raw mask")
    return sum(_lib.BOOTSTRAP[k] for k in names)


def evaluate_rollout(env: BatchedGridEnvironment, gamma: float = 0.99, lam: float = 0.95, bootstrap: Sequence[str] = (),
                     reward_shift: float = 0.0, reward_scale: float = 1.0, stream=None):
    """Values, advantages and returns of the environment's LAST rollout, computed on the device by the value network
    ``env.set_value`` installed (``gs_rollout_evaluate``: one pass of the critic over ``obs_seq`` and the terminal observations, one
    GAE kernel).  ``bootstrap``: which episode ends bootstrap from the value of their terminal observation -- any of "terminated"
    (here: the time limit) and "truncated", or the raw mask; () is the reference's ``1 - terminals``.  Returns an object with
    ``log_probs`` [T, B] (None unless the rollout was stochastic), ``values`` [T + 1, B], ``terminal_values`` [n_terminal],
    ``advantages`` and ``returns`` [T, B] as zero-copy ``DeviceArray`` views (``torch.as_tensor(x, device="cuda")``), valid until
    the next rollout, and ``rows_per_tile``.  ``stream``: the consumer's stream handle (None: the call returns when all is there)."""
    h = env.handle
    h.rollout_evaluate(gamma, lam, _bootstrap_mask(bootstrap), reward_shift, reward_scale)
    return SimpleNamespace(**h.rollout_onpolicy_arrays(stream))


def evaluate_rollout_q(env: BatchedGridEnvironment, gamma: float = 0.99, bootstrap: Sequence[str] = (), reward_shift: float = 0.0,
                       reward_scale: float = 1.0, stream=None):
    """The twin Q networks of ``env.set_q`` over the environment's LAST rollout, on the device (``gs_rollout_evaluate_q``; after
    ``evaluate_rollout``, whose ``values`` and ``terminal_values`` it reads): per stored (observation, action) pair the value of
    every installed twin under its online and its target image, their minimum, IQL's advantage ``q_adv = min(Q1, Q2) - V`` and the
    one-step TD target ``r' + gamma * vnext`` (``vnext`` as ``gae_np`` takes it; ``bootstrap`` as ``evaluate_rollout``).  Returns an
    object with ``q`` and ``q_min`` (dicts "online" / "target"; ``q[src]`` a list of the two twins, None where not installed),
    ``q_adv`` and ``td_target``, all [T, B] zero-copy ``DeviceArray`` views valid until the next rollout, plus ``installed`` and
    ``rows_per_tile``."""
    h = env.handle
    h.rollout_evaluate_q(gamma, _bootstrap_mask(bootstrap), reward_shift, reward_scale)
    return SimpleNamespace(**h.rollout_q_arrays(stream))


def q_rollout_np(q, observations, actions, exact: bool = False) -> np.ndarray:
    """What ``gs_rollout_evaluate_q`` computes for one twin and one image: ``q`` (an ``MLPQ``) on the stored pairs ``observations``
    [T, B, obs_dim] (raw) and ``actions`` [T, B, A] (float64), as float64 [T, B].  The device contract -- the observation normalised
    in float64 and rounded once, the action rounded once, float32 layers; with ``exact`` the same rounded operands in float64
    throughout (what the float32 result is measured against)."""
    return q.forward_np(observations, actions, exact)


def td_target_np(rewards, values, terminals, terminal_values, terminal_index, gamma: float = 0.99, bootstrap_mask: int = 0,
                 reward_shift: float = 0.0, reward_scale: float = 1.0) -> np.ndarray:
    """``td_target`` [T, B] of ``gs_rollout_evaluate_q`` restated in NumPy, every operation IEEE float64 in the device's order:
    ``r' + gamma * vnext`` with the ``r'`` and ``vnext`` of ``gae_np`` (arguments as there)."""
    rewards, values = np.asarray(rewards, dtype=np.float64), np.asarray(values, dtype=np.float64)
    terminals = np.asarray(terminals).astype(np.uint8)
    T, B = rewards.shape
    term_v = np.zeros((T, B))
    idx = np.asarray(terminal_index, dtype=np.int64).reshape(-1, 2)
    term_v[idx[:, 0], idx[:, 1]] = np.asarray(terminal_values, dtype=np.float64)[:len(idx)]
    done = terminals != 0
    vnext = np.where(done, np.where((terminals & int(bootstrap_mask)) != 0, term_v, 0.0), values[1:T + 1])
    r = (rewards - float(reward_shift)) * float(reward_scale)
    return r + float(gamma) * vnext


def q_combine_np(q_online, q_target, values):
    """(q_min online, q_min target, q_adv) of ``gs_rollout_evaluate_q`` from the twins' values: ``q_online`` / ``q_target`` sequences
    of one or two [T, B] arrays (the installed twins), ``values`` [T + 1, B] (or [T, B]).  ``fmin`` over the twins; ``q_adv`` is one
    rounded float64 subtraction."""
    mins = []
    for qs in (q_online, q_target):
        qs = [np.asarray(x, dtype=np.float64) for x in qs if x is not None]
        mins.append(qs[0].copy() if len(qs) == 1 else np.fmin(qs[0], qs[1]))
    T = mins[0].shape[0]
    return mins[0], mins[1], mins[0] - np.asarray(values, dtype=np.float64)[:T]


def polyak_np(params, target, tau: float) -> np.ndarray:
    """The target update of ``gs_q_target_update`` in float32, operation by operation: ``(tau32 * p) + (omt32 * t)`` with
    ``tau32 = float32(tau)`` and ``omt32 = float32(1 - tau)`` (the difference in float64, rounded once)."""
    tau = float(tau)
    if not (math.isfinite(tau) and 0.0 <= tau <= 1.0):
        raise ValueError(f"tau = {tau} must lie in [0, 1]")
    f = np.float32
    p, t = np.asarray(params, dtype=f), np.asarray(target, dtype=f)
    return (f(tau) * p) + (f(1.0 - tau) * t)


def evaluate_rollout_q_next(env: BatchedGridEnvironment, gamma: float = 0.99, alpha: float = 0.0, bootstrap: Sequence[str] = (),
                            stochastic: bool = True, seed: int = 0, draw: int = 0, reward_shift: float = 0.0, reward_scale: float = 1.0,
                            stream=None):
    """The policy-action Bellman target over the environment's LAST rollout, on the device (``gs_rollout_evaluate_q_next``; the
    reference's ``CQL._update_critic``, algorithms/offline.py:173-178): the installed float32 tanh-Gaussian policy's action and
    log-probability at every next state (``stochastic=False``: ``a' = tanh(mean)``), every installed twin's TARGET image on it,
    their minimum, and ``td_target = r' + gamma (q_next_min - alpha next_log_probs)`` where the episode went on (``bootstrap`` as
    ``evaluate_rollout``: such an end takes the same expression on its terminal observation; any other end 0).  The noise is
    ``q_next_noise_np(seed, draw, t * B + b, A)``.  It does not need ``evaluate_rollout``.  Returns an object with
    ``next_pre_head`` [T, B, 2 A] float32, ``next_actions`` / ``next_noise`` [T, B, A], ``next_log_probs``, ``q_next_min``,
    ``td_target`` [T, B], ``q_next`` (a list of the two twins, None where not installed), the terminal list's ``term_*`` arrays
    ([n_terminal, ...]; None without a bootstrap mask), all zero-copy ``DeviceArray`` views valid until the next rollout, plus
    ``installed``, ``rows_per_tile`` and ``n_terminal``."""
    gamma, alpha = float(gamma), float(alpha)
    if not (math.isfinite(alpha) and alpha >= 0.0):
        raise ValueError(f"evaluate_rollout_q_next: alpha = {alpha} must be a finite value >= 0")
    if not isinstance(stochastic, (bool, np.bool_)):
        raise ValueError(f"evaluate_rollout_q_next: stochastic = {stochastic!r} must be True or False")
    _q_next_seed(seed, draw, "evaluate_rollout_q_next")
    h = env.handle
    h.rollout_evaluate_q_next(_lib.q_next_config(gamma, alpha, _bootstrap_mask(bootstrap), bool(stochastic), int(seed), int(draw), reward_shift,
                                                 reward_scale))
    return SimpleNamespace(**h.rollout_q_next_arrays(stream))


def refresh_targets(env: BatchedGridEnvironment, batch, groups, gamma: float = 0.99, alpha: float = 0.0, bootstrap: Sequence[str] = (),
                    stochastic: bool = True, seed: int = 0, draw: int = 0, reward_shift: float = 0.0, reward_scale: float = 1.0,
                    stream=None) -> None:
    """Per-minibatch targets (``gs_learner_refresh``, asynchronous): the signal ``groups`` -- names of
    ``_lib.REFRESH_GROUPS`` ("td_policy", "q_target", "td_value", "q_adv"), one or several, or the bits -- re-evaluated for the
    transitions ``batch["indices"]`` names (a minibatch of ``OnPolicyBatches.epoch``, or any dict with a device int32 array of
    ``t * B + b``) under the networks as they are NOW, and written into the arrays of ``evaluate_rollout_q_next`` ("td_policy") /
    ``evaluate_rollout_q`` (the others) at those transitions; every other position keeps its bits.  What the reference's
    ``update(batch)`` recomputes per minibatch (algorithms/offline.py:173-178, :482-540).  The evaluation a group replaces rows of
    must have run on the last rollout ("td_policy": under the same ``bootstrap``).  The other arguments are
    ``evaluate_rollout_q_next``'s; the noise of row j is ``q_next_noise_np(seed, draw, [j], A)``.  ``refresh_rows_np`` restates
    which rows are read."""
    gamma, alpha = float(gamma), float(alpha)
    bits = _lib.refresh_groups(groups)
    if bits <= 0 or bits & ~sum(_lib.REFRESH_GROUPS.values()):
        raise ValueError(f"refresh_targets: groups = {groups!r} names no group or an unknown one (any of {sorted(_lib.REFRESH_GROUPS)})")
    if not (math.isfinite(alpha) and alpha >= 0.0):
        raise ValueError(f"refresh_targets: alpha = {alpha} must be a finite value >= 0")
    if not isinstance(stochastic, (bool, np.bool_)):
        raise ValueError(f"refresh_targets: stochastic = {stochastic!r} must be True or False")
    _q_next_seed(seed, draw, "refresh_targets")
    if not hasattr(batch, "get") or batch.get("indices") is None:
        raise ValueError("refresh_targets: the batch holds no 'indices'")
    env.handle.learner_refresh(batch, _lib.refresh_config(bits, gamma, alpha, _bootstrap_mask(bootstrap), bool(stochastic), int(seed), int(draw),
                                                          reward_shift, reward_scale), stream=stream)


def refresh_rows_np(indices, T: int, B: int, terminals, terminal_index, bootstrap_mask: int = 0):
    """Which rows ``gs_learner_refresh`` reads for the batch ``indices`` [n] over a rollout of ``T`` steps and ``B`` instances,
    restated in NumPy: (own [n], next [n], pairs [m, 2]).  ``own[i]`` = j_i, the index clamped into [0, T B): row j_i of the
    flattened ``obs_seq`` [(T + 1) B, obs_dim] is the transition's state; ``next[i]`` = j_i + B its next state; ``pairs``: the
    (i, e) of every batch row whose transition ended an episode under the mask (``terminals`` [T, B] & ``bootstrap_mask``) and has
    an entry e in ``terminal_index`` [(t, b)] -- in ascending i, a duplicate index once per occurrence; where an (t, b) occurs
    more than once in the list the LAST entry counts (the device's map is scattered in list order)."""
    idx = np.asarray(indices)
    if idx.ndim != 1 or (idx.size and not np.issubdtype(idx.dtype, np.integer)):
        raise ValueError("refresh_rows_np: indices must be a one-dimensional array of integers")
    T, B, mask = int(T), int(B), int(bootstrap_mask)
    if T <= 0 or B <= 0:
        raise ValueError(f"refresh_rows_np: T = {T} and B = {B} must be > 0")
    if not 0 <= mask <= 3:
        raise ValueError(f"refresh_rows_np: bootstrap_mask = {mask} outside 0 .. 3")
    flags = np.asarray(terminals).astype(np.uint8)
    if flags.shape != (T, B):
        raise ValueError(f"refresh_rows_np: terminals must be [{T}, {B}], got {flags.shape}")
    own = np.clip(idx.astype(np.int64), 0, T * B - 1)
    entry = np.full(T * B, -1, dtype=np.int64)
    tb = np.asarray(terminal_index, dtype=np.int64).reshape(-1, 2)
    inside = (tb[:, 0] >= 0) & (tb[:, 0] < T) & (tb[:, 1] >= 0) & (tb[:, 1] < B)
    entry[(tb[:, 0] * B + tb[:, 1])[inside]] = np.nonzero(inside)[0]
    hit = ((flags.reshape(-1)[own] & mask) != 0) & (entry[own] >= 0)
    rows = np.nonzero(hit)[0]
    return own, own + B, np.stack([rows, entry[own[rows]]], axis=1).astype(np.int64).reshape(-1, 2)


def _q_next_seed(seed, draw, who: str) -> None:
    integer = lambda x: isinstance(x, (int, np.integer)) and not isinstance(x, (bool, np.bool_))
    if not integer(seed) or not 0 <= int(seed) < 1 << 64:
        raise ValueError(f"{who}: seed = {seed!r} must be an integer in [0, 2^64)")
    if not integer(draw) or not 0 <= int(draw) < 1 << 32:
        raise ValueError(f"{who}: draw = {draw!r} must be an integer in [0, 2^32)")


def q_next_noise_np(seed: int, draw: int, index, A: int, terminal: bool = False) -> np.ndarray:
    """eps [n, A] of ``gs_rollout_evaluate_q_next`` for the transitions ``index`` [n] (``t * B + b`` each; NOT a row's place in a
    list): ``eps[j, k]`` = component ``k & 3`` of the four normals of Philox4x32-10 with counter (index[j], k >> 2, draw, tag) and
    key ``seed`` -- ``pathwise_noise_np``'s recipe (every word w a uniform (w + 1/2) 2^-32, words (0, 1) and (2, 3) one Box-Muller
    pair each, cosine then sine).  tag: 'QNXT' for the rollout's rows, 'QNTE' (``terminal``) for the terminal observations."""
    _q_next_seed(seed, draw, "q_next_noise_np")
    A = int(A)
    idx = np.asarray(index)
    if A <= 0:
        raise ValueError(f"q_next_noise_np: A = {A} must be > 0")
    if idx.ndim != 1 or (idx.size and (not np.issubdtype(idx.dtype, np.integer) or idx.min() < 0 or idx.max() >= 1 << 32)):
        raise ValueError("q_next_noise_np: index must be a one-dimensional array of integers in [0, 2^32)")
    n, quads = idx.size, (A + 3) // 4
    i = np.repeat(idx.astype(np.uint64), quads)
    q = np.tile(np.arange(quads, dtype=np.uint64), n)
    full = lambda x: np.full(i.shape, int(x) & 0xFFFFFFFF, dtype=np.uint64)
    tag = _lib.Q_NEXT_TERMINAL_TAG if terminal else _lib.Q_NEXT_ROLLOUT_TAG
    seed = int(seed)
    w = np.stack(_philox4x32(i, q, full(draw), full(tag), seed & 0xFFFFFFFF, seed >> 32), axis=1).astype(np.float64)
    u = (w + 0.5) * (1.0 / 4294967296.0)
    ra, rb = np.sqrt(-2.0 * np.log(u[:, 0])), np.sqrt(-2.0 * np.log(u[:, 2]))
    ta, tb = 2.0 * math.pi * u[:, 1], 2.0 * math.pi * u[:, 3]
    z = np.stack([ra * np.cos(ta), ra * np.sin(ta), rb * np.cos(tb), rb * np.sin(tb)], axis=1)
    return z.reshape(n, 4 * quads)[:, :A].copy()


def policy_rows_np(policy, observations, eps, exact: bool = False, pre_head=None):
    """(pre_head [n, 2 A], actions [n, A], log_probs [n]) of ``gs_k_policy_rows_f32`` restated in NumPy: ``policy`` (an ``MLPPolicy``
    with the Gaussian head) on raw ``observations`` [n, obs_dim] under the float32 device contract (``exact``: the same rounded
    operands in float64 throughout, what the float32 result is measured against), then the sampling head of the pathwise actor
    step (``learner._pathwise_sample``: ITS exp, tanh and log, float64 on the pre-head values) with the noise ``eps`` [n, A]; None is
    the deterministic actor, eps = 0.  ``pre_head``: values to run the head on in place of the layers' (the device's own, for a
    bit-for-bit statement of the head)."""
    from .learner import _pathwise_sample      # (learner.py imports this module)

    if getattr(policy, "head", None) != "gaussian_tanh":
        raise ValueError("policy_rows_np: the policy needs the Gaussian head (mean | log_std)")
    obs = np.asarray(observations, dtype=np.float64)
    if obs.ndim != 2 or obs.shape[1] != policy.obs_dim:
        raise ValueError(f"policy_rows_np: observations must be [n, {policy.obs_dim}], got {obs.shape}")
    n, A = obs.shape[0], policy.action_dim
    if pre_head is None:
        pre = policy.pre_head_np(obs, "float32", exact)
    else:
        pre = np.asarray(pre_head)
        if pre.shape != (n, 2 * A):
            raise ValueError(f"policy_rows_np: pre_head must be [{n}, {2 * A}], got {pre.shape}")
    if eps is None:
        eps = np.zeros((n, A))
    eps = np.asarray(eps, dtype=np.float64)
    if eps.shape != (n, A):
        raise ValueError(f"policy_rows_np: eps must be [{n}, {A}], got {eps.shape}")
    _, _, _, a, lp = _pathwise_sample(pre.astype(np.float64), eps)
    return pre, a, lp


def td_policy_np(rewards, next_log_probs, q_next_min, terminals, terminal_q, terminal_index, gamma: float = 0.99, alpha: float = 0.0,
                 bootstrap_mask: int = 0, reward_shift: float = 0.0, reward_scale: float = 1.0, terminal_log_probs=None) -> np.ndarray:
    """``td_target`` [T, B] of ``gs_rollout_evaluate_q_next`` restated in NumPy, every operation IEEE float64 in the device's order:
    ``r' + gamma * v`` with ``r' = (rewards - reward_shift) * reward_scale`` and ``v = q_next_min - alpha * next_log_probs`` where
    the transition did not end an episode, the terminal entry's value where it did and its flag meets ``bootstrap_mask``, 0
    otherwise (mask 0: the reference's ``1 - terminals``, algorithms/offline.py:175-178).  The terminal entry's value for the
    transition ``terminal_index[e]`` (t, b): ``terminal_q[e] - alpha * terminal_log_probs[e]`` (the device's ``term_q_min`` and
    ``term_log_probs``), or ``terminal_q[e]`` itself without ``terminal_log_probs`` (the device's ``term_value``)."""
    rewards = np.asarray(rewards, dtype=np.float64)
    lp, qm = np.asarray(next_log_probs, dtype=np.float64), np.asarray(q_next_min, dtype=np.float64)
    terminals = np.asarray(terminals).astype(np.uint8)
    if rewards.ndim != 2 or lp.shape != rewards.shape or qm.shape != rewards.shape or terminals.shape != rewards.shape:
        raise ValueError(f"td_policy_np: rewards, next_log_probs, q_next_min and terminals must share one [T, B] shape, got {rewards.shape}, "
                         f"{lp.shape}, {qm.shape}, {terminals.shape}")
    gamma, alpha, mask = float(gamma), float(alpha), int(bootstrap_mask)
    if not math.isfinite(gamma):
        raise ValueError(f"td_policy_np: gamma = {gamma} must be finite")
    if not (math.isfinite(alpha) and alpha >= 0.0):
        raise ValueError(f"td_policy_np: alpha = {alpha} must be a finite value >= 0")
    if not 0 <= mask <= 3:
        raise ValueError(f"td_policy_np: bootstrap_mask = {mask} outside 0 .. 3")
    T, B = rewards.shape
    idx = np.asarray(terminal_index, dtype=np.int64).reshape(-1, 2)
    tq = np.asarray(terminal_q, dtype=np.float64).reshape(-1)
    if mask and len(tq) < len(idx):
        raise ValueError(f"td_policy_np: {len(idx)} terminal entries but {len(tq)} terminal values")
    term_v = np.zeros((T, B))
    if mask and len(idx):
        tv = tq[:len(idx)]
        if terminal_log_probs is not None:
            tv = tv - alpha * np.asarray(terminal_log_probs, dtype=np.float64).reshape(-1)[:len(idx)]
        term_v[idx[:, 0], idx[:, 1]] = tv
    done = terminals != 0
    v = qm - alpha * lp
    vnext = np.where(done, np.where((terminals & mask) != 0, term_v, 0.0), v)
    r = (rewards - float(reward_shift)) * float(reward_scale)
    return r + gamma * vnext


def collect_onpolicy_data(env: BatchedGridEnvironment, policy, value, num_steps: int, seed: int = 0, reset: bool = True,
                          gamma: float = 0.99, lam: float = 0.95, bootstrap: Sequence[str] = (), reward_shift: float = 0.0,
                          reward_scale: float = 1.0) -> Dict[str, np.ndarray]:
    """``collect_policy_data`` under the STOCHASTIC ``policy`` plus what a policy-gradient update needs, as host arrays in the
    same transition order (index = t * B + b): ``log_probs``, ``values`` (of ``observations``), ``advantages`` and ``returns``
    under the value network ``value`` (an ``MLPValue``), all computed on the device."""
    rollout_device(env, num_steps, seed=seed, reset=reset, policy=policy, stochastic=True)
    env.set_value(value)
    env.handle.rollout_evaluate(gamma, lam, _bootstrap_mask(bootstrap), reward_shift, reward_scale)
    d = env.handle.rollout_download()
    T, B = int(num_steps), env.num_envs
    out = {k: d[k].reshape((T * B,) + d[k].shape[2:]) for k in ("observations", "actions", "rewards", "next_observations")}
    out["terminals"] = d["terminals"].reshape(T * B) != 0
    o = env.handle.rollout_onpolicy_download(("log_probs", "values", "advantages", "returns"))
    out["log_probs"], out["values"] = o["log_probs"].reshape(T * B), o["values"][:T].reshape(T * B)
    out["advantages"], out["returns"] = o["advantages"].reshape(T * B), o["returns"].reshape(T * B)
    return out


# ---- constraint costs (include/gridstep.h "constraint costs of a rollout") --------------------------------------

@dataclass
class ConstraintLimits:
    """The limits of the three constraint channels: ``voltage`` (lo, hi) per unit, ``frequency`` (lo, hi) Hz, ``thermal`` the line
    loading limit.  ``ConstraintLimits.of(env)``: the environment's own voltage and frequency limits and 0.8, the threshold of the
    reference's reward (grid_env.py:785-826) and ``thermal_constraint``'s default (safe.py:554)."""
    voltage: Tuple[float, float] = (0.95, 1.05)
    frequency: Tuple[float, float] = (59.5, 60.5)
    thermal: float = 0.8

    @classmethod
    def of(cls, env, **override) -> "ConstraintLimits":
        kw = dict(voltage=tuple(env.voltage_limits), frequency=tuple(env.frequency_limits), thermal=0.8)
        kw.update(override)
        return cls(**kw)


def _nm(spec_or_nm) -> Tuple[int, int]:
    if hasattr(spec_or_nm, "n") and hasattr(spec_or_nm, "m"):
        return int(spec_or_nm.n), int(spec_or_nm.m)
    n, m = spec_or_nm
    return int(n), int(m)


def _kinds(kinds):
    ks = [kinds] * 3 if isinstance(kinds, (str, int, np.integer)) else list(kinds)
    if len(ks) != 3:
        raise ValueError(f"kinds: one kind or three, got {len(ks)}")
    return [_lib.COST_KIND[k] if isinstance(k, str) else int(k) for k in ks]


def costs_np(obs, spec_or_nm, limits: ConstraintLimits, kinds="excess"):
    """(margins float64, counts int32, costs float64), [..., 3] each, of observation rows ``obs`` [..., obs_dim]: the contract of
    ``gs_rollout_costs`` (include/gridstep.h) restated in NumPy.  ``spec_or_nm``: a ``FeederSpec`` or (n, m).  Only the first
    2 n + 2 m + 1 columns are read: |V| at 2 i, the line loading at 2 n + 2 k + 1, the frequency at 2 n + 2 m."""
    obs = np.asarray(obs, dtype=np.float64)
    n, m = _nm(spec_or_nm)
    vm = obs[..., 0:2 * n:2]
    load = np.abs(obs[..., 2 * n + 1:2 * n + 2 * m:2])
    f = obs[..., 2 * n + 2 * m]
    (vlo, vhi), (flo, fhi), lim = limits.voltage, limits.frequency, float(limits.thermal)
    margins = np.empty(obs.shape[:-1] + (3,))
    with np.errstate(invalid="ignore"):
        margins[..., 0] = np.min(np.minimum(vm - vlo, vhi - vm), axis=-1)                       # safe.py:513-522
        margins[..., 1] = np.minimum(f - flo, fhi - f)                                          # safe.py:534-542
        margins[..., 2] = lim - np.max(load, axis=-1) if m else lim                             # safe.py:554-561
        counts = np.stack([np.sum((vm < vlo) | (vm > vhi), axis=-1), ((f < flo) | (f > fhi)).astype(np.int64),   # base.py:153-167
                           np.sum(load > lim, axis=-1)], axis=-1).astype(np.int32)
        neg = margins < 0.0
    by_kind = (np.where(neg, -margins, 0.0),            # excess, safe.py:471 (a NaN margin: 0)
               np.where(neg, 1.0, 0.0),                 # indicator, safe.py:282
               counts.astype(np.float64))
    costs = np.stack([by_kind[k][..., c] for c, k in enumerate(_kinds(kinds))], axis=-1)
    return margins, counts, costs


def rollout_costs_np(next_observations, spec_or_nm, limits: ConstraintLimits, kinds="excess"):
    """``costs_np`` over a downloaded rollout: ``next_observations`` [T, B, obs_dim] (or [T * B, obs_dim]) as ``rollout_download`` /
    ``collect_*_data`` return them -- the terminal observation where the transition ended an episode, not the fresh one after the
    reset.  Returns margins, counts, costs channel-major, [3, T, B] (or [3, T * B]), and n_violating [3] int64."""
    margins, counts, costs = costs_np(next_observations, spec_or_nm, limits, kinds)
    cm = lambda a: np.ascontiguousarray(np.moveaxis(a, -1, 0))
    margins = cm(margins)
    with np.errstate(invalid="ignore"):
        n_violating = np.sum(margins.reshape(3, -1) < 0.0, axis=1).astype(np.int64)
    return margins, cm(counts), cm(costs), n_violating


def rollout_costs(env: BatchedGridEnvironment, limits: Optional[ConstraintLimits] = None, kinds="excess", stream=None):
    """Constraint margins, violation counts and costs of every transition of the environment's LAST rollout, computed on the device
    (``gs_rollout_costs``: one streaming kernel over the first 2 n + 2 m + 1 columns of ``obs_seq[1:]`` and of the terminal
    observations).  ``limits``: None = ``ConstraintLimits.of(env)``; ``kinds``: "excess", "indicator" or "count", one or three.
    Returns an object with ``margins``, ``costs`` (float64), ``counts`` (int32), [3, T, B] zero-copy ``DeviceArray`` views (channel
    order ``_lib.COST_CHANNELS``), and ``n_violating`` [3] int64; valid until the next rollout.  ``stream``: as ``evaluate_rollout``."""
    h = env.handle
    h.rollout_costs(_lib.cost_config(ConstraintLimits.of(env) if limits is None else limits, kinds))
    a = h.rollout_costs_arrays(stream)
    return SimpleNamespace(margins=a["margins"], counts=a["counts"], costs=a["costs"], n_violating=a["n_violating"])


def evaluate_rollout_costs(env: BatchedGridEnvironment, gamma=0.99, lam=0.95, bootstrap: Sequence[str] = (), cost_shift=0.0, cost_scale=1.0,
                           stream=None):
    """Cost values, cost advantages and cost returns of the LAST rollout under the cost critics ``env.set_cost_value`` installed
    (``gs_rollout_evaluate_costs``, after ``rollout_costs``): per channel the critic over ``obs_seq`` and the terminal observations
    and the recurrence of ``evaluate_rollout`` with that channel's costs as rewards.  ``gamma``, ``lam``, ``cost_shift``,
    ``cost_scale``: a scalar or one per channel; ``bootstrap`` is shared.  Returns an object whose ``values``, ``terminal_values``,
    ``advantages`` and ``returns`` are lists of three ``DeviceArray`` views, None for a channel without a critic."""
    h = env.handle
    h.rollout_evaluate_costs(gamma, lam, _bootstrap_mask(bootstrap), cost_shift, cost_scale)
    a = h.rollout_costs_arrays(stream)
    return SimpleNamespace(**{k: a[k] for k in _lib.COST_CRITIC_KEYS})


def constraint_values(env: BatchedGridEnvironment, observations, limits: Optional[ConstraintLimits] = None, kinds="excess") -> Dict[str, np.ndarray]:
    """``margins``, ``counts`` and ``costs``, [rows, 3] each, of host ``observations`` [rows, obs_dim] (``gs_costs_eval``): the
    reference's constraint values (safe.py:26-32, >= 0 is safe) of arbitrary rows, e.g. what ``env.step`` returned."""
    return env.handle.costs_eval(observations, _lib.cost_config(ConstraintLimits.of(env) if limits is None else limits, kinds))


def collect_constrained_data(env: BatchedGridEnvironment, policy, value, cost_values, num_steps: int, seed: int = 0, reset: bool = True,
                             limits: Optional[ConstraintLimits] = None, kinds="excess", gamma: float = 0.99, lam: float = 0.95,
                             bootstrap: Sequence[str] = (), reward_shift: float = 0.0, reward_scale: float = 1.0, cost_gamma=0.99,
                             cost_lam=0.95, cost_shift=0.0, cost_scale=1.0) -> Dict[str, np.ndarray]:
    """``collect_onpolicy_data`` plus the constraint signals, as host arrays in the same transition order (index = t * B + b):
    ``constraint_margins`` and ``constraint_costs`` [T * B, 3], and ``cost_advantages`` / ``cost_returns``, dicts from the channel
    index to [T * B] for the channels with a critic.  ``cost_values``: a dict channel (index or name in ``_lib.COST_CHANNELS``) ->
    ``MLPValue``, or a sequence of three with None for a channel without one; these replace the installed cost critics."""
    if isinstance(cost_values, dict):
        given = {(_lib.COST_CHANNELS.index(c) if isinstance(c, str) else int(c)): v for c, v in cost_values.items()}
    else:
        given = {c: v for c, v in enumerate(cost_values)}
    out = collect_onpolicy_data(env, policy, value, num_steps, seed=seed, reset=reset, gamma=gamma, lam=lam, bootstrap=bootstrap,
                                reward_shift=reward_shift, reward_scale=reward_scale)
    h = env.handle
    for c in range(3):
        env.set_cost_value(c, given.get(c))
    critics = tuple(c for c in range(3) if given.get(c) is not None)
    h.rollout_costs(_lib.cost_config(ConstraintLimits.of(env) if limits is None else limits, kinds))
    if critics:
        h.rollout_evaluate_costs(cost_gamma, cost_lam, _bootstrap_mask(bootstrap), cost_shift, cost_scale)
    T, B = int(num_steps), env.num_envs
    d = h.rollout_costs_download(("margins", "costs", "advantages", "returns") if critics else ("margins", "costs"), channels=critics)
    out["constraint_margins"] = np.ascontiguousarray(d["margins"].reshape(3, T * B).T)
    out["constraint_costs"] = np.ascontiguousarray(d["costs"].reshape(3, T * B).T)
    out["cost_advantages"] = {c: d["advantages"][c].reshape(T * B) for c in critics}
    out["cost_returns"] = {c: d["returns"][c].reshape(T * B) for c in critics}
    return out


# ---- episode accounting (include/gridstep.h "episode accounting") -------------------------------------------------

def _success_floor(success_return) -> float:
    f = float(success_return)
    if np.isnan(f) or f == np.inf:
        raise ValueError("success_return must be finite or -inf")
    return f


def _episode_stats_np(rec: dict, with_costs: bool, success_return: float) -> SimpleNamespace:
    """``gs_episode_stats`` of a record list, in NumPy (np.mean / np.std: the device's own order is DESIGN.md section 17's)."""
    full = (rec["episode_flags"] & _lib.GS_EPISODE_PARTIAL) == 0
    ret, length = rec["episode_return"][full], rec["episode_length"][full]
    n = int(full.sum())
    nan = float("nan")
    clean = rec["episode_any_violating"][full] == 0 if with_costs else np.ones(n, dtype=bool)
    return SimpleNamespace(
        count=n, count_partial=int(len(full) - n),
        return_mean=float(np.mean(ret)) if n else nan, return_std=float(np.std(ret)) if n else nan,
        return_min=float(np.min(ret)) if n else nan, return_max=float(np.max(ret)) if n else nan,
        length_mean=float(np.mean(length)) if n else nan, length_min=float(np.min(length)) if n else nan,
        length_max=float(np.max(length)) if n else nan,
        cost_mean=np.array([float(np.mean(rec["episode_cost"][c][full])) if n and with_costs else nan for c in range(3)]),
        violating=np.array([int(rec["episode_violating"][c][full].sum()) if with_costs else 0 for c in range(3)], dtype=np.int64),
        n_success=int(np.sum(clean & (ret > success_return))))


def episodes_np(rewards, terminals, costs=None, margins=None, carry=None, start="fresh", success_return: float = -1000.0):
    """(records, stats, carry): the contract of ``gs_rollout_episodes`` (include/gridstep.h) restated in NumPy, operation by operation.
    ``rewards`` [T, B] float64 and ``terminals`` [T, B] uint8 done flags of one rollout; with ``costs`` and ``margins`` [3, T, B]
    (``rollout_costs``) the episodic costs and violating steps as well.  Per instance, t = 0 .. T-1 in order: ``ret = ret + r``, one
    rounded float64 addition per step; ``len += 1``; ``cost[c] = cost[c] + costs[c, t, b]``; a step violates channel c where
    ``margins[c, t, b] < 0`` (a NaN margin counts as nothing); where ``terminals[t, b] != 0`` a record is filed and the carries start
    again from zero with ``ordinal + 1``.  ``start``: "fresh" (zero carries, nothing partial), "unknown" (zero carries, every instance's
    open episode partial) or "continue" (``carry`` as a previous call returned it).
    ``records``: a dict of ``episode_index`` [n, 2] (t_end, b), ``episode_return``, ``episode_length``, ``episode_ordinal``,
    ``episode_flags`` (the done flag's bits 0, 1; 4 = partial) and with costs ``episode_cost`` / ``episode_violating`` [3, n] and
    ``episode_any_violating`` [n], sorted by (b, t_end).  ``stats``: the fields of ``gs_episode_stats`` over the complete records.
    ``carry``: ``ep_return``, ``ep_length``, ``ep_ordinal``, ``ep_partial`` [B] and with costs ``ep_cost`` / ``ep_violating`` [3, B],
    ``ep_any_violating`` [B]."""
    floor = _success_floor(success_return)
    rewards = np.asarray(rewards, dtype=np.float64)
    terminals = np.asarray(terminals).astype(np.uint8)
    T, B = rewards.shape
    with_costs = costs is not None
    if with_costs != (margins is not None):
        raise ValueError("episodes_np: costs and margins go together")
    if start not in _lib.EPISODES_START:
        raise ValueError(f"episodes_np: start {start!r} is none of {sorted(_lib.EPISODES_START)}")
    if start == "continue":
        if carry is None:
            raise ValueError("episodes_np: start='continue' needs the carry of the previous call")
        if with_costs != ("ep_cost" in carry):
            raise ValueError("episodes_np: the carry was made with costs " + ("off" if with_costs else "on"))
        ret, length, ordinal = carry["ep_return"].astype(np.float64), carry["ep_length"].astype(np.int32), carry["ep_ordinal"].astype(np.int32)
        partial = carry["ep_partial"].astype(np.uint8)
        if with_costs:
            cost, viol, anyv = carry["ep_cost"].astype(np.float64), carry["ep_violating"].astype(np.int32), carry["ep_any_violating"].astype(np.int32)
    else:
        ret, length, ordinal = np.zeros(B), np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.int32)
        partial = np.full(B, 1 if start == "unknown" else 0, dtype=np.uint8)
        cost, viol, anyv = np.zeros((3, B)), np.zeros((3, B), dtype=np.int32), np.zeros(B, dtype=np.int32)
    if with_costs:
        costs, margins = np.asarray(costs, dtype=np.float64).reshape(3, T, B), np.asarray(margins, dtype=np.float64).reshape(3, T, B)
    filed = {k: [] for k in ("t", "b", "ret", "len", "ord", "flags", "cost", "viol", "anyv")}
    for t in range(T):
        ret = ret + rewards[t]
        length = length + 1
        if with_costs:
            cost = cost + costs[:, t]
            with np.errstate(invalid="ignore"):
                bad = margins[:, t] < 0.0
            viol = viol + bad
            anyv = anyv + bad.any(axis=0)
        done = np.nonzero(terminals[t] != 0)[0]
        if len(done):
            filed["t"].append(np.full(len(done), t, dtype=np.int32)); filed["b"].append(done.astype(np.int32))
            filed["ret"].append(ret[done]); filed["len"].append(length[done]); filed["ord"].append(ordinal[done])
            filed["flags"].append((terminals[t, done] & 3).astype(np.int32) | np.where(partial[done] != 0, _lib.GS_EPISODE_PARTIAL, 0).astype(np.int32))
            if with_costs:
                filed["cost"].append(cost[:, done]); filed["viol"].append(viol[:, done]); filed["anyv"].append(anyv[done])
                cost[:, done] = 0.0; viol[:, done] = 0; anyv[done] = 0
            ret[done] = 0.0; length[done] = 0; ordinal[done] += 1; partial[done] = 0
    cat = lambda k, dt, axis=0, empty=(0,): np.concatenate(filed[k], axis=axis).astype(dt) if filed[k] else np.zeros(empty, dtype=dt)
    t_end, b_of = cat("t", np.int32), cat("b", np.int32)
    order = np.lexsort((t_end, b_of))        # by b, then t_end
    rec = dict(episode_index=np.stack([t_end, b_of], axis=1)[order].astype(np.int32), episode_return=cat("ret", np.float64)[order],
               episode_length=cat("len", np.int32)[order], episode_ordinal=cat("ord", np.int32)[order], episode_flags=cat("flags", np.int32)[order])
    new_carry = dict(ep_return=ret, ep_length=length.astype(np.int32), ep_ordinal=ordinal.astype(np.int32), ep_partial=partial)
    if with_costs:
        rec.update(episode_cost=cat("cost", np.float64, 1, (3, 0))[:, order], episode_violating=cat("viol", np.int32, 1, (3, 0))[:, order],
                   episode_any_violating=cat("anyv", np.int32)[order])
        new_carry.update(ep_cost=cost, ep_violating=viol.astype(np.int32), ep_any_violating=anyv.astype(np.int32))
    return rec, _episode_stats_np(rec, with_costs, floor), new_carry


class EpisodeRecords:
    """What ``rollout_episodes`` left on the device: the list arrays (``episode_index`` [n, 2] (t_end, b), ``episode_return``,
    ``episode_length``, ``episode_ordinal``, ``episode_flags`` [n]; with costs ``episode_cost`` and ``episode_violating``, lists of
    three [n] per channel, and ``episode_any_violating``) and the carries (``ep_return``, ``ep_length``, ``ep_ordinal``,
    ``ep_partial`` [B]; with costs ``ep_cost``, ``ep_violating`` [3, B], ``ep_any_violating``) as zero-copy ``DeviceArray`` views
    (``torch.as_tensor(x, device="cuda")``; None where there are no costs); ``n_episodes``; and ``stats``, a host object with the
    fields of ``gs_episode_stats``.  The list is valid until the next rollout or accounting.  ``download()``: host copies, the cost
    arrays [3, n]."""

    def __init__(self, handle, arrays: dict, stats) -> None:
        self._handle = handle
        self.n_episodes, self.with_costs = arrays["n_episodes"], arrays["with_costs"]
        for k, _ in _lib.EPISODE_LIST_KEYS + _lib.EPISODE_CARRY_KEYS:
            setattr(self, k, arrays[k])
        self.stats = stats

    def download(self, want=None) -> dict:
        return self._handle.rollout_episodes_download(want, n_episodes=self.n_episodes)


def _stats_object(s) -> SimpleNamespace:
    """A ``gs_episode_stats`` as a plain host object (``cost_mean`` float64 [3], ``violating`` int64 [3])."""
    return SimpleNamespace(count=int(s.count), count_partial=int(s.count_partial), return_mean=float(s.return_mean), return_std=float(s.return_std),
                           return_min=float(s.return_min), return_max=float(s.return_max), length_mean=float(s.length_mean),
                           length_min=float(s.length_min), length_max=float(s.length_max), cost_mean=np.array(list(s.cost_mean), dtype=np.float64),
                           violating=np.array(list(s.violating), dtype=np.int64), n_success=int(s.n_success))


def rollout_episodes(env: BatchedGridEnvironment, start: str = "continue", costs: bool = False, success_return: float = -1000.0,
                     stream=None) -> EpisodeRecords:
    """The episodes the environment's LAST rollout finished -- return, length, ordinal, end flags and, with ``costs`` (after
    ``rollout_costs``), episodic cost and violating steps per channel -- and the carries of the episodes still open, computed on the
    device (``gs_rollout_episodes``).  An episode that straddles rollouts is one episode: ``start="continue"`` takes the carries the
    previous accounted rollout left; "fresh" states that ``env.reset()`` came directly before the rollout; "unknown" marks every
    instance's open episode partial (left out of ``stats``).  ``success_return``: an episode succeeds with no violating step and a
    return above it (the reference's -1000; -inf: no floor).  ``stream``: as ``evaluate_rollout``."""
    h = env.handle
    h.rollout_episodes(_lib.episode_config(start, costs, _success_floor(success_return)))
    arrays = h.rollout_episodes_arrays(stream)
    stats = h.rollout_episodes_download(("stats",), n_episodes=arrays["n_episodes"])["stats"]
    return EpisodeRecords(h, arrays, _stats_object(stats))


class EpisodeMonitor:
    """A learning curve over device rollouts: after every rollout ``update()`` accounts its episodes on the device
    (``rollout_episodes``) and merges the rollout's statistics into running ones on the host -- Chan's merge on (count, mean, M2) --
    and keeps the last ``window`` complete returns and lengths.  ``after_reset()`` tells it that ``env.reset()`` came before the
    next rollout ("fresh"); otherwise it continues, and before its first rollout it assumes nothing ("unknown": the open episodes
    are partial and left out).  Reports ``count``, ``mean_return``, ``std_return``, ``min_return``, ``max_return``, ``mean_length``,
    ``mean_cost`` [3], ``violating`` [3], ``success_rate``; ``window_mean_return`` / ``window_mean_length`` over the window."""

    def __init__(self, env: Optional[BatchedGridEnvironment] = None, window: int = 100) -> None:
        from collections import deque
        self.env, self._start = env, "unknown"
        self.returns, self.lengths = deque(maxlen=int(window)), deque(maxlen=int(window))
        self.count, self.count_partial, self._mean, self._m2 = 0, 0, 0.0, 0.0
        self.min_return, self.max_return = float("nan"), float("nan")
        self._length_total, self._cost_mean, self._cost_count = 0, np.zeros(3), 0
        self.violating, self.n_success = np.zeros(3, dtype=np.int64), 0

    def after_reset(self) -> None:
        self._start = "fresh"

    def update(self, costs: bool = False, success_return: float = -1000.0, stream=None) -> EpisodeRecords:
        rec = rollout_episodes(self.env, self._start, costs, success_return, stream)
        self._start = "continue"
        returns = lengths = None
        if rec.n_episodes:
            d = rec.download(("episode_return", "episode_length", "episode_flags"))
            full = (d["episode_flags"] & _lib.GS_EPISODE_PARTIAL) == 0
            returns, lengths = d["episode_return"][full], d["episode_length"][full]
        self.merge(rec.stats, returns, lengths, with_costs=costs)
        return rec

    def merge(self, stats, returns=None, lengths=None, with_costs: Optional[bool] = None) -> None:
        """Merge one rollout's statistics (an object with the fields of ``gs_episode_stats``); ``returns`` / ``lengths``: its
        complete episodes, for the window."""
        self.count_partial += int(stats.count_partial)
        nb = int(stats.count)
        if returns is not None:
            self.returns.extend(float(x) for x in returns); self.lengths.extend(int(x) for x in lengths)
        if nb == 0:
            return
        na, n = self.count, self.count + nb
        mb, m2b = float(stats.return_mean), float(stats.return_std) ** 2 * nb
        delta = mb - self._mean
        self._mean = self._mean + delta * (nb / n) if na else mb
        self._m2 = self._m2 + m2b + delta * delta * (na * nb / n) if na else m2b
        self.min_return = float(stats.return_min) if na == 0 else min(self.min_return, float(stats.return_min))
        self.max_return = float(stats.return_max) if na == 0 else max(self.max_return, float(stats.return_max))
        self._length_total += int(round(float(stats.length_mean) * nb))
        self.count = n
        self.n_success += int(stats.n_success)
        cost_mean = np.asarray(stats.cost_mean, dtype=np.float64)
        if with_costs is None:
            with_costs = not np.isnan(cost_mean).all()
        if with_costs:
            nc = self._cost_count + nb
            self._cost_mean = self._cost_mean + (cost_mean - self._cost_mean) * (nb / nc)
            self._cost_count = nc
            self.violating = self.violating + np.asarray(stats.violating, dtype=np.int64)

    mean_return = property(lambda self: self._mean if self.count else float("nan"))
    std_return = property(lambda self: float(np.sqrt(self._m2 / self.count)) if self.count else float("nan"))
    mean_length = property(lambda self: self._length_total / self.count if self.count else float("nan"))
    mean_cost = property(lambda self: self._cost_mean.copy() if self._cost_count else np.full(3, np.nan))
    success_rate = property(lambda self: self.n_success / self.count if self.count else float("nan"))
    window_mean_return = property(lambda self: float(np.mean(self.returns)) if self.returns else float("nan"))
    window_mean_length = property(lambda self: float(np.mean(self.lengths)) if self.lengths else float("nan"))


def evaluate_policy(env: BatchedGridEnvironment, policy, episodes_per_instance: int = 1, deterministic: bool = True, seed: int = 0,
                    limits: Optional[ConstraintLimits] = None, kinds="excess", success_return: float = -1000.0,
                    max_steps: Optional[int] = None, rollout_steps: Optional[int] = None) -> Dict[str, object]:
    """The reference's ``BenchmarkSuite._run_evaluation`` (benchmarking/benchmark_suite.py:360-429), batched and on the device:
    ``env.reset(seed=seed)``, then rollouts of ``rollout_steps`` steps (default: min(episode_length, 32)) under ``policy`` (an
    ``MLPPolicy``; ``stochastic = not deterministic``), rollout r with the noise seed ``seed + r``, each followed by ``rollout_costs``
    (where ``limits`` is given) and ``rollout_episodes``, until every instance has finished ``episodes_per_instance`` episodes.
    Only an instance's first ``episodes_per_instance`` episodes count, so instances with short episodes are not over-represented.
    Raises ``PowerFlowError`` where that would take more than ``max_steps`` steps per instance (default: ``episodes_per_instance *
    episode_length`` rounded up to whole rollouts -- no episode outlives the time limit).
    Returns the reference's keys: ``episode_returns`` (float64 [B * episodes_per_instance], rollout by rollout and within one by
    (instance, end step)), ``mean_return``, ``std_return`` (np.std), ``safety_violations`` (steps violating any channel, None
    without ``limits``), ``success_rate`` (no violating step -- vacuous without ``limits`` -- and return > ``success_return``),
    ``mean_cost`` (mean episodic cost per channel [3], None without ``limits``); plus ``episode_lengths``, ``episodes`` and ``steps``."""
    K, B = int(episodes_per_instance), env.num_envs
    if K < 1:
        raise ValueError("evaluate_policy: episodes_per_instance >= 1")
    floor = _success_floor(success_return)
    T = int(rollout_steps) if rollout_steps else max(1, min(env.episode_length, 32))
    if max_steps is None:
        max_steps = -(-K * env.episode_length // T) * T
    with_costs = limits is not None
    env.reset(seed=seed)
    env.set_policy(policy, stochastic=not deterministic)
    h = env.handle
    returns, lengths, costs, anyv = [], [], [], []
    steps, r = 0, 0
    while True:
        if steps + T > int(max_steps):
            raise PowerFlowError(f"evaluate_policy: not every instance finished {K} episode(s) within max_steps = {max_steps} steps")
        h.rollout(T, "mlp", seed=seed + r)
        if with_costs:
            h.rollout_costs(_lib.cost_config(limits, kinds))
        h.rollout_episodes(_lib.episode_config("fresh" if r == 0 else "continue", with_costs, floor))
        want = ["episode_return", "episode_length", "episode_ordinal", "ep_ordinal"] + (["episode_cost", "episode_any_violating"] if with_costs else [])
        d = h.rollout_episodes_download(want)
        keep = d["episode_ordinal"] < K
        returns.append(d["episode_return"][keep]); lengths.append(d["episode_length"][keep])
        if with_costs:
            costs.append(d["episode_cost"][:, keep]); anyv.append(d["episode_any_violating"][keep])
        steps += T; r += 1
        if int(d["ep_ordinal"].min()) >= K:
            break
    returns, lengths = np.concatenate(returns), np.concatenate(lengths)
    clean = np.concatenate(anyv) == 0 if with_costs else np.ones(len(returns), dtype=bool)
    return dict(episode_returns=returns, episode_lengths=lengths, mean_return=float(np.mean(returns)), std_return=float(np.std(returns)),
                safety_violations=int(np.concatenate(anyv).sum()) if with_costs else None,
                success_rate=float(np.sum(clean & (returns > floor)) / len(returns)),
                mean_cost=np.mean(np.concatenate(costs, axis=1), axis=1) if with_costs else None, episodes=int(len(returns)), steps=int(steps))


class GridDataset:
    """Transition store with the reference's normalisation (algorithms/base.py:207-224):
    observations / actions standardised per column with ``std + 1e-6``, rewards by their scalar
    mean / std; ``next_observations`` use the observation statistics."""

    def __init__(self, observations, actions, rewards, next_observations, terminals, normalize: bool = True) -> None:
        self.observations = np.asarray(observations, dtype=np.float64)
        self.actions = np.asarray(actions, dtype=np.float64)
        self.rewards = np.asarray(rewards, dtype=np.float64)
        self.next_observations = np.asarray(next_observations, dtype=np.float64)
        self.terminals = np.asarray(terminals)
        if normalize:
            self._normalize_data()
        self.size = len(self.observations)

    def _normalize_data(self) -> None:
        self.obs_mean = np.mean(self.observations, axis=0)
        self.obs_std = np.std(self.observations, axis=0) + 1e-6
        self.observations = (self.observations - self.obs_mean) / self.obs_std
        self.next_observations = (self.next_observations - self.obs_mean) / self.obs_std
        self.action_mean = np.mean(self.actions, axis=0)
        self.action_std = np.std(self.actions, axis=0) + 1e-6
        self.actions = (self.actions - self.action_mean) / self.action_std
        self.reward_mean = np.mean(self.rewards)
        self.reward_std = np.std(self.rewards) + 1e-6
        self.rewards = (self.rewards - self.reward_mean) / self.reward_std

    def sample_batch(self, batch_size: int, rng: Optional[np.random.Generator] = None) -> Dict[str, np.ndarray]:
        rng = rng or np.random.default_rng()
        idx = rng.integers(0, self.size, batch_size)
        return {"observations": self.observations[idx], "actions": self.actions[idx], "rewards": self.rewards[idx],
                "next_observations": self.next_observations[idx], "terminals": self.terminals[idx].astype(np.float64)}

    def get_all_data(self) -> Dict[str, np.ndarray]:
        return {"observations": self.observations, "actions": self.actions, "rewards": self.rewards,
                "next_observations": self.next_observations, "terminals": self.terminals.astype(np.float64)}

    def denormalize_action(self, action: np.ndarray) -> np.ndarray:
        return action * self.action_std + self.action_mean if hasattr(self, "action_mean") else action

    def denormalize_observation(self, obs: np.ndarray) -> np.ndarray:
        return obs * self.obs_std + self.obs_mean if hasattr(self, "obs_mean") else obs


_M32 = 0xFFFFFFFF


def _philox4x32(c0, c1, c2, c3, k0: int, k1: int):
    """Philox4x32-10 (Salmon et al. 2011) on uint64 arrays holding 32-bit words."""
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = ((p1 >> 32) ^ c1 ^ k0) & _M32, p1 & _M32, ((p0 >> 32) ^ c3 ^ k1) & _M32, p0 & _M32
        k0, k1 = (k0 + 0x9E3779B9) & _M32, (k1 + 0xBB67AE85) & _M32
    return c0, c1, c2, c3


class DeviceGridDataset:
    """``GridDataset`` over the environment's LAST rollout, on the device: the same attributes (``size``, ``obs_mean``, ``obs_std``,
    ``action_mean``, ``action_std``, ``reward_mean``, ``reward_std``; the standard deviations include the reference's + 1e-6) and the
    same ``sample_batch`` keys, the batches being ``DeviceArray`` views (``torch.as_tensor(b[k], device="cuda")``) of memory the handle
    owns, valid until the next ``sample_batch``.  The statistics come from a fixed reduction tree: a column that never varies has
    its value as mean and a raw standard deviation of exactly 0 (``constant_columns``), where ``np.std`` leaves ~1e-9 of noise.
    After a further rollout on the environment: ``rebuild()`` (new statistics) or ``rebuild(keep_stats=True)`` (same normalisation,
    new terminal map); until then sampling raises."""

    def __init__(self, env: BatchedGridEnvironment, normalize: bool = True) -> None:
        if not getattr(env.handle, "_rollout_T", 0):
            raise PowerFlowError("DeviceGridDataset: the environment holds no rollout (rollout_device / collect_random_data first)")
        self.env, self.normalize = env, bool(normalize)
        self._draw = 0
        self.rebuild()

    def rebuild(self, keep_stats: bool = False) -> None:
        """Build on the environment's last rollout.  ``keep_stats``: keep the normalisation (after a new rollout under a retrained
        policy), build only the terminal map."""
        h = self.env.handle
        h.dataset_build(keep_stats=keep_stats)
        st = h.dataset_stats()
        self.size, self.rows_per_chunk = st["n"], st["rows_per_chunk"]
        self.raw = st
        self.constant_columns = st["obs_std"] == 0.0
        self.obs_mean, self.obs_std = st["obs_mean"], st["obs_std"] + 1e-6
        self.action_mean, self.action_std = st["act_mean"], st["act_std"] + 1e-6
        self.reward_mean, self.reward_std = st["reward_mean"], st["reward_std"] + 1e-6

    @property
    def policy_obs_std(self) -> np.ndarray:
        """``obs_std`` with 1.0 on ``constant_columns``: what ``MLPPolicy.from_sequential(obs_std=)`` should divide by (a column
        that never varies carries no information; dividing it by 1e-6 only amplifies what a later rollout adds to it)."""
        return np.where(self.constant_columns, 1.0, self.obs_std)

    def set_stats(self, obs_mean, obs_std, action_mean, action_std, reward_mean, reward_std) -> None:
        """Install RAW statistics (standard deviations without the + 1e-6) in place of the computed ones."""
        self.env.handle.dataset_set_stats(obs_mean, obs_std, action_mean, action_std, reward_mean, reward_std)
        self.rebuild(keep_stats=True)

    @staticmethod
    def indices_np(seed: int, draw: int, n: int, N: int) -> np.ndarray:
        """The indices ``sample_batch(n, seed=seed)`` draws on the device in its call number ``draw`` (gs_dataset_sample): sample i =
        word i & 3 of Philox-4x32 keyed by ``seed`` with counter (i >> 2, draw low word, draw high word, 'SMPL'), index =
        (word * N) >> 32.  Pure NumPy, no device."""
        seed, draw, n, N = int(seed) & 0xFFFFFFFFFFFFFFFF, int(draw) & 0xFFFFFFFFFFFFFFFF, int(n), int(N)
        if not 0 < N < 2 ** 31:
            raise ValueError(f"indices_np: N = {N} outside (0, 2^31)")
        q = np.arange((n + 3) // 4, dtype=np.uint64)
        full = lambda v: np.full(q.shape, v, dtype=np.uint64)
        w = _philox4x32(q, full(draw & _M32), full(draw >> 32), full(0x534D504C), seed & _M32, seed >> 32)
        words = np.stack(w, axis=1).reshape(-1)[:n]
        return ((words * np.uint64(N)) >> np.uint64(32)).astype(np.int64)

    def sample_batch(self, batch_size: int, seed: int = 0, indices=None, dtype=np.float64, out=None, stream=None) -> Dict[str, object]:
        """One minibatch, gathered and normalised by one kernel.  Without ``indices`` they are drawn on the device with replacement
        (``indices_np(seed, k, batch_size, size)`` for the k-th such call on this dataset).  ``out``: the caller's device arrays
        (torch tensors) per key; ``stream``: the consumer's stream handle (None: the call returns when the batch is complete)."""
        draw = 0
        if indices is None:
            draw, self._draw = self._draw, self._draw + 1
        return self.env.handle.dataset_sample(batch_size, indices=indices, seed=seed, draw=draw, dtype=dtype, normalize=self.normalize,
                                              out=out, stream=stream)

    def denormalize_action(self, action):
        return action * self.action_std + self.action_mean if self.normalize else action

    def denormalize_observation(self, obs):
        return obs * self.obs_std + self.obs_mean if self.normalize else obs


# ---- on-policy minibatch epochs (include/gridstep.h "on-policy minibatch epochs") --------------------------------

def permutation_np(seed: int, epoch, N: int, positions=None) -> np.ndarray:
    """perm(seed, epoch) of [0, N) as ``gs_onpolicy_batch`` evaluates it per position (include/gridstep.h), int64 [N]: a four-round
    Feistel network over [0, 2^(2 h)), h the smallest integer >= 1 with 2^(2 h) >= N, its round function word 0 of Philox-4x32 keyed
    by ``seed`` with counter (R, round, epoch, 'PERM'); values that land at or above N walk on through the network until they come
    back below it.  ``positions``: only these positions of the permutation (it is stateless per position); ``epoch`` may be an
    array [E] of epochs, the result then being [E, positions].  Pure NumPy, no device."""
    seed, N = int(seed) & 0xFFFFFFFFFFFFFFFF, int(N)
    if not 0 < N < 2 ** 31:
        raise ValueError(f"permutation_np: N = {N} outside (0, 2^31)")
    pos = np.arange(N, dtype=np.int64) if positions is None else np.asarray(positions, dtype=np.int64).reshape(-1)
    if pos.size and (pos.min() < 0 or pos.max() >= N):
        raise ValueError(f"permutation_np: positions outside [0, {N})")
    ep = np.asarray(epoch, dtype=np.int64) & _M32
    shape = pos.shape if ep.ndim == 0 else (ep.size, pos.size)
    x = np.broadcast_to(pos.astype(np.uint64), shape).reshape(-1).copy()
    e = np.broadcast_to(ep.astype(np.uint64).reshape(-1, 1), (ep.size, pos.size)).reshape(-1)
    h = 1
    while (1 << (2 * h)) < N:
        h += 1
    mask, hb = np.uint64((1 << h) - 1), np.uint64(h)

    def one_pass(x, e):
        L, R = x >> hb, x & mask
        for rnd in range(4):
            w = _philox4x32(R, np.full(x.shape, rnd, dtype=np.uint64), e, np.full(x.shape, 0x5045524D, dtype=np.uint64), seed & _M32, seed >> 32)[0]
            L, R = R, L ^ (w & mask)
        return (L << hb) | R

    y = one_pass(x, e)
    while True:
        out = np.nonzero(y >= np.uint64(N))[0]
        if out.size == 0:
            return y.astype(np.int64).reshape(shape)
        y[out] = one_pass(y[out], e[out])


def onpolicy_batch_np(indices, observations, actions, log_probs, advantages, returns, values, cost_advantages=None, cost_returns=None,
                      lambdas=(0.0, 0.0, 0.0), adv_norm="rollout", adv_stats=None, adv_eps: float = 1e-8, dtype=np.float32, obs_shift=None,
                      obs_scale=None) -> Dict[str, object]:
    """The minibatch ``gs_onpolicy_batch`` leaves for the transitions ``indices`` (j = t * B + b), restated from downloaded arrays
    operation by operation: ``observations`` [N, obs_dim] (``obs_seq[:T]``), ``actions`` [N, A], ``log_probs`` (or None), ``advantages``,
    ``returns``, ``values`` [N] (``values[:T]``), ``cost_advantages`` / ``cost_returns`` sequences of three [N] arrays or None per
    channel.  ``adv_stats``: the (mean, raw std) the advantages are normalised with, as the device reported them -- the rollout's
    (``OnPolicyBatches.stats``) for "rollout", the batch's ``adv_stats`` for "minibatch"; unused for "none".  Everything is computed in
    float64 and rounded once to ``dtype``."""
    j = np.asarray(indices, dtype=np.int64)
    dt = np.dtype(dtype)
    flat = lambda a: np.asarray(a, dtype=np.float64).reshape(-1)
    cadv = [None] * 3 if cost_advantages is None else list(cost_advantages)
    cret = [None] * 3 if cost_returns is None else list(cost_returns)
    comb = flat(advantages)[j]
    for c in range(3):
        if float(lambdas[c]) != 0.0:
            comb = comb - float(lambdas[c]) * flat(cadv[c])[j]          # the product rounded, then the difference
    mode = _lib.ADV_NORM[adv_norm] if isinstance(adv_norm, str) else int(adv_norm)
    stats = np.array([np.nan, np.nan])
    if mode != 0:
        stats = np.asarray(adv_stats, dtype=np.float64).reshape(2)
        comb = (comb - stats[0]) / (stats[1] + float(adv_eps))
    obs = np.asarray(observations, dtype=np.float64)
    obs = obs.reshape(-1, obs.shape[-1])[j]
    if obs_shift is not None:
        obs = (obs - np.asarray(obs_shift, dtype=np.float64)) * np.asarray(obs_scale, dtype=np.float64)
    act = np.asarray(actions, dtype=np.float64)
    out = dict(observations=obs.astype(dt), actions=act.reshape(-1, act.shape[-1])[j].astype(dt),
               log_probs=None if log_probs is None else flat(log_probs)[j].astype(dt), advantages=comb.astype(dt),
               returns=flat(returns)[j].astype(dt), values=flat(values)[j].astype(dt),
               cost_advantages=[None if a is None else flat(a)[j].astype(dt) for a in cadv],
               cost_returns=[None if a is None else flat(a)[j].astype(dt) for a in cret],
               indices=j.astype(np.int32), adv_stats=stats)
    return out


class OnPolicyBatches:
    """Epochs of minibatches over the environment's LAST evaluated rollout, on the device (``gs_onpolicy_*``): every transition exactly
    once per epoch in the order of ``permutation_np(seed, epoch, N)``, each minibatch one gather that leaves what a clipped-surrogate
    step reads -- observations in the policy's normalisation, actions, old log-probabilities, the (Lagrangian) advantage normalised
    over the rollout or the minibatch, returns, values, cost advantages and returns -- in ``dtype``.

    ``policy``: an ``MLPPolicy`` (or ``MLPValue``) whose ``obs_mean`` and ``1 / obs_std`` normalise the observations, or give
    ``obs_mean`` / ``obs_std`` directly; neither: raw observations.  ``lambdas``: {channel name or index: multiplier}, the advantage
    becoming ``adv - sum_c lambda_c cost_adv_c``.  ``fields``: names of ``_lib.ONPOLICY_BATCH_FIELDS`` (None: all but the cost fields,
    which join when a multiplier is given).  ``prepare()`` after every ``evaluate_rollout`` / ``evaluate_rollout_costs``; then
    ``for batch in batches.epoch(e): ...`` yields dicts of zero-copy ``DeviceArray`` views valid until the next one."""

    def __init__(self, env, minibatch: int, policy=None, obs_mean=None, obs_std=None, lambdas=None, adv_norm: str = "rollout",
                 dtype=np.float32, fields=None, seed: int = 0, adv_eps: float = 1e-8) -> None:
        self.minibatch = int(minibatch)
        if self.minibatch <= 0:
            raise ValueError(f"OnPolicyBatches: minibatch = {minibatch} must be positive")
        if adv_norm not in _lib.ADV_NORM:
            raise ValueError(f"OnPolicyBatches: adv_norm {adv_norm!r}; one of {sorted(_lib.ADV_NORM)}")
        if policy is not None and (obs_mean is not None or obs_std is not None):
            raise ValueError("OnPolicyBatches: either a policy or obs_mean / obs_std")
        if policy is not None:
            obs_mean, obs_std = policy.obs_mean, policy.obs_std
        if (obs_mean is None) != (obs_std is None):
            raise ValueError("OnPolicyBatches: obs_mean and obs_std go together")
        self.obs_shift = None if obs_mean is None else np.array(obs_mean, dtype=np.float64).reshape(-1)
        self.obs_scale = None if obs_std is None else 1.0 / np.array(obs_std, dtype=np.float64).reshape(-1)
        self.lambdas = [0.0, 0.0, 0.0]
        self.set_lambdas(lambdas or {})
        if fields is None:
            fields = ["observations", "actions", "log_probs", "advantages", "returns", "values", "indices"]
            if any(x != 0.0 for x in self.lambdas):
                fields += ["cost_advantages", "cost_returns"]
        self.fields = _lib.onpolicy_fields(fields)
        self.env, self.adv_norm, self.dtype, self.seed, self.adv_eps = env, adv_norm, np.dtype(dtype), int(seed), float(adv_eps)
        self.size = 0

    def set_lambdas(self, lambdas) -> None:
        """New multipliers {channel name or index: value} (the others keep theirs); they count from the next ``prepare()``."""
        for name, value in dict(lambdas).items():
            if isinstance(name, str):
                if name not in _lib.COST_CHANNELS:
                    raise ValueError(f"OnPolicyBatches: unknown cost channel {name!r}; one of {_lib.COST_CHANNELS}")
                c = _lib.COST_CHANNELS.index(name)
            else:
                c = int(name)
                if not 0 <= c < 3:
                    raise ValueError(f"OnPolicyBatches: cost channel {c} outside 0 .. 2")
            self.lambdas[c] = float(value)

    def prepare(self, stream=None) -> None:
        """Combine and reduce the advantages of the environment's last rollout (``gs_onpolicy_prepare``, asynchronous).  ``stream``
        is accepted for symmetry with the evaluation calls: every batch is handed to its consumer's stream by ``epoch``."""
        h = self.env.handle
        h.onpolicy_prepare(self.adv_norm, self.dtype, self.fields, self.lambdas, self.adv_eps, self.obs_shift, self.obs_scale)
        self.size = int(getattr(h, "_rollout_T", 0)) * int(self.env.num_envs)

    def prepared(self, stream=None) -> "OnPolicyBatches":
        """``prepare()``, returning the object: ``for batch in OnPolicyBatches(env, 4096).prepared().epoch(0): ...``"""
        self.prepare(stream)
        return self

    @property
    def stats(self) -> SimpleNamespace:
        """``n``, ``adv_mean`` and the raw ``adv_std`` of the combined advantage over the rollout (host copies; waits for ``prepare``)."""
        return SimpleNamespace(**self.env.handle.onpolicy_stats())

    def __len__(self) -> int:
        return -(-self.size // self.minibatch)

    def bounds(self):
        """(first, n) of every minibatch of an epoch; the last one is ragged."""
        return [(k, min(self.minibatch, self.size - k)) for k in range(0, self.size, self.minibatch)]

    def epoch(self, e: int, out=None, stream=None):
        """The minibatches of epoch ``e``, in order.  ``out``: the caller's device arrays per key, used by every full-size batch (the
        ragged one goes to the handle's own buffers); ``stream``: the consumer's stream handle."""
        if self.size <= 0:
            raise PowerFlowError("OnPolicyBatches: prepare() first")
        for first, n in self.bounds():
            yield self.env.handle.onpolicy_batch(self.seed, e, first, n, out=out if n == self.minibatch else None, stream=stream)


# ---- recorded datasets as the handle's rollout (include/gridstep.h "a recorded dataset as the handle's rollout") ----

ROLLOUT_KEYS = ("observations", "actions", "rewards", "next_observations", "terminals")
_BREAK_CHUNK = 1 << 14      # rows the by-bits comparisons look at at a time


def _bits(x: np.ndarray) -> np.ndarray:
    """the array's elements as unsigned integers of their width: equality by bits (a NaN equals the same NaN, 0.0 is not -0.0)"""
    if x.dtype.itemsize not in (4, 8):
        raise PowerFlowError(f"observations are {x.dtype}; float64 or float32")
    return x.view(np.uint64 if x.dtype.itemsize == 8 else np.uint32)


def _rows_differ(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """[rows] bool: row i of ``a`` differs from row i of ``b`` by bits ([rows, D] each, C-contiguous views), looked at ``_BREAK_CHUNK``
    rows at a time so that no second copy of the observations is made"""
    out = np.empty(len(a), dtype=bool)
    for i in range(0, len(a), _BREAK_CHUNK):
        x, y = np.ascontiguousarray(a[i:i + _BREAK_CHUNK]), np.ascontiguousarray(b[i:i + _BREAK_CHUNK])
        out[i:i + _BREAK_CHUNK] = (_bits(x) != _bits(y)).any(axis=1)
    return out


def _flags(terminals) -> np.ndarray:
    t = np.asarray(terminals)
    return t.astype(np.uint8) if t.dtype == np.bool_ else t


def _as_tb(data: dict, B: int) -> dict:
    """``data`` as [T, B, ...] arrays: what ``Handle.rollout_download`` returns is passed through, the flat time-major dictionary of
    ``collect_random_data`` (transition index = t * B + b) is reshaped, not copied"""
    missing = [k for k in ROLLOUT_KEYS if k not in data]
    if missing:
        raise PowerFlowError(f"a rollout dictionary needs {missing}")
    out = {k: np.asarray(data[k]) for k in ROLLOUT_KEYS + ("final_observation", "log_probs") if data.get(k) is not None}
    if out["observations"].ndim == 2:
        N = len(out["observations"])
        if N % B:
            raise PowerFlowError(f"{N} time-major transitions are no whole number of steps of {B} instances")
        for k in ROLLOUT_KEYS + ("log_probs",):
            if k in out:
                out[k] = out[k].reshape((N // B, B) + out[k].shape[1:])
    out["terminals"] = _flags(out["terminals"])
    return out


def load_rollout_data(env: BatchedGridEnvironment, data: dict, chunk_rows: int = 0):
    """Installs a recorded dataset as the environment's rollout (``gs_rollout_load``, the inverse of ``Handle.rollout_download``):
    every entry that reads "the last rollout" -- ``DeviceGridDataset``, ``evaluate_rollout*``, ``rollout_costs``, ``rollout_episodes``,
    ``OnPolicyBatches``, ``DeviceLearner``, ``refresh_targets``, ``FederatedLearners`` -- then runs on it unchanged.  ``data``: the
    [T, B, ...] dictionary of ``Handle.rollout_download`` or the flat time-major one of ``collect_random_data`` (reshaped, not copied),
    float64 or float32; a bool ``terminals`` means "terminated" (bit 0); ``final_observation`` and ``log_probs`` are taken if present.
    A live transition's ``next_observations`` must equal, by bits, the ``observations`` one step later (``transitions_to_rollout``
    marks the breaks of a recorded trajectory).  The environment itself -- state, random chains, current observation -- is not
    touched, and need not have been reset.  Returns the ``gs_rollout_device`` view."""
    d = _as_tb(data, env.num_envs)
    env.handle.rollout_load(d["observations"], d.get("actions"), d["rewards"], d["next_observations"], d["terminals"],
                            final_observation=d.get("final_observation"), log_probs=d.get("log_probs"), chunk_rows=chunk_rows)
    return env.handle.rollout_device_view()


def transitions_to_rollout(data: dict, num_envs: int, timeouts=None) -> dict:
    """A recorded trajectory in the reference's flat form (``GridDataset``'s five arrays, transition i + 1 following transition i)
    as a [T, B, ...] rollout dictionary for ``load_rollout_data``: column b is transitions ``b * T .. (b + 1) * T - 1`` with
    ``T = N // num_envs``; the ``N - T * num_envs`` transitions at the end are dropped and reported as ``remainder``.  ``terminals``
    (bool or uint8) keeps its bits, ``timeouts`` [N] sets bit 1 (truncated).  A live transition whose ``next_observations`` differs
    by bits from the ``observations`` that follow it in its column -- the last one of a column included -- is a BREAK: the recording
    stopped there, which is a truncation, so it gets bit 1 and bootstraps under ``bootstrap=("truncated",)`` and under nothing else.
    ``breaks`` is their number."""
    B = int(num_envs)
    obs, nxt = np.asarray(data["observations"]), np.asarray(data["next_observations"])
    N = len(obs)
    T = N // B
    if B < 1 or T < 1:
        raise PowerFlowError(f"{N} transitions do not fill {B} columns")
    flags = _flags(data["terminals"]).astype(np.uint8).reshape(-1).copy()
    if timeouts is not None:
        flags[np.asarray(timeouts).reshape(-1) != 0] |= 2
    flags = flags[:T * B]
    # by bits, row i against row i + 1; a column's last row follows nothing
    differs = np.ones(T * B, dtype=bool)
    if T * B > 1:
        differs[:-1] = _rows_differ(nxt[:T * B - 1], obs[1:T * B])
    differs[T - 1::T] = True
    breaks = differs & (flags == 0)
    flags[breaks] |= 2
    tb = lambda x: np.swapaxes(np.asarray(x)[:T * B].reshape((B, T) + np.asarray(x).shape[1:]), 0, 1)
    out = {k: np.ascontiguousarray(tb(data[k])) for k in ("observations", "actions", "rewards", "next_observations")}
    out["terminals"] = np.ascontiguousarray(tb(flags))
    out["final_observation"] = np.ascontiguousarray(out["next_observations"][T - 1])
    out["remainder"], out["breaks"] = N - T * B, int(breaks.sum())
    return out


def rollout_to_transitions(data: dict) -> dict:
    """The inverse of ``transitions_to_rollout``'s layout: a [T, B, ...] rollout dictionary as flat arrays in which column b's
    transitions follow one another (index = b * T + t); ``terminals`` keeps its uint8 flags."""
    out = {}
    for k in ROLLOUT_KEYS:
        x = np.asarray(data[k])
        out[k] = np.ascontiguousarray(np.swapaxes(x, 0, 1)).reshape((x.shape[0] * x.shape[1],) + x.shape[2:])
    return out


def concat_rollouts(a: dict, b: dict) -> dict:
    """Two [T, B, ...] rollout dictionaries joined along T.  Legal exactly when ``a``'s ``final_observation`` equals ``b``'s
    ``observations[0]`` by bits -- two consecutive ``reset=False`` rollouts of one environment --, since ``b``'s first step then
    starts where ``a``'s last one ended; raises otherwise, naming the first instance that differs.  ``log_probs`` are kept when both
    have them."""
    fa, ob = a.get("final_observation"), np.asarray(b["observations"])
    if fa is None:
        raise PowerFlowError("concat_rollouts: the first rollout has no final_observation (rollout_download(want=(..., 'final_observation')))")
    fa = np.asarray(fa)
    if fa.shape != ob.shape[1:] or fa.dtype != ob.dtype:
        raise PowerFlowError(f"concat_rollouts: final_observation {fa.shape} {fa.dtype} against observations[0] {ob.shape[1:]} {ob.dtype}")
    differ = _rows_differ(fa, ob[0])
    if differ.any():
        raise PowerFlowError(f"concat_rollouts: the second rollout does not start where the first ended: instance {int(np.argmax(differ))} is the first of "
                             f"{int(differ.sum())} whose observations[0] differs from the first rollout's final_observation")
    out = {k: np.concatenate([np.asarray(a[k]), np.asarray(b[k])], axis=0) for k in ROLLOUT_KEYS}
    out["terminals"] = np.concatenate([_flags(a["terminals"]), _flags(b["terminals"])], axis=0)
    fb = b.get("final_observation")
    out["final_observation"] = np.asarray(b["next_observations"])[-1].copy() if fb is None else np.asarray(fb)
    if a.get("log_probs") is not None and b.get("log_probs") is not None:
        out["log_probs"] = np.concatenate([np.asarray(a["log_probs"]), np.asarray(b["log_probs"])], axis=0)
    return out


def download_rollout(env: BatchedGridEnvironment) -> dict:
    """The environment's last rollout as the [T, B, ...] dictionary ``load_rollout_data`` takes: the five arrays,
    ``final_observation``, and ``log_probs`` when the rollout recorded them."""
    h = env.handle
    d = h.rollout_download(want=ROLLOUT_KEYS + ("final_observation",))
    d.pop("n_terminal")
    try:
        d["log_probs"] = h.rollout_onpolicy_download(("log_probs",))["log_probs"]
    except PowerFlowError as e:          # (GS_E_STATE: the rollout recorded none)
        if f"libgridstep error {_lib.GS_E_STATE}:" not in str(e):
            raise
    return d


def save_rollout(env_or_data, path) -> None:
    """``np.savez`` of a rollout: the [T, B, ...] arrays plus ``final_observation``, and ``log_probs`` when recorded.  An environment:
    its last rollout (``download_rollout``); a dictionary: as it is."""
    d = env_or_data if isinstance(env_or_data, dict) else download_rollout(env_or_data)
    keep = {k: np.asarray(d[k]) for k in ROLLOUT_KEYS + ("final_observation", "log_probs") if d.get(k) is not None}
    keep["terminals"] = _flags(keep["terminals"])
    with open(path, "wb") as f:
        np.savez(f, **keep)


def load_rollout(env: BatchedGridEnvironment, path, chunk_rows: int = 0):
    """``load_rollout_data`` on what ``save_rollout`` wrote; returns the ``gs_rollout_device`` view."""
    with np.load(path) as z:
        return load_rollout_data(env, {k: z[k] for k in z.files}, chunk_rows=chunk_rows)


def continue_rollout(env: BatchedGridEnvironment, num_steps: int, keep: int, seed: int = 0, policy=None, stochastic: bool = False,
                     actions: Optional[np.ndarray] = None, t0: Optional[int] = None):
    """A sliding window on the device (``gs_rollout_continue``): the last ``keep`` steps of the environment's rollout stay, moved to
    the front, and ``num_steps`` new steps follow from where the environment stands; the rollout then has ``keep + num_steps`` steps and
    everything that reads "the last rollout" runs on that window.  ``policy`` / ``stochastic`` / ``actions`` ([num_steps, B, A], the new
    steps only) as ``rollout_device``; ``t0``: the step index the first new step draws with (None: where the last collection's draws
    ended, so that ``rollout_device(T1)`` then ``continue_rollout(T2, keep)`` with one seed holds the tail of ``rollout_device(T1 + T2)``
    by bits).  ``keep > 0`` needs a rollout that was collected here (not loaded) and an environment that was not moved since; the
    window is a new rollout to every track.  Returns the ``gs_rollout_device`` view."""
    if policy is not None and actions is not None:
        raise ValueError("continue_rollout: either actions or a policy")
    if env._needs_reset:
        env.reset(seed=seed)
    h = env.handle
    if policy is not None:
        if policy is not True:
            env.set_policy(policy, stochastic=stochastic)
        h.rollout_continue(int(num_steps), int(keep), "mlp", seed=seed, t0=t0)
    elif actions is None:
        h.rollout_continue(int(num_steps), int(keep), "random", seed=seed, t0=t0)
    else:
        h.rollout_continue(int(num_steps), int(keep), "uploaded", actions=np.asarray(actions, dtype=np.float64), t0=t0)
    return h.rollout_device_view()


def rollout_window_np(old: dict, new: dict, keep: int) -> dict:
    """What ``continue_rollout`` leaves, restated: the last ``keep`` steps of the [T, B, ...] rollout dictionary ``old`` joined with
    ``new`` (``concat_rollouts``: ``new`` must start where ``old`` ended).  Where both carry the device's terminal list
    (``terminal_index`` [n, 2] of (t, b), in any order, and ``terminal_obs`` [n, D]), the result has it too: ``old``'s entries with
    ``t >= T_old - keep`` in the order they lie in, renumbered ``t -= T_old - keep``, then ``new``'s with ``t += keep``."""
    T_old, keep = len(np.asarray(old["observations"])), int(keep)
    if not 0 <= keep <= T_old:
        raise PowerFlowError(f"rollout_window_np: keep = {keep} outside 0 .. {T_old}")
    drop = T_old - keep
    tail = {k: np.asarray(old[k])[drop:] for k in ROLLOUT_KEYS + ("log_probs",) if old.get(k) is not None}
    tail["final_observation"] = old.get("final_observation")
    out = concat_rollouts(tail, new)
    if all(d.get(k) is not None for d in (old, new) for k in ("terminal_index", "terminal_obs")):
        oi, ni = np.asarray(old["terminal_index"]).reshape(-1, 2), np.asarray(new["terminal_index"]).reshape(-1, 2)
        stay = oi[:, 0] >= drop
        out["terminal_index"] = np.concatenate([oi[stay] - np.array([drop, 0], dtype=oi.dtype), ni + np.array([keep, 0], dtype=ni.dtype)], axis=0)
        out["terminal_obs"] = np.concatenate([np.asarray(old["terminal_obs"])[stay], np.asarray(new["terminal_obs"])], axis=0)
    return out


class ReplayWindow:
    """The last ``capacity_steps`` steps of an environment's experience as its rollout, on the device: ``collect(num_steps)`` keeps
    ``min(capacity_steps - num_steps, current T)`` steps and appends ``num_steps`` fresh ones (``continue_rollout``), so the window
    fills up and then slides.  ``DeviceGridDataset``, ``OnPolicyBatches``, the learners and ``refresh_targets`` read it as the last
    rollout.  After the environment was moved between two collections (``reset``, ``step``, ``evaluate_policy``) the window cannot go
    on: ``collect(..., fresh=True)`` starts it again."""

    def __init__(self, env: BatchedGridEnvironment, capacity_steps: int) -> None:
        if int(capacity_steps) < 1:
            raise ValueError("ReplayWindow: capacity_steps < 1")
        self.env, self.capacity = env, int(capacity_steps)

    @property
    def steps(self) -> int:
        return 0 if self.env._needs_reset else self.env.handle.rollout_window_info()["T"]

    def collect(self, num_steps: int, seed: int = 0, policy=None, stochastic: bool = False, actions=None, fresh: bool = False):
        """``num_steps`` new steps behind what the window keeps; ``fresh``: keep nothing (after the environment was moved, or over
        a loaded rollout, which ``continue_rollout`` refuses to go on from).  Returns the ``gs_rollout_device`` view."""
        num_steps = int(num_steps)
        if not 0 < num_steps <= self.capacity:
            raise ValueError(f"ReplayWindow.collect: num_steps = {num_steps} outside 1 .. {self.capacity}")
        keep = 0 if fresh else min(self.capacity - num_steps, self.steps)
        return continue_rollout(self.env, num_steps, keep, seed=seed, policy=policy, stochastic=stochastic, actions=actions)
