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
"""
from __future__ import annotations

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
