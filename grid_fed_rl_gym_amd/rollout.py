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
"""
from __future__ import annotations

from types import SimpleNamespace
from typing import Dict, Optional, Sequence

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
