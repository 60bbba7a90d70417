"""The learner on the device (``gs_learner_*``, include/gridstep.h): the networks that ``env.set_policy``,
``env.set_value`` and ``env.set_cost_value`` installed become trainable where they lie.  ``DeviceLearner.step(batch)`` runs, per
network, one clipped-surrogate (PPO) or critic update on a minibatch of ``OnPolicyBatches.epoch`` -- forward pass, loss, backward
pass, a deterministic gradient reduction and Adam, which also rewrites the image the rollout and critic kernels read: the next
``rollout_device(policy="mlp")`` acts with the updated policy and no weight crosses the host.

``ppo_grad_np``, ``value_grad_np`` and ``adam_np`` restate the arithmetic in NumPy -- what the kernels are tested against.
"""
from __future__ import annotations

import math
from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from .policy import HALF_LOG_2PI, LOG_STD_MAX, LOG_STD_MIN, MLPPolicy, MLPValue

HALF_LOG_2PIE = HALF_LOG_2PI + 0.5      # 0.5 * log(2 pi e): a unit Gaussian's entropy


def _activate(x: np.ndarray, kind: str) -> np.ndarray:
    zero = x.dtype.type(0)
    if kind == "relu":
        return np.maximum(x, zero)
    if kind == "tanh":
        return np.tanh(x)
    if kind == "elu":
        return np.where(x > zero, x, np.expm1(np.minimum(x, zero)))
    raise ValueError(f"activation must be one of {sorted(_lib.ACTIVATION)}, got {kind!r}")


def _act_grad(y: np.ndarray, kind: str) -> np.ndarray:
    """act'(x) from the saved output y = act(x), as the backward kernel takes it"""
    one, zero = y.dtype.type(1), y.dtype.type(0)
    if kind == "relu":
        return np.where(y > zero, one, zero)
    if kind == "tanh":
        return one - y * y
    return np.where(y > zero, one, y + one)


def _forward(layers, obs_n, activation: str, exact: bool):
    work = np.float64 if exact else np.float32
    rounded = [(np.asarray(w).astype(np.float32).astype(work), np.asarray(b).astype(np.float32).astype(work)) for w, b in layers]
    x = np.asarray(obs_n).astype(np.float32).astype(work)
    if x.ndim != 2 or x.shape[1] != rounded[0][0].shape[1]:
        raise ValueError(f"observations must be [n, {rounded[0][0].shape[1]}], got {x.shape}")
    acts = [x]
    for l, (w, b) in enumerate(rounded):
        x = x @ w.T + b
        if l < len(rounded) - 1:
            x = _activate(x, activation)
        acts.append(x)
    return rounded, acts


def _backward(rounded, acts, ghead, activation: str):
    """[(dW_l, db_l)] from the head gradient [n, last width] (the layers' dtype)"""
    grads: List[Tuple[np.ndarray, np.ndarray]] = [None] * len(rounded)      # type: ignore[list-item]
    delta = ghead
    for l in range(len(rounded) - 1, -1, -1):
        grads[l] = (delta.T @ acts[l], delta.sum(axis=0))
        if l:
            delta = (delta @ rounded[l][0]) * _act_grad(acts[l], activation)
    return grads


def ppo_grad_np(policy_layers, obs_n, actions, lp_old, adv, clip: float, ent_coef: float, exact: bool = False, clipped=None,
                activation: str = "relu") -> Dict[str, Any]:
    """The clipped-surrogate loss of include/gridstep.h and its gradient, as ``gs_learner_step`` computes them for the policy.
    ``policy_layers``: [(W [out, in], b [out])], the last of width 2 A (mean | log_std); ``obs_n`` [n, obs_dim] the NORMALISED
    observations (rounded to float32); ``actions`` [n, A] and ``lp_old`` [n] float64 as the rollout stored them; ``adv`` [n].
    Layers in float32 -- or, with ``exact``, the same float32-rounded operands in float64 throughout (what the float32 result is
    measured against, the ``pre_head_np`` pattern); the head in float64 either way, its gradient rounded once to float32 unless
    ``exact``.  ``clipped``: flags [n] to use in place of the ones this evaluation finds (a sample whose ratio lies at a rounding
    from 1 +- clip).  Returns ``grads`` [(dW, db)], ``log_probs_new``, ``ratio``, ``clipped``, ``surrogate_terms``,
    ``entropy_terms`` [n], ``log_std_outside`` [n, A] (the clamp is active), and the scalars ``loss``, ``surrogate``,
    ``entropy``, ``approx_kl``, ``clip_fraction``."""
    rounded, acts = _forward(policy_layers, obs_n, activation, exact)
    out = acts[-1].astype(np.float64)
    n, A = out.shape[0], out.shape[1] // 2
    a = np.asarray(actions, dtype=np.float64).reshape(n, A)
    lp_old = np.asarray(lp_old, dtype=np.float64).reshape(n)
    adv = np.asarray(adv).astype(np.float64).reshape(n)
    mean, lsr = out[:, :A], out[:, A:]
    inside = (lsr >= LOG_STD_MIN) & (lsr <= LOG_STD_MAX)
    ls = np.clip(lsr, LOG_STD_MIN, LOG_STD_MAX)
    lim = 1.0 - 1e-7
    x = np.arctanh(np.clip(a, -lim, lim))
    inv = np.exp(-ls)
    e = (x - mean) * inv
    terms = (((-0.5 * e) * e - ls) - HALF_LOG_2PI) - np.log((1.0 - a * a) + 1e-6)
    lp = terms[:, 0].copy()
    ent = ls[:, 0] + HALF_LOG_2PIE
    for k in range(1, A):
        lp += terms[:, k]
        ent += ls[:, k] + HALF_LOG_2PIE
    r = np.exp(lp - lp_old)
    lo, hi = 1.0 - clip, 1.0 + clip
    surr = np.minimum(r * adv, np.clip(r, lo, hi) * adv)
    found = ((adv > 0.0) & (r > hi)) | ((adv < 0.0) & (r < lo))
    flags = found if clipped is None else np.asarray(clipped).reshape(n).astype(bool)
    dlp = np.where(flags, 0.0, -((r * adv) / n))
    gmean = dlp[:, None] * (e * inv)
    gls = np.where(inside, dlp[:, None] * (e * e - 1.0) - ent_coef / n, 0.0)
    ghead = np.concatenate([gmean, gls], axis=1)
    ghead = ghead if exact else ghead.astype(np.float32)
    surrogate, entropy = math.fsum(surr) / n, math.fsum(ent) / n
    return dict(grads=_backward(rounded, acts, ghead, activation), log_probs_new=lp, ratio=r, clipped=found.astype(np.int32),
                surrogate_terms=surr, entropy_terms=ent, log_std_outside=~inside, loss=-surrogate - ent_coef * entropy,
                surrogate=surrogate, entropy=entropy, approx_kl=math.fsum(lp_old - lp) / n, clip_fraction=float(np.count_nonzero(found)) / n)


def value_grad_np(value_layers, obs_n, returns, exact: bool = False, activation: str = "relu") -> Dict[str, Any]:
    """The critic's loss ``mean (v - ret)^2`` and its gradient, as ``gs_learner_step`` computes them: ``value_layers`` with a last
    width of 1, ``obs_n`` [n, obs_dim] normalised, ``returns`` [n]; ``exact`` as for ``ppo_grad_np``.  Returns ``grads``
    [(dW, db)], ``values`` [n] (float64), ``loss_terms`` [n] and ``loss``."""
    rounded, acts = _forward(value_layers, obs_n, activation, exact)
    v = acts[-1].astype(np.float64)[:, 0]
    n = v.shape[0]
    d = v - np.asarray(returns).astype(np.float64).reshape(n)
    ghead = ((2.0 * d) / n)[:, None]
    ghead = ghead if exact else ghead.astype(np.float32)
    return dict(grads=_backward(rounded, acts, ghead, activation), values=v, loss_terms=d * d, loss=math.fsum(d * d) / n)


def adam_np(p, g, m, v, t: int, cfg, grad_norm: float):
    """One Adam step in float32, operation by operation as ``gs_k_train_adam`` performs it (include/gridstep.h states the order):
    ``p``, ``g``, ``m``, ``v`` arrays of one shape, ``t`` the step's number from 1, ``cfg`` a mapping or object with ``lr``,
    ``betas`` (or ``beta1`` / ``beta2``), ``eps``, ``weight_decay``, ``max_grad_norm``; ``grad_norm``: the norm of the WHOLE
    gradient (the device's figure), used when ``max_grad_norm`` > 0.  Returns the new (p, m, v)."""
    get = (lambda k, d=None: cfg.get(k, d)) if isinstance(cfg, dict) else (lambda k, d=None: getattr(cfg, k, d))
    betas = get("betas")
    b1, b2 = (float(betas[0]), float(betas[1])) if betas is not None else (float(get("beta1")), float(get("beta2")))
    lr, eps, wd, mx = float(get("lr")), float(get("eps")), float(get("weight_decay", 0.0)), float(get("max_grad_norm", 0.0))
    f = np.float32
    p, g, m, v = (np.asarray(x, dtype=f) for x in (p, g, m, v))
    if mx > 0.0:
        g = g * f(min(1.0, mx / (float(grad_norm) + 1e-6)))
    if f(wd) != 0.0:
        g = g + f(wd) * p
    m = f(b1) * m + f(1.0 - b1) * g
    v = f(b2) * v + (f(1.0 - b2) * g) * g
    denom = np.sqrt(v) / f(math.sqrt(1.0 - b2 ** t)) + f(eps)
    p = p - f(lr / (1.0 - b1 ** t)) * (m / denom)
    return p, m, v


def split_parameters(flat, dims: Sequence[int]) -> Tuple[List[np.ndarray], List[np.ndarray]]:
    """(W, b) lists from a flat array in torch order (W_0 row-major [out, in], b_0, W_1, ...) for the widths ``dims``."""
    flat = np.asarray(flat)
    if flat.shape != (sum(dims[l + 1] * (dims[l] + 1) for l in range(len(dims) - 1)),):
        raise ValueError(f"split_parameters: {flat.shape} values for the widths {list(dims)}")
    W, b, at = [], [], 0
    for l in range(len(dims) - 1):
        n_in, n_out = int(dims[l]), int(dims[l + 1])
        W.append(flat[at:at + n_out * n_in].reshape(n_out, n_in).copy()); at += n_out * n_in
        b.append(flat[at:at + n_out].copy()); at += n_out
    return W, b


class DeviceLearner:
    """Adam on the networks installed on ``env``'s device handle.  ``nets``: "policy" (a float32 Gaussian policy of
    ``env.set_policy``), "value" (``env.set_value``) and cost critics by channel name, as in ``env.set_cost_value``.  The
    hyper-parameters are torch's (``weight_decay``: L2 added to the gradient; ``max_grad_norm`` 0: no clipping); ``clip`` and
    ``ent_coef`` are the policy's.  Creating the learner snapshots each network's installed weights as float32 master parameters and
    zeroes Adam's state; installing a network again ends its learner (create a new ``DeviceLearner``).

    ``step(batch)``: one ``gs_learner_step`` per network on a dict of ``OnPolicyBatches.epoch`` (prepared with float32 and the
    networks' own observation normalisation).  After a step the ``MLPPolicy`` / ``MLPValue`` objects the networks were installed
    from no longer describe them: ``policy()`` / ``value(net)`` rebuild current ones from the device's parameters."""

    def __init__(self, env, nets: Sequence[str] = ("policy", "value"), lr: float = 3e-4, betas: Tuple[float, float] = (0.9, 0.999),
                 eps: float = 1e-8, weight_decay: float = 0.0, clip: float = 0.2, ent_coef: float = 0.0, max_grad_norm: float = 0.0) -> None:
        if isinstance(nets, str):
            nets = (nets,)
        self.nets = tuple(nets)
        if not self.nets:
            raise ValueError("DeviceLearner: no network named")
        self._ids = [_lib.learner_net(k) for k in self.nets]      # (ValueError for an unknown name)
        if len(set(self._ids)) != len(self._ids):
            raise ValueError(f"DeviceLearner: a network is named twice in {self.nets}")
        if len(betas) != 2:
            raise ValueError("DeviceLearner: betas = (beta1, beta2)")
        values = dict(lr=lr, beta1=betas[0], beta2=betas[1], eps=eps, weight_decay=weight_decay, clip=clip, max_grad_norm=max_grad_norm)
        for k, x in values.items():
            if not math.isfinite(float(x)) or float(x) < 0.0:
                raise ValueError(f"DeviceLearner: {k} = {x} must be finite and >= 0")
        if float(betas[0]) >= 1.0 or float(betas[1]) >= 1.0:
            raise ValueError(f"DeviceLearner: betas = {tuple(betas)} must lie in [0, 1)")
        if not math.isfinite(float(ent_coef)):
            raise ValueError(f"DeviceLearner: ent_coef = {ent_coef} must be finite")
        self.env = env
        self.config = dict(lr=float(lr), betas=(float(betas[0]), float(betas[1])), eps=float(eps), weight_decay=float(weight_decay),
                           clip=float(clip), ent_coef=float(ent_coef), max_grad_norm=float(max_grad_norm))
        cfg = _lib.learner_config(**self.config)
        for net in self._ids:
            env.handle.learner_create(net, cfg)

    def _id(self, net) -> int:
        k = _lib.learner_net(net)
        if k not in self._ids:
            raise ValueError(f"DeviceLearner: {net!r} is not one of this learner's networks {self.nets}")
        return k

    def step(self, batch: dict, stream=None) -> None:
        """One update of every network on ``batch`` (asynchronous on the handle's stream; ``stream``: a consumer's stream)."""
        n = int(batch["observations"].shape[0])
        for net in self._ids:
            self.env.handle.learner_step(net, batch, n, stream)

    def stats(self, net="policy") -> dict:
        """The last step's ``loss``, ``surrogate``, ``entropy``, ``approx_kl``, ``clip_fraction``, ``value_loss``, ``grad_norm`` and
        ``step`` (waits for the step; NaN where the network has no such figure)."""
        k = self._id(net)
        return self.env.handle.learner_stats(k)

    def info(self, net="policy") -> dict:
        k = self._id(net)
        return self.env.handle.learner_info(k)

    def download(self, net="policy", want=("params", "grads", "m", "v")) -> dict:
        """Flat float32 host copies, in torch order, of the master parameters, the last gradient and Adam's moments."""
        k = self._id(net)
        return self.env.handle.learner_download(k, want)

    def parameters(self, net="policy") -> Tuple[List[np.ndarray], List[np.ndarray]]:
        """The master parameters as float32 (W, b) lists, W [out, in] as torch's ``Linear.weight``."""
        k = self._id(net)
        return split_parameters(self.env.handle.learner_download(k, ("params",))["params"], self.env.handle.learner_info(k)["dims"])

    def gradients(self, net="policy") -> Tuple[List[np.ndarray], List[np.ndarray]]:
        """The last step's gradient (before clipping and weight decay) as float32 (dW, db) lists."""
        k = self._id(net)
        return split_parameters(self.env.handle.learner_download(k, ("grads",))["grads"], self.env.handle.learner_info(k)["dims"])

    def _meta(self, k: int) -> dict:
        key = "policy" if k == _lib.GS_LEARNER_POLICY else "value" if k == _lib.GS_LEARNER_VALUE else k - _lib.GS_LEARNER_COST_VALUE
        meta = self.env._installed_nets().get(key)
        if meta is None:
            raise _lib.PowerFlowError("DeviceLearner: the network was not installed through this environment (set_policy / set_value / set_cost_value)")
        return meta

    def policy(self) -> MLPPolicy:
        """A current ``MLPPolicy`` (float32, Gaussian head) from the device's parameters, with the normalisation the policy was
        installed with: for checkpoints, for ``set_policy`` on another environment, for loading into a torch module."""
        k = self._id("policy")
        meta = self._meta(k)
        W, b = self.parameters(k)
        return MLPPolicy(W, b, activation=self.env.handle.learner_info(k)["activation"], head="gaussian_tanh", obs_mean=meta["obs_mean"],
                         obs_std=meta["obs_std"], compute="float32")

    def value(self, net="value") -> MLPValue:
        """A current ``MLPValue`` of the reward critic or of a cost critic, as ``policy()``."""
        k = self._id(net)
        if k == _lib.GS_LEARNER_POLICY:
            raise ValueError("DeviceLearner.value: the policy is no critic (policy())")
        meta = self._meta(k)
        W, b = self.parameters(k)
        return MLPValue(W, b, activation=self.env.handle.learner_info(k)["activation"], obs_mean=meta["obs_mean"], obs_std=meta["obs_std"])

    def views(self, net="policy", stream=None) -> dict:
        """The last step's per-sample arrays as zero-copy ``DeviceArray`` views: ``log_probs_new``, ``ratio`` (float64), ``clipped``
        (int32), ``loss_terms`` and ``entropy_terms`` (float64) [n]; None where the network has none (a critic has ``loss_terms``)."""
        k = self._id(net)
        return self.env.handle.learner_view(k, stream)
