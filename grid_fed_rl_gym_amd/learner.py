"""The learner on the device (``gs_learner_*``, include/gridstep.h): the networks that ``env.set_policy``,
``env.set_value`` and ``env.set_cost_value`` installed become trainable where they lie.  ``DeviceLearner.step(batch)`` runs, per
network, one clipped-surrogate (PPO) or critic update on a minibatch of ``OnPolicyBatches.epoch`` -- forward pass, loss, backward
pass, a deterministic gradient reduction and Adam, which also rewrites the image the rollout and critic kernels read: the next
``rollout_device(policy="mlp")`` acts with the updated policy and no weight crosses the host.

``ppo_grad_np``, ``value_grad_np``, ``awr_grad_np``, ``expectile_grad_np``, ``pathwise_grad_np`` (with ``pathwise_noise_np``), ``cql_grad_np`` (with ``cql_uniform_np`` and ``cql_noise_np``) and ``adam_np`` restate the arithmetic in NumPy -- what the kernels are tested against; ``anchor_term_np``, ``fisher_np`` and ``ewc_merge_np`` restate the parameter anchors.
"""
from __future__ import annotations

import math
from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from .policy import HALF_LOG_2PI, LOG_STD_MAX, LOG_STD_MIN, MLPPolicy, MLPQ, MLPValue
from .rollout import _bootstrap_mask, _philox4x32

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


def _backward(rounded, acts, ghead, activation: str, deltas: Optional[list] = None):
    """[(dW_l, db_l)] from the head gradient [n, last width] (the layers' dtype); ``deltas``: a list that receives delta_l [n, width
    of layer l] per layer, in layer order"""
    grads: List[Tuple[np.ndarray, np.ndarray]] = [None] * len(rounded)      # type: ignore[list-item]
    delta = ghead
    for l in range(len(rounded) - 1, -1, -1):
        grads[l] = (delta.T @ acts[l], delta.sum(axis=0))
        if deltas is not None:
            deltas.insert(0, delta)
        if l:
            delta = (delta @ rounded[l][0]) * _act_grad(acts[l], activation)
    return grads


def _with_backprop(result: Dict[str, Any], exact: bool, acts, deltas) -> Dict[str, Any]:
    """``exact`` results also carry ``backprop``: ``acts`` (a_0 = the input rows, then every layer's output) and ``deltas`` (dL / d
    pre-activation per layer) in float64 -- dW_l = delta_l^T a_l and db_l = the column sums of delta_l, term by term, for bounds on
    what rounding those terms can cost"""
    if exact:
        result["backprop"] = dict(acts=acts, deltas=deltas)
    result["passes"] = dict(acts=acts, deltas=deltas, exact=bool(exact))      # (in the evaluation's own precision: what ``fisher_np`` squares)
    return result


def _gaussian_head(out: np.ndarray, actions):
    """The Gaussian head of include/gridstep.h in float64 on the pre-head values ``out`` [n, 2 A] (mean | log_std) and the stored
    actions: ``inside`` [n, A] (the clamp of log_std is inactive), ``inv`` = exp(-ls), ``e``, and per sample the log-probability
    ``lp`` and the entropy ``ent``, summed in action order from k = 0."""
    n, A = out.shape[0], out.shape[1] // 2
    a = np.asarray(actions, dtype=np.float64).reshape(n, A)
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
    return inside, inv, e, lp, ent


def _head_grad(dlp: np.ndarray, inside, inv, e, ent_coef: float, n: int, exact: bool) -> np.ndarray:
    """dL / d(mean | log_std) [n, 2 A] from dL/dlp [n]: the clamp rule, - ent_coef / n, one rounding to float32 unless ``exact``"""
    gmean = dlp[:, None] * (e * inv)
    gls = np.where(inside, dlp[:, None] * (e * e - 1.0) - ent_coef / n, 0.0)
    ghead = np.concatenate([gmean, gls], axis=1)
    return ghead if exact else ghead.astype(np.float32)


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
    n = out.shape[0]
    inside, inv, e, lp, ent = _gaussian_head(out, actions)
    lp_old = np.asarray(lp_old, dtype=np.float64).reshape(n)
    adv = np.asarray(adv).astype(np.float64).reshape(n)
    r = np.exp(lp - lp_old)
    lo, hi = 1.0 - clip, 1.0 + clip
    surr = np.minimum(r * adv, np.clip(r, lo, hi) * adv)
    found = ((adv > 0.0) & (r > hi)) | ((adv < 0.0) & (r < lo))
    flags = found if clipped is None else np.asarray(clipped).reshape(n).astype(bool)
    dlp = np.where(flags, 0.0, -((r * adv) / n))
    ghead = _head_grad(dlp, inside, inv, e, ent_coef, n, exact)
    surrogate, entropy = math.fsum(surr) / n, math.fsum(ent) / n
    deltas: list = []
    out = dict(grads=_backward(rounded, acts, ghead, activation, deltas), log_probs_new=lp, ratio=r, clipped=found.astype(np.int32),
               surrogate_terms=surr, entropy_terms=ent, log_std_outside=~inside, loss=-surrogate - ent_coef * entropy,
               surrogate=surrogate, entropy=entropy, approx_kl=math.fsum(lp_old - lp) / n, clip_fraction=float(np.count_nonzero(found)) / n)
    return _with_backprop(out, exact, acts, deltas)


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
    deltas: list = []
    out = dict(grads=_backward(rounded, acts, ghead, activation, deltas), values=v, loss_terms=d * d, loss=math.fsum(d * d) / n)
    return _with_backprop(out, exact, acts, deltas)


def awr_grad_np(policy_layers, obs_n, actions, adv, temperature: float, weight_max: float, ent_coef: float, exact: bool = False,
                capped=None, activation: str = "relu", lp_old=None) -> Dict[str, Any]:
    """The advantage-weighted log-likelihood of include/gridstep.h ("the learner's loss") and its gradient, as ``gs_learner_step``
    computes them under GS_LOSS_AWR: ``w = fmin(exp(adv / temperature), weight_max)`` times the log-probability of the STORED
    action; both may be ``inf`` (unit weights, no cap: behaviour cloning).  Arguments as ``ppo_grad_np``; ``capped``: flags [n] to
    use in place of the ones this evaluation finds (a sample whose weight lies at a rounding from ``weight_max``: a flagged sample
    takes ``weight_max`` in the gradient, an unflagged one ``exp(adv / temperature)``); ``lp_old`` [n]: the rollout's
    log-probabilities where it recorded any, for ``approx_kl`` alone.  Returns ``grads`` [(dW, db)], ``log_probs_new``, ``weights``,
    ``capped``, ``loss_terms`` (w lp), ``entropy_terms`` [n], ``log_std_outside`` [n, A] and the scalars ``loss``, ``surrogate``,
    ``entropy``, ``approx_kl`` (NaN without ``lp_old``) and ``clip_fraction`` (the capped share)."""
    temperature, weight_max = _awr_check(temperature, weight_max)
    rounded, acts = _forward(policy_layers, obs_n, activation, exact)
    out = acts[-1].astype(np.float64)
    n = out.shape[0]
    inside, inv, e, lp, ent = _gaussian_head(out, actions)
    adv = np.asarray(adv).astype(np.float64).reshape(n)
    with np.errstate(over="ignore"):
        u = np.exp(adv / temperature)
    w = np.fmin(u, weight_max)
    found = u > weight_max
    w_grad = w if capped is None else np.where(np.asarray(capped).reshape(n).astype(bool), weight_max, u)
    dlp = -(w_grad / n)
    ghead = _head_grad(dlp, inside, inv, e, ent_coef, n, exact)
    terms = w * lp
    surrogate, entropy = math.fsum(terms) / n, math.fsum(ent) / n
    kl = float("nan") if lp_old is None else math.fsum(np.asarray(lp_old, dtype=np.float64).reshape(n) - lp) / n
    deltas: list = []
    out = dict(grads=_backward(rounded, acts, ghead, activation, deltas), log_probs_new=lp, weights=w, capped=found.astype(np.int32),
               loss_terms=terms, entropy_terms=ent, log_std_outside=~inside, loss=-surrogate - ent_coef * entropy,
               surrogate=surrogate, entropy=entropy, approx_kl=kl, clip_fraction=float(np.count_nonzero(found)) / n)
    return _with_backprop(out, exact, acts, deltas)


def expectile_grad_np(value_layers, obs_n, returns, expectile: float, exact: bool = False, activation: str = "relu") -> Dict[str, Any]:
    """The expectile regression ``mean q (v - ret)^2``, ``q = expectile`` where ``v < ret`` and ``1 - expectile`` elsewhere, and its
    gradient, as ``gs_learner_step`` computes them under GS_LOSS_EXPECTILE; arguments and results as ``value_grad_np``, plus
    ``below`` [n] (``v < ret``).  At 0.5 the head gradient is exactly half of ``value_grad_np``'s."""
    tau = _expectile_check(expectile)
    rounded, acts = _forward(value_layers, obs_n, activation, exact)
    v = acts[-1].astype(np.float64)[:, 0]
    n = v.shape[0]
    d = v - np.asarray(returns).astype(np.float64).reshape(n)
    q = np.where(d < 0.0, tau, 1.0 - tau)
    ghead = (q * ((2.0 * d) / n))[:, None]
    ghead = ghead if exact else ghead.astype(np.float32)
    terms = q * (d * d)
    deltas: list = []
    out = dict(grads=_backward(rounded, acts, ghead, activation, deltas), values=v, below=d < 0.0, loss_terms=terms, loss=math.fsum(terms) / n)
    return _with_backprop(out, exact, acts, deltas)


def pathwise_noise_np(seed: int, draw: int, n: int, A: int, tag: int = _lib.PATHWISE_NOISE_TAG) -> np.ndarray:
    """eps [n, A] of a pathwise actor step: ``eps[i, k]`` = component ``k & 3`` of the four normals of Philox4x32-10 with counter
    (i, k >> 2, draw, 'PWNO') and key ``seed`` -- ``fed_noise_np``'s recipe (every word w a uniform (w + 1/2) 2^-32, words (0, 1)
    and (2, 3) one Box-Muller pair each, cosine then sine) under the actor step's counter.  ``tag``: the counter's fourth word, for
    the steps that share the sampling head under a tag of their own (``cql_noise_np``)."""
    n, A = int(n), int(A)
    if n < 0 or A <= 0:
        raise ValueError(f"pathwise_noise_np: n = {n} must be >= 0 and A = {A} > 0")
    quads = (A + 3) // 4
    i = np.repeat(np.arange(n, dtype=np.uint64), quads)
    q = np.tile(np.arange(quads, dtype=np.uint64), n)
    full = lambda x: np.full(i.shape, int(x) & 0xFFFFFFFF, dtype=np.uint64)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    w = np.stack(_philox4x32(i, q, full(draw), full(tag), seed & 0xFFFFFFFF, seed >> 32), axis=1).astype(np.float64)
    u = (w + 0.5) * (1.0 / 4294967296.0)
    ra, rb = np.sqrt(-2.0 * np.log(u[:, 0])), np.sqrt(-2.0 * np.log(u[:, 2]))
    ta, tb = 2.0 * math.pi * u[:, 1], 2.0 * math.pi * u[:, 3]
    z = np.stack([ra * np.cos(ta), ra * np.sin(ta), rb * np.cos(tb), rb * np.sin(tb)], axis=1)
    return z.reshape(n, 4 * quads)[:, :A].copy()


# exp, tanh and log of the pathwise heads, operation by operation as the kernels perform them (gw_exp, gw_tanh, gw_log of csrc/gw_math.h): rounded
# float64 +, -, *, / alone, so that the heads are restated to the bit whatever math library NumPy was built on
_PW_LN2_HI, _PW_LN2_LO, _PW_INV_LN2 = 6.93147180369123816490e-01, 1.90821492927058770002e-10, 1.4426950408889634
_PW_HALF_LOG_2PI = 0.91893853320467274178      # the kernels' literal: 0.5 log(2 pi) rounded to nearest, one ulp above policy.HALF_LOG_2PI
_PW_INV_FACT = [1.0 / math.factorial(j) for j in range(24)]
_PW_INV_ODD = [1.0 / (2 * j + 1) for j in range(1, 16)]


def pathwise_exp_np(x) -> np.ndarray:
    """exp as the pathwise heads compute it: k = rint(x / ln 2), r = x - k ln 2 in two parts, the Taylor sum to r^17 by Horner's
    rule, times 2^k."""
    x = np.asarray(x, dtype=np.float64)
    k = np.rint(x * _PW_INV_LN2)
    r = (x - k * _PW_LN2_HI) - k * _PW_LN2_LO
    p = np.full(x.shape, _PW_INV_FACT[17])
    for j in range(16, -1, -1):
        p = _PW_INV_FACT[j] + r * p
    return np.ldexp(p, k.astype(np.int64))


def pathwise_tanh_np(x) -> np.ndarray:
    """tanh as the pathwise heads compute it, u = min(|x|, 40): below 0.5 from m = expm1(2 u) (the Taylor sum to (2 u)^23) as
    m / (m + 2), else from e = exp(-2 u) as (1 - e) / (1 + e); the sign of x."""
    x = np.asarray(x, dtype=np.float64)
    u = np.fmin(np.abs(x), 40.0)
    y = 2.0 * np.where(u < 0.5, u, 0.0)
    p = np.full(x.shape, _PW_INV_FACT[23])
    for j in range(22, 0, -1):
        p = _PW_INV_FACT[j] + y * p
    m = y * p
    e = pathwise_exp_np(-2.0 * u)
    return np.copysign(np.where(u < 0.5, m / (m + 2.0), (1.0 - e) / (1.0 + e)), x)


def pathwise_log_np(v) -> np.ndarray:
    """log of positive normal numbers as the pathwise heads compute it: v = m 2^e with sqrt(1/2) <= m < sqrt(2), s = (m - 1) / (m + 1),
    log m = 2 s (1 + z P(z)) with z = s s and P the sum of z^(j - 1) / (2 j + 1), j = 1 .. 15; plus e ln 2 in two parts."""
    v = np.asarray(v, dtype=np.float64)
    m, e = np.frexp(v)
    small = m < 0.7071067811865476
    m = np.where(small, m * 2.0, m)
    ed = (e - small).astype(np.float64)
    f = m - 1.0
    s = f / (2.0 + f)
    z = s * s
    p = np.full(v.shape, _PW_INV_ODD[14])
    for j in range(13, -1, -1):
        p = _PW_INV_ODD[j] + z * p
    t2 = 2.0 * s
    logm = t2 + t2 * (z * p)
    return ed * _PW_LN2_HI + (ed * _PW_LN2_LO + logm)


def _pathwise_sample(out: np.ndarray, eps):
    """The sampling head of include/gridstep.h ("the pathwise actor step") in float64 on the pre-head values ``out`` [n, 2 A] (mean |
    log_std) and the noise ``eps`` [n, A]: ``inside`` [n, A] (the clamp of log_std is inactive), ``std``, the actions ``a`` =
    tanh(mean + std eps), and per sample the log-probability ``lp``, summed in action order from k = 0."""
    n, A = out.shape[0], out.shape[1] // 2
    eps = np.asarray(eps, dtype=np.float64).reshape(n, A)
    mean, lsr = out[:, :A], out[:, A:]
    inside = (lsr >= LOG_STD_MIN) & (lsr <= LOG_STD_MAX)
    ls = np.clip(lsr, LOG_STD_MIN, LOG_STD_MAX)
    std = pathwise_exp_np(ls)
    a = pathwise_tanh_np(mean + std * eps)
    terms = (((-0.5 * eps) * eps - ls) - _PW_HALF_LOG_2PI) - pathwise_log_np((1.0 - a * a) + 1e-6)
    lp = terms[:, 0].copy()
    for k in range(1, A):
        lp += terms[:, k]
    return inside, std, eps, a, lp


def _pathwise_head(inside, std, eps, a, lp, q, dq_da, alpha: float, bc_coef: float, stored, exact: bool, which=None):
    """The actor head of include/gridstep.h in float64: the smaller twin (``which``: choices to use in place of the ones found),
    the loss terms, and dL / d(mean | log_std) [n, 2 A], rounded once to float32 unless ``exact``."""
    n, A = a.shape
    if len(q) == 1:
        found = np.zeros(n, dtype=np.int32)
    else:
        found = np.where(q[0] <= q[1], 0, 1).astype(np.int32)
    use = found if which is None else np.asarray(which).reshape(n).astype(np.int32)
    if use.size and (use.min() < 0 or use.max() >= len(q)):
        raise ValueError(f"pathwise_grad_np: which must name one of the {len(q)} twin(s)")
    rows = np.arange(n)
    qs, ds = np.stack(q, axis=0), np.stack(dq_da, axis=0)
    qmin = qs[use, rows]
    dq = ds[use, rows].astype(np.float64)
    if bc_coef != 0.0:
        d = a - np.asarray(stored, dtype=np.float64).reshape(n, A)
    else:
        d = np.zeros_like(a)
    sq = d * d
    bc = sq[:, 0].copy()
    for k in range(1, A):
        bc += sq[:, k]
    terms = (alpha * lp - qmin) + bc_coef * bc
    om = 1.0 - a * a
    t1 = (alpha * (2.0 * a)) / (om + 1e-6)
    t2 = (2.0 * bc_coef) * d
    G = (((t1 - dq) + t2) * om) / n
    gls = np.where(inside, (G * std) * eps - alpha / n, 0.0)
    ghead = np.concatenate([G, gls], axis=1)
    return found, use, qmin, bc, terms, (ghead if exact else ghead.astype(np.float32))


def pathwise_grad_np(policy_layers, q_layers_list, obs_n, eps, alpha: float, bc_coef: float, stored_actions=None, exact: bool = False,
                     which=None, activation: str = "relu", q_activation: str = "relu") -> Dict[str, Any]:
    """The pathwise actor loss of include/gridstep.h ("the pathwise actor step") and its gradient with respect to the POLICY, as
    ``gs_learner_step_pathwise`` computes them: ``L = mean(alpha lp - min_w Q_w(s, a) + bc_coef |a - a_stored|^2)`` with
    ``a = tanh(mean + std eps)`` and the gradient flowing through the twins into the policy.  ``policy_layers`` as for
    ``ppo_grad_np``; ``q_layers_list``: one or two Q networks' [(W, b)] over [obs | action] (the last width 1), used read-only;
    ``obs_n`` [n, obs_dim] the NORMALISED observations; ``eps`` [n, A] the noise (zeros: the deterministic actor);
    ``stored_actions`` [n, A] float64, needed when ``bc_coef`` != 0.  Layers in float32 -- or, with ``exact``, the same
    float32-rounded operands in float64 throughout --, the heads in float64, head gradients rounded once to float32 unless
    ``exact``; the action enters a twin rounded to float32 either way.  ``which`` [n]: the twin to take per sample in place of
    the smaller one this evaluation finds (a sample whose two values lie at a rounding from each other).  Returns ``grads``
    [(dW, db)] of the policy, ``actions`` [n, A], ``log_probs`` [n], ``q`` [twins, n] (float64), ``q_min`` [n], ``which`` [n]
    (found here), ``dq_da`` [twins, n, A], ``bc_terms``, ``loss_terms`` [n], ``log_std_outside`` [n, A] and the scalars ``loss``,
    ``surrogate`` (mean q_min) and ``entropy`` (-mean lp)."""
    alpha, bc_coef = _pathwise_check(alpha, bc_coef)
    q_layers_list = list(q_layers_list)
    if not 1 <= len(q_layers_list) <= 2:
        raise ValueError(f"pathwise_grad_np: one or two Q networks, got {len(q_layers_list)}")
    rounded, acts = _forward(policy_layers, obs_n, activation, exact)
    out = acts[-1].astype(np.float64)
    n, A = out.shape[0], out.shape[1] // 2
    if out.shape[1] != 2 * A or A == 0:
        raise ValueError(f"pathwise_grad_np: the policy's last width {out.shape[1]} must be 2 A (mean | log_std)")
    eps = np.asarray(eps, dtype=np.float64)
    if eps.shape != (n, A):
        raise ValueError(f"pathwise_grad_np: eps must be [{n}, {A}], got {eps.shape}")
    if bc_coef != 0.0 and (stored_actions is None or np.shape(stored_actions) != (n, A)):
        raise ValueError(f"pathwise_grad_np: bc_coef != 0 needs stored_actions [{n}, {A}]")
    inside, std, eps, a, lp = _pathwise_sample(out, eps)
    work = np.float64 if exact else np.float32
    D = acts[0].shape[1]
    sa = np.concatenate([acts[0], a.astype(np.float32).astype(work)], axis=1)
    qv, dq = [], []
    for layers in q_layers_list:
        if np.asarray(layers[0][0]).shape[1] != D + A or np.asarray(layers[-1][0]).shape[0] != 1:
            raise ValueError(f"pathwise_grad_np: a Q network maps {D + A} columns to 1")
        qr, qa = _forward(layers, sa, q_activation, exact)
        delta = np.ones((n, 1), dtype=work)
        for l in range(len(qr) - 1, 0, -1):
            delta = (delta @ qr[l][0]) * _act_grad(qa[l], q_activation)
        qv.append(qa[-1].astype(np.float64)[:, 0])
        dq.append(delta @ qr[0][0][:, D:])
    found, use, qmin, bc, terms, ghead = _pathwise_head(inside, std, eps, a, lp, qv, dq, alpha, bc_coef, stored_actions, exact, which)
    ghead = ghead.astype(work) if exact else ghead
    deltas: list = []
    res = dict(grads=_backward(rounded, acts, ghead, activation, deltas), actions=a, log_probs=lp, q=np.stack(qv, axis=0), q_min=qmin, which=found,
               dq_da=np.stack(dq, axis=0), bc_terms=bc, loss_terms=terms, log_std_outside=~inside, loss=math.fsum(terms) / n,
               surrogate=math.fsum(qmin) / n, entropy=-(math.fsum(lp) / n))
    return _with_backprop(res, exact, acts, deltas)


def cql_noise_np(seed: int, draw: int, n: int, A: int) -> np.ndarray:
    """eps [n, A] of a conservative critic step's policy candidates: ``pathwise_noise_np`` under the tag 'CQLN', so that a pathwise
    step with the same seed and draw does not reuse the numbers."""
    return pathwise_noise_np(seed, draw, n, A, tag=_lib.CQL_NOISE_TAG)


def cql_uniform_np(seed: int, draw: int, n: int, A: int) -> np.ndarray:
    """The uniform candidate actions [n, A] (float64) of a conservative critic step: ``u[i, k] = (word + 0.5) 2^-31 - 1`` with
    ``word`` = word ``k & 3`` of Philox4x32-10 with counter (i, k >> 2, draw, 'CQLU') and key ``seed``; every operation is exact in
    float64, and the values lie strictly inside (-1, 1).  The twin reads them rounded to float32."""
    n, A = int(n), int(A)
    if n < 0 or A <= 0:
        raise ValueError(f"cql_uniform_np: n = {n} must be >= 0 and A = {A} > 0")
    quads = (A + 3) // 4
    i = np.repeat(np.arange(n, dtype=np.uint64), quads)
    q = np.tile(np.arange(quads, dtype=np.uint64), n)
    full = lambda x: np.full(i.shape, int(x) & 0xFFFFFFFF, dtype=np.uint64)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    w = np.stack(_philox4x32(i, q, full(draw), full(_lib.CQL_UNIFORM_TAG), seed & 0xFFFFFFFF, seed >> 32), axis=1).astype(np.float64)
    u = (w + 0.5) * (1.0 / 2147483648.0) - 1.0
    return u.reshape(n, 4 * quads)[:, :A].copy()


_STAT_THREADS = 1024      # GS_TR_STAT_THREADS


def _block_sum_np(x) -> float:
    """The sum of ``x`` in the order of the one-workgroup statistics kernels (gs_k_train_stats, gs_k_cql_lse): thread t adds entries
    t, t + 1024, ... ascending from 0.0, then the balanced tree of csrc/block_reduce.h over the 1024 threads (partners at 32, 16,
    ..., 1 lanes within a wavefront of 64, then at 8, 4, 2, 1 over the 16 wavefronts)."""
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    pad = (-x.size) % _STAT_THREADS
    rows = np.concatenate([x, np.zeros(pad)]).reshape(-1, _STAT_THREADS)
    v = np.zeros(_STAT_THREADS)
    for r in rows:
        v = v + r      # (a thread whose entry lies beyond the end adds nothing; + 0.0 leaves a sum that began at 0.0 as it is)
    v = v.reshape(_STAT_THREADS // 64, 64)
    lane = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        v = v + v[:, lane ^ off]
    w = v[:, 0]
    wave = np.arange(w.size)
    for off in (8, 4, 2, 1):
        w = w + w[wave ^ off]
    return float(w[0])


def _cql_weight_check(conservative_weight) -> float:
    cw = float(conservative_weight)
    if not math.isfinite(cw) or cw < 0.0:
        raise ValueError(f"conservative_weight = {cw} must be finite and >= 0")
    return cw


CQL_EXP_FLOOR = -700.0      # GS_CQL_EXP_FLOOR: what lies this far below the maximum adds nothing to the logsumexp


def cql_grad_np(q_layers, obs_n, data_actions, random_actions, policy_actions, targets, conservative_weight: float, exact: bool = False,
                activation: str = "relu", q=None, scalars=None) -> Dict[str, Any]:
    """The conservative critic loss of include/gridstep.h ("the conservative critic step") of ONE twin and its gradient, as
    ``gs_learner_step_conservative`` computes them: ``mse(Q(s, a_data), y) + conservative_weight (logsumexp_j q_j - mean Q(s,
    a_data))`` with j over all 3 n values ``Q(s, a_data) | Q(s, a_random) | Q(s, a_policy)`` -- the logsumexp runs over the batch,
    as the reference's.  ``q_layers``: [(W, b)] over [obs | action], the last width 1; ``obs_n`` [n, obs_dim] the NORMALISED
    observations; the three action arrays [n, A] (constants of the step; they enter the twin rounded to float32); ``targets`` [n].
    Layers in float32 -- or, with ``exact``, the same float32-rounded operands in float64 throughout, with the library's exp and
    log and exactly rounded sums --, the head in float64, its gradient rounded once to float32 unless ``exact``.  ``q`` [3 n]: values
    to run the head on in place of this evaluation's (the device's float32 values, widened); ``scalars``: (m, S, ...) to take the
    maximum and the sum of exponentials from (the device's), as ``pre_head=`` in ``policy_rows_np``.  Returns what ``value_grad_np``
    returns -- ``grads`` [(dW, db)], ``values`` [n], ``loss_terms`` [n] ((q_i - y_i)^2), ``loss`` (value_loss + conservative_weight
    penalty) -- plus ``value_loss``, ``q`` [3 n], ``weights`` [3 n] (the softmax over the batch), ``penalty`` and ``scalars`` [4]
    (m, S, lse, qbar)."""
    cw = _cql_weight_check(conservative_weight)
    work = np.float64 if exact else np.float32
    obs = np.asarray(obs_n).astype(np.float32)
    n = obs.shape[0]
    blocks = []
    for name, a in (("data_actions", data_actions), ("random_actions", random_actions), ("policy_actions", policy_actions)):
        a = np.asarray(a)
        if a.ndim != 2 or a.shape[0] != n:
            raise ValueError(f"cql_grad_np: {name} must be [{n}, A], got {a.shape}")
        blocks.append(np.concatenate([obs, a.astype(np.float32)], axis=1))
    if n == 0 or np.asarray(q_layers[-1][0]).shape[0] != 1:
        raise ValueError("cql_grad_np: at least one row, and a Q network whose last width is 1")
    rounded, acts = _forward(q_layers, np.concatenate(blocks, axis=0), activation, exact)
    qv = acts[-1].astype(np.float64)[:, 0]
    if q is not None:
        qv = np.asarray(q, dtype=np.float64).reshape(3 * n)
    y = np.asarray(targets).astype(np.float64).reshape(n)
    m = float(np.max(qv)) if scalars is None else float(scalars[0])
    d = qv - m
    inside = d >= CQL_EXP_FLOOR
    e = np.where(inside, np.exp(np.where(inside, d, 0.0)) if exact else pathwise_exp_np(np.where(inside, d, 0.0)), 0.0)
    if scalars is not None:
        S = float(scalars[1])
    else:
        S = math.fsum(e) if exact else _block_sum_np(e)
    lse = m + (math.log(S) if exact else float(pathwise_log_np(np.float64(S))))
    qbar = (math.fsum(qv[:n]) if exact else _block_sum_np(qv[:n])) / n
    penalty = lse - qbar
    p = e / S
    inv_n = 1.0 / n
    dq = qv[:n] - y
    terms = dq * dq
    g = np.concatenate([(2.0 * dq) * inv_n + cw * (p[:n] - inv_n), cw * p[n:]])[:, None]
    ghead = g if exact else g.astype(np.float32)
    deltas: list = []
    value_loss = (math.fsum(terms) if exact else _block_sum_np(terms)) / n
    out = dict(grads=_backward(rounded, acts, ghead, activation, deltas), values=qv[:n], loss_terms=terms, loss=value_loss + cw * penalty,
               value_loss=value_loss, q=qv, weights=p, penalty=penalty, scalars=np.array([m, S, lse, qbar]))
    return _with_backprop(out, exact, acts, deltas)


def _pathwise_check(alpha, bc_coef) -> Tuple[float, float]:
    alpha, bc_coef = float(alpha), float(bc_coef)
    for k, x in (("alpha", alpha), ("bc_coef", bc_coef)):
        if not math.isfinite(x) or x < 0.0:
            raise ValueError(f"{k} = {x} must be finite and >= 0")
    return alpha, bc_coef


def _awr_check(temperature, weight_max) -> Tuple[float, float]:
    temperature, weight_max = float(temperature), float(weight_max)
    for k, x in (("temperature", temperature), ("weight_max", weight_max)):
        if math.isnan(x) or not x > 0.0:
            raise ValueError(f"{k} = {x} must be > 0 (inf allowed)")
    return temperature, weight_max


def _expectile_check(expectile) -> float:
    tau = float(expectile)
    if not 0.0 < tau < 1.0:
        raise ValueError(f"expectile = {expectile} must lie in (0, 1)")
    return tau


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


def anchor_term_np(g, w, prox=None, mu: float = 0.0, importance=None, centre=None, lam: float = 0.0) -> np.ndarray:
    """The terms on the parameters in float32, operation by operation as ``gs_k_train_anchor`` performs them (include/gridstep.h
    "parameter anchors"): ``g`` the reduced gradient of the loss and ``w`` the master parameters, arrays of one shape; ``mu`` != 0:
    ``g = g + mu * (w - prox)``; ``lam`` != 0: ``g = g + lam * (importance * (w - centre))``; the coefficients rounded once to
    float32.  Returns the total gradient, what ``grad_norm``, the clip and Adam see."""
    f = np.float32
    g, w = np.asarray(g, dtype=f), np.asarray(w, dtype=f)
    if f(mu) != f(0.0):
        g = g + f(mu) * (w - np.asarray(prox, dtype=f))
    if f(lam) != f(0.0):
        g = g + f(lam) * (np.asarray(importance, dtype=f) * (w - np.asarray(centre, dtype=f)))
    return g


def anchor_penalty_terms_np(w, prox=None, importance=None, centre=None) -> Tuple[Optional[np.ndarray], Optional[np.ndarray]]:
    """The float64 terms ``gs_k_train_anchor`` sums for ``gs_learner_anchor_stats``: ``d d`` with d the FLOAT32 difference w - prox,
    and ``A (d d)`` with d the float32 difference w - centre (None for a slot that is not given).  ``penalty_prox = mu / 2`` times
    the sum of the first, ``penalty_ewc = lambda / 2`` times the sum of the second."""
    f = np.float32
    w = np.asarray(w, dtype=f)
    tp = te = None
    if prox is not None:
        d = (w - np.asarray(prox, dtype=f)).astype(np.float64)
        tp = d * d
    if importance is not None:
        d = (w - np.asarray(centre, dtype=f)).astype(np.float64)
        te = np.asarray(importance, dtype=f).astype(np.float64) * (d * d)
    return tp, te


def fisher_np(result: Dict[str, Any], n: int, exact: bool = False) -> List[Tuple[np.ndarray, np.ndarray]]:
    """The per-sample (empirical) Fisher diagonal of a minibatch, SUMMED over its samples, as ``gs_learner_fisher_accumulate`` adds
    it to the pending sum: [(FW_l, Fb_l)] with ``FW_l = sum_i ((n delta_l[i])^2)^T (a_l[i])^2`` and ``Fb_l = sum_i (n delta_l[i])^2``
    from the ``passes`` a ``*_grad_np`` result carries (``acts`` and ``deltas`` in the evaluation's own precision: evaluate it with the same ``exact``);
    ``n``: the minibatch size the head divided by.  ``n delta`` is d l_i / d(pre-activation) of the per-sample terms l_i of
    L = (1/n) sum l_i, so every entry is sum_i (d l_i / d theta)^2.  Float64 when ``exact``; float32 products and sums otherwise."""
    work = np.float64 if exact else np.float32
    if "passes" not in result or result["passes"]["exact"] != bool(exact):
        raise ValueError(f"fisher_np: evaluate the restatement with exact={bool(exact)} (its result carries the passes in that precision)")
    acts, deltas = result["passes"]["acts"], result["passes"]["deltas"]
    out = []
    for l, d in enumerate(deltas):
        t = work(n) * np.asarray(d).astype(work)
        A = t * t
        a = np.asarray(acts[l]).astype(work)
        out.append((A.T @ (a * a), A.sum(axis=0)))
    return out


def fisher_importance_np(pending, samples: int, min_importance: float = 1e-3) -> np.ndarray:
    """``F = max(float32(pending / samples), float32(min_importance))`` of ``gs_learner_fisher_commit`` (float32)."""
    f = np.float32
    return np.maximum((np.asarray(pending, dtype=np.float64) / float(samples)).astype(f), f(min_importance))


def ewc_merge_np(A, c, F, w, decay: float = 1.0, exact: bool = False) -> Tuple[np.ndarray, np.ndarray]:
    """The merge of ``gs_learner_fisher_commit``: the consolidated importance ``A`` and centre ``c`` (None: the slot is empty) take a
    task of importance ``F`` whose optimum is ``w``: ``A' = decay A + F``, ``c' = ((decay A) c + F w) / A'`` (``w`` where ``A'`` is 0),
    per parameter in float64 on the float32 values, each rounded once to float32.  The first merge gives (F, w).  ``exact``: float64
    in and out, nothing rounded to float32 -- the recursion whose ``A (p - c)`` is ``sum_k decay^(K - 1 - k) F_k (p - p_k)``."""
    f = np.float64 if exact else np.float32
    F64, w64 = np.asarray(F, dtype=f).astype(np.float64), np.asarray(w, dtype=f).astype(np.float64)
    if A is None:
        return F64.astype(f), w64.astype(f)
    dA = float(decay) * np.asarray(A, dtype=f).astype(np.float64)
    An = dA + F64
    with np.errstate(invalid="ignore", divide="ignore"):
        cn = np.where(An != 0.0, (dA * np.asarray(c, dtype=f).astype(np.float64) + F64 * w64) / An, w64)
    return An.astype(f), cn.astype(f)


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
    ``ent_coef`` are the policy's.  ``policy_loss``: "ppo" (the clipped surrogate), "awr" (the advantage-weighted log-likelihood of
    the stored actions, weights ``fmin(exp(A / temperature), weight_max)``; it needs no recorded log-probabilities, so a random-
    or uploaded-action rollout trains the policy) or "bc" (AWR with both ``inf``: behaviour cloning).  ``value_loss``: "mse" or
    "expectile" (IQL's value loss at ``expectile``), for every critic named.  Creating the learner snapshots each network's installed weights as float32 master parameters and
    zeroes Adam's state; installing a network again ends its learner (create a new ``DeviceLearner``).

    State-action critics: "q1" and "q2" name the twin Q networks of ``env.set_q``; their step regresses
    Q(s, a) on the one-step TD target of the last ``evaluate_rollout_q`` (``q_loss``: "mse" or "expectile") over the batch's
    observations and, through its indices, the rollout's stored actions.  ``advantage_source="q"``: the policy's head weights with
    ``q_adv = min(Q1, Q2) - V`` of that evaluation instead of the batch's advantages; ``value_target="q"``: the reward critic
    regresses on the target networks' ``min(Q1, Q2)`` instead of the batch's returns -- with ``policy_loss="awr"`` and
    ``value_loss="expectile"`` that is IQL.  ``update_targets(tau)`` moves the target networks.

    Policy-action targets: ``q_target="policy"`` makes the Q learners regress on ``td_target`` of the last
    ``evaluate_rollout_q_next`` -- ``r' + gamma (min Q_target(s', pi(s')) - alpha log pi(a' | s'))``, the critic target of SAC,
    TD3 + BC and DDPG -- instead of the last ``evaluate_rollout_q``'s (``set_q_target`` changes it later; it is the handle's state).

    The pathwise actor: ``policy_loss="pathwise"`` makes the policy's step ``gs_learner_step_pathwise`` --
    ``mean(alpha lp - min(Q1, Q2)(s, a) + bc_coef |a - a_stored|^2)`` with ``a`` sampled inside the step
    (``pathwise_stochastic=False``: ``a = tanh(mean)``) and the gradient flowing through the installed twins, which need learners
    ("q1" / "q2" among ``nets``, of this or of another ``DeviceLearner`` on the handle) but are not stepped by it.  The noise of a
    step is ``pathwise_noise_np(pathwise_seed, draw, n, A)`` with ``draw`` = the policy's steps taken.  Host state: the C loss kind
    is not involved.

    Per-minibatch targets: ``fresh_targets=True`` makes ``step(batch)`` re-evaluate, for the batch's
    transitions and with the networks as they are at that moment, the signals its steps are about to read (``refresh_targets``),
    in the reference's order.  Under ``q_target="policy"``: "td_policy" (``gamma``, this learner's ``alpha``, ``bootstrap``, noise
    seed ``target_seed``, ``draw`` = the first Q net's steps taken, sampled unless ``pathwise_stochastic=False``), the Q steps,
    then the other networks.  Under the IQL wiring (``advantage_source="q"`` and ``value_target="q"``): "q_target", the value
    step, "td_value", the Q steps, "q_adv", the policy step.  The full evaluations (``evaluate_rollout_q_next`` /
    ``evaluate_rollout_q``) then run once, before the first epoch.  The default calls no new entry.

    The conservative critic: ``conservative_weight`` > 0 makes the Q networks' step
    ``gs_learner_step_conservative`` -- CQL's ``mse(Q(s, a), y) + conservative_weight (logsumexp over the batch of Q(s, a_data) |
    Q(s, a_uniform) | Q(s, a_policy) - mean Q(s, a_data))`` per twin, the policy's candidates sampled inside the step
    (``conservative_stochastic=False``: ``tanh(mean)``).  It needs ``q_loss="mse"`` and a learner for the policy on the handle (of
    this or of another ``DeviceLearner``), which it reads and does not step.  The uniform candidates of a step are
    ``cql_uniform_np(conservative_seed, draw, n, A)`` and its noise ``cql_noise_np(...)`` with ``draw`` = that twin's steps taken.

    Parameter anchors: ``anchor_here`` / ``set_anchor(prox_mu=)`` add FedProx's proximal term to every later
    step of a network, ``consolidate`` / ``set_anchor(ewc_lambda=)`` elastic weight consolidation on the per-sample Fisher diagonal
    of the network's own loss; both are off until asked for and act on the reduced gradient on the device.

    ``step(batch)``: one ``gs_learner_step`` per network on a dict of ``OnPolicyBatches.epoch`` (prepared with float32 and the
    networks' own observation normalisation).  After a step the ``MLPPolicy`` / ``MLPValue`` objects the networks were installed
    from no longer describe them: ``policy()`` / ``value(net)`` rebuild current ones from the device's parameters."""

    def __init__(self, env, nets: Sequence[str] = ("policy", "value"), lr: float = 3e-4, betas: Tuple[float, float] = (0.9, 0.999),
                 eps: float = 1e-8, weight_decay: float = 0.0, clip: float = 0.2, ent_coef: float = 0.0, max_grad_norm: float = 0.0,
                 policy_loss: str = "ppo", temperature: float = 1.0, weight_max: float = 20.0, value_loss: str = "mse",
                 expectile: float = 0.7, q_loss: str = "mse", advantage_source: str = "batch", value_target: str = "batch",
                 alpha: float = 0.0, bc_coef: float = 0.0, pathwise_stochastic: bool = True, pathwise_seed: int = 0,
                 q_target: str = "value", conservative_weight: float = 0.0, conservative_stochastic: bool = True,
                 conservative_seed: int = 0, fresh_targets: bool = False, gamma: float = 0.99, bootstrap: Sequence[str] = (),
                 target_seed: int = 0) -> None:
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
        self._loss_struct(_lib.GS_LEARNER_POLICY, policy_loss, temperature, weight_max, expectile)      # (ValueError also for a
        self._loss_struct(_lib.GS_LEARNER_VALUE, value_loss, temperature, weight_max, expectile)        # network not in `nets`)
        self._loss_struct(_lib.GS_LEARNER_Q, q_loss, temperature, weight_max, expectile, what="q_loss")
        losses = {k: self._loss_struct(k, policy_loss if k == _lib.GS_LEARNER_POLICY else q_loss if k >= _lib.GS_LEARNER_Q else value_loss,
                                       temperature, weight_max, expectile) for k in self._ids}
        signals = {}
        for what, source, k in (("advantage_source", advantage_source, _lib.GS_LEARNER_POLICY), ("value_target", value_target, _lib.GS_LEARNER_VALUE)):
            if source not in _lib.SIGNALS:
                raise ValueError(f"DeviceLearner: {what} = {source!r} must be one of {sorted(_lib.SIGNALS)}")
            if source == "q":
                if k not in self._ids:
                    raise ValueError(f"DeviceLearner: {what} = 'q' needs {'policy' if k == _lib.GS_LEARNER_POLICY else 'value'!r} among nets {self.nets}")
                signals[k] = source
        self.advantage_source, self.value_target = advantage_source, value_target
        self._pathwise: Optional[dict] = None
        if policy_loss == "pathwise":
            if _lib.GS_LEARNER_POLICY not in self._ids:
                raise ValueError(f"DeviceLearner: policy_loss = 'pathwise' needs 'policy' among nets {self.nets}")
            self._pathwise = self._pathwise_state(alpha, bc_coef, pathwise_stochastic, pathwise_seed)
        else:
            _pathwise_check(alpha, bc_coef)
        if q_target not in _lib.Q_TARGETS:
            raise ValueError(f"DeviceLearner: q_target = {q_target!r} must be one of {sorted(_lib.Q_TARGETS)}")
        if q_target == "policy" and not any(k >= _lib.GS_LEARNER_Q for k in self._ids):
            raise ValueError(f"DeviceLearner: q_target = 'policy' needs 'q1' or 'q2' among nets {self.nets}")
        self.q_target = q_target
        self._conservative: Optional[dict] = None
        state = self._conservative_state(conservative_weight, conservative_stochastic, conservative_seed)
        if state["conservative_weight"] > 0.0:
            if not any(k >= _lib.GS_LEARNER_Q for k in self._ids):
                raise ValueError(f"DeviceLearner: conservative_weight > 0 needs 'q1' or 'q2' among nets {self.nets}")
            if q_loss != "mse":
                raise ValueError(f"DeviceLearner: conservative_weight > 0 needs q_loss = 'mse' (the penalty joins the squared error), got {q_loss!r}")
            self._conservative = state
        self._fresh: Optional[dict] = None
        if not isinstance(fresh_targets, (bool, np.bool_)):
            raise ValueError(f"DeviceLearner: fresh_targets = {fresh_targets!r} must be True or False")
        if fresh_targets:
            self._fresh = self._fresh_state(q_target, advantage_source, value_target, gamma, bootstrap, target_seed, float(alpha),
                                            bool(pathwise_stochastic))
        self.fresh_targets = bool(fresh_targets)
        self.env = env
        self.config = dict(lr=float(lr), betas=(float(betas[0]), float(betas[1])), eps=float(eps), weight_decay=float(weight_decay),
                           clip=float(clip), ent_coef=float(ent_coef), max_grad_norm=float(max_grad_norm))
        cfg = _lib.learner_config(**self.config)
        for net in self._ids:
            env.handle.learner_create(net, cfg)
            if losses[net].kind != _lib.GS_LOSS_DEFAULT:      # (a learner left at "ppo" / "mse" never calls the entry)
                env.handle.learner_set_loss(net, losses[net])
            if net in signals:                                # (a learner left at "batch" never calls the entry)
                env.handle.learner_set_signal(net, signals[net])
        if q_target != "value":                               # (a learner left at "value" never calls the entry)
            env.handle.q_set_target_source(q_target)

    @staticmethod
    def _loss_struct(k: int, loss: str, temperature, weight_max, expectile, what: Optional[str] = None) -> "_lib.gs_learner_loss":
        """The ``gs_learner_loss`` of network number ``k`` for the loss named ``loss``; ValueError for what the ABI would refuse."""
        policy = k == _lib.GS_LEARNER_POLICY
        names = ("ppo", "awr", "bc", "pathwise") if policy else ("mse", "expectile")
        if loss not in names:
            raise ValueError(f"DeviceLearner: {what or ('policy_loss' if policy else 'value_loss')} = {loss!r} must be one of {names}")
        if loss == "bc":
            return _lib.learner_loss("awr", math.inf, math.inf, 0.0)
        if loss == "awr":
            temperature, weight_max = _awr_check(temperature, weight_max)
            return _lib.learner_loss("awr", temperature, weight_max, 0.0)
        if loss == "expectile":
            return _lib.learner_loss("expectile", 0.0, 0.0, _expectile_check(expectile))
        return _lib.learner_loss("default", 0.0, 0.0, 0.0)

    @staticmethod
    def _pathwise_state(alpha, bc_coef, stochastic, seed) -> dict:
        alpha, bc_coef = _pathwise_check(alpha, bc_coef)
        if not isinstance(stochastic, (bool, np.bool_)):
            raise ValueError(f"DeviceLearner: pathwise_stochastic = {stochastic!r} must be True or False")
        if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not 0 <= int(seed) < 2 ** 64:
            raise ValueError(f"DeviceLearner: pathwise_seed = {seed!r} must be an integer in [0, 2^64)")
        return dict(alpha=alpha, bc_coef=bc_coef, stochastic=bool(stochastic), seed=int(seed))

    @staticmethod
    def _conservative_state(conservative_weight, stochastic, seed) -> dict:
        cw = _cql_weight_check(conservative_weight)
        if not isinstance(stochastic, (bool, np.bool_)):
            raise ValueError(f"DeviceLearner: conservative_stochastic = {stochastic!r} must be True or False")
        if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not 0 <= int(seed) < 2 ** 64:
            raise ValueError(f"DeviceLearner: conservative_seed = {seed!r} must be an integer in [0, 2^64)")
        return dict(conservative_weight=cw, stochastic=bool(stochastic), seed=int(seed))

    def _fresh_state(self, q_target, advantage_source, value_target, gamma, bootstrap, seed, alpha, stochastic) -> dict:
        """What ``fresh_targets=True`` refreshes per minibatch, and under which configuration; ValueError for what cannot be."""
        if not any(k >= _lib.GS_LEARNER_Q for k in self._ids):
            raise ValueError(f"DeviceLearner: fresh_targets = True needs 'q1' or 'q2' among nets {self.nets}")
        if q_target == "policy":
            wiring = "policy"
        elif advantage_source == "q" and value_target == "q":
            wiring = "iql"
        else:
            raise ValueError("DeviceLearner: fresh_targets = True needs q_target = 'policy' (the policy-action target) or the IQL wiring "
                             "(advantage_source = 'q' and value_target = 'q')")
        gamma = float(gamma)
        if not math.isfinite(gamma):
            raise ValueError(f"DeviceLearner: gamma = {gamma} must be finite")
        if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not 0 <= int(seed) < 2 ** 64:
            raise ValueError(f"DeviceLearner: target_seed = {seed!r} must be an integer in [0, 2^64)")
        return dict(wiring=wiring, gamma=gamma, mask=_bootstrap_mask(bootstrap), seed=int(seed), alpha=alpha, stochastic=stochastic)

    def _refresh(self, batch: dict, groups: str, stream=None) -> None:
        """One ``gs_learner_refresh`` of ``groups`` on ``batch`` under the ``fresh_targets`` configuration; the noise of
        "td_policy" is drawn with ``draw`` = the first Q net's steps taken."""
        f = self._fresh
        draw = 0
        if groups == "td_policy":
            draw = int(self.env.handle.learner_info(next(k for k in self._ids if k >= _lib.GS_LEARNER_Q))["step"]) & 0xFFFFFFFF
        cfg = _lib.refresh_config(groups, f["gamma"], f["alpha"] if groups == "td_policy" else 0.0, f["mask"], f["stochastic"], f["seed"], draw)
        self.env.handle.learner_refresh(batch, cfg, stream=stream)

    def set_loss(self, net="policy", loss: Optional[str] = None, temperature: float = 1.0, weight_max: float = 20.0,
                 expectile: float = 0.7, alpha: float = 0.0, bc_coef: float = 0.0, pathwise_stochastic: bool = True,
                 pathwise_seed: int = 0) -> None:
        """Another loss for ``net`` from its next step (``gs_learner_set_loss``): the policy's "ppo", "awr" (``temperature``,
        ``weight_max``), "bc" or "pathwise" (``alpha``, ``bc_coef``, ``pathwise_stochastic``, ``pathwise_seed``; host state, the C
        loss returns to its default); a critic's "mse" or "expectile" (``expectile``).  Adam's moments and step count stay, and a
        ``FederatedLearners`` on the learner stays valid."""
        k = self._id(net)
        if loss is None:
            raise ValueError("DeviceLearner.set_loss: name the loss")
        struct = self._loss_struct(k, loss, temperature, weight_max, expectile)
        state = self._pathwise_state(alpha, bc_coef, pathwise_stochastic, pathwise_seed) if loss == "pathwise" else None
        self.env.handle.learner_set_loss(k, struct)
        if k == _lib.GS_LEARNER_POLICY:
            self._pathwise = state

    def loss(self, net="policy") -> dict:
        """The loss of ``net`` in force: ``name`` ("ppo", "awr", "bc", "mse" or "expectile") and ``gs_learner_get_loss``'s ``kind``,
        ``temperature``, ``weight_max`` and ``expectile``."""
        k = self._id(net)
        out = self.env.handle.learner_get_loss(k)
        if k == _lib.GS_LEARNER_POLICY and self._pathwise is not None:
            out.update(self._pathwise, name="pathwise")
        elif out["kind"] == "default":
            out["name"] = "ppo" if k == _lib.GS_LEARNER_POLICY else "mse"
        elif out["kind"] == "awr":
            out["name"] = "bc" if math.isinf(out["temperature"]) and math.isinf(out["weight_max"]) else "awr"
        else:
            out["name"] = "expectile"
        return out

    def _id(self, net) -> int:
        k = _lib._net_number(net)
        if k not in self._ids:
            raise ValueError(f"DeviceLearner: {net!r} is not one of this learner's networks {self.nets}")
        return k

    def step(self, batch: dict, stream=None) -> None:
        """One update of every network on ``batch`` (asynchronous on the handle's stream; ``stream``: a consumer's stream)."""
        n = int(batch["observations"].shape[0])
        if self._fresh is not None:
            return self._step_fresh(batch, n, stream)
        for net in self._ids:
            self._step_net(net, batch, n, stream)

    def _step_net(self, net: int, batch: dict, n: int, stream=None) -> None:
        if net == _lib.GS_LEARNER_POLICY and self._pathwise is not None:
            self.step_pathwise(batch, stream=stream)
        elif net >= _lib.GS_LEARNER_Q and self._conservative is not None:
            self.step_conservative(batch, net, stream=stream)
        else:
            self.env.handle.learner_step(net, batch, n, stream)

    def _step_fresh(self, batch: dict, n: int, stream=None) -> None:
        """``step`` under ``fresh_targets=True``: the reference's order of recomputation and optimiser steps inside one
        ``update(batch)``.  The policy-action wiring (algorithms/offline.py:166-255): "td_policy", the Q steps, then every other
        network.  The IQL wiring (:482-540): "q_target", the value step, "td_value", the Q steps, "q_adv", the policy step, then
        every other network."""
        qs = [k for k in self._ids if k >= _lib.GS_LEARNER_Q]
        if self._fresh["wiring"] == "policy":
            self._refresh(batch, "td_policy", stream)
            order = qs + [k for k in self._ids if k < _lib.GS_LEARNER_Q]
            for net in order:
                self._step_net(net, batch, n, stream)
            return
        self._refresh(batch, "q_target", stream)
        self._step_net(_lib.GS_LEARNER_VALUE, batch, n, stream)
        self._refresh(batch, "td_value", stream)
        for net in qs:
            self._step_net(net, batch, n, stream)
        self._refresh(batch, "q_adv", stream)
        self._step_net(_lib.GS_LEARNER_POLICY, batch, n, stream)
        for net in self._ids:
            if net not in qs and net not in (_lib.GS_LEARNER_VALUE, _lib.GS_LEARNER_POLICY):
                self._step_net(net, batch, n, stream)

    def step_pathwise(self, batch: dict, alpha: Optional[float] = None, bc_coef: Optional[float] = None, stochastic: Optional[bool] = None,
                      seed: Optional[int] = None, draw: Optional[int] = None, stream=None) -> None:
        """One pathwise actor update of the policy on ``batch`` (``gs_learner_step_pathwise``, asynchronous): what is not given is
        the learner's ``policy_loss="pathwise"`` state (``alpha`` 0, ``bc_coef`` 0, stochastic, seed 0 without one); ``draw``: by
        default the policy's steps taken."""
        k = self._id("policy")
        base = self._pathwise or dict(alpha=0.0, bc_coef=0.0, stochastic=True, seed=0)
        state = self._pathwise_state(base["alpha"] if alpha is None else alpha, base["bc_coef"] if bc_coef is None else bc_coef,
                                     base["stochastic"] if stochastic is None else stochastic, base["seed"] if seed is None else seed)
        if draw is None:
            draw = self.env.handle.learner_info(k)["step"]
        if isinstance(draw, bool) or not isinstance(draw, (int, np.integer)) or not 0 <= int(draw) < 2 ** 32:
            raise ValueError(f"DeviceLearner.step_pathwise: draw = {draw!r} must be an integer in [0, 2^32)")
        cfg = _lib.pathwise_config(state["alpha"], state["bc_coef"], state["stochastic"], state["seed"], int(draw))
        self.env.handle.learner_step_pathwise(batch, int(batch["observations"].shape[0]), cfg, stream)

    def pathwise_views(self, stream=None) -> dict:
        """The last pathwise step's arrays as zero-copy ``DeviceArray`` views (``gs_learner_pathwise_view``): ``actions``, ``noise``
        [n, A], ``log_probs``, ``q_min``, ``bc_terms``, ``loss_terms`` [n], ``which`` [n] (int32), ``q`` and ``dq_da`` lists per twin
        (None for a twin that is not installed), ``installed``, and ``pre_head`` / ``pre_head_stride`` (the policy's float32 rows
        mean | log_std in the learners' shared scratch, valid until any learner's next step)."""
        self._id("policy")
        return self.env.handle.learner_pathwise_view(stream)

    def step_conservative(self, batch: dict, net, conservative_weight: Optional[float] = None, stochastic: Optional[bool] = None,
                          seed: Optional[int] = None, draw: Optional[int] = None, stream=None) -> None:
        """One conservative critic update of twin ``net`` ("q1" / "q2") on ``batch`` (``gs_learner_step_conservative``,
        asynchronous): what is not given is the learner's ``conservative_weight`` state (weight 0, stochastic, seed 0 without one);
        ``draw``: by default that twin's steps taken, so twins stepped in turn see the same candidate actions."""
        k = self._id(net)
        if k < _lib.GS_LEARNER_Q:
            raise ValueError(f"DeviceLearner.step_conservative: {net!r} is not a Q network ('q1' / 'q2')")
        base = self._conservative or dict(conservative_weight=0.0, stochastic=True, seed=0)
        state = self._conservative_state(base["conservative_weight"] if conservative_weight is None else conservative_weight,
                                         base["stochastic"] if stochastic is None else stochastic, base["seed"] if seed is None else seed)
        if draw is None:
            draw = self.env.handle.learner_info(k)["step"]
        if isinstance(draw, bool) or not isinstance(draw, (int, np.integer)) or not 0 <= int(draw) < 2 ** 32:
            raise ValueError(f"DeviceLearner.step_conservative: draw = {draw!r} must be an integer in [0, 2^32)")
        cfg = _lib.conservative_config(state["conservative_weight"], state["stochastic"], state["seed"], int(draw))
        self.env.handle.learner_step_conservative(k, batch, int(batch["observations"].shape[0]), cfg, stream)

    def conservative_views(self, stream=None) -> dict:
        """The last conservative step's arrays as zero-copy ``DeviceArray`` views (``gs_learner_conservative_view``):
        ``random_actions``, ``policy_actions``, ``policy_noise`` [n, A], ``policy_log_probs``, ``loss_terms`` [n], ``q``, ``weights``
        [3 n] (rows: data | uniform | policy), ``scalars`` [4] (m, S, lse, qbar), ``targets`` [n] (float32), ``net``, ``n``,
        ``action_dim``, and ``pre_head`` / ``pre_head_stride`` as ``pathwise_views``'."""
        if not any(k >= _lib.GS_LEARNER_Q for k in self._ids):
            raise ValueError(f"DeviceLearner.conservative_views: no Q network among this learner's nets {self.nets}")
        return self.env.handle.learner_conservative_view(stream)

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
        key = ("policy" if k == _lib.GS_LEARNER_POLICY else "value" if k == _lib.GS_LEARNER_VALUE else _lib.Q_NETS[k - _lib.GS_LEARNER_Q]
               if k >= _lib.GS_LEARNER_Q else k - _lib.GS_LEARNER_COST_VALUE)
        meta = self.env._installed_nets().get(key)
        if meta is None:
            raise _lib.PowerFlowError("DeviceLearner: the network was not installed through this environment (set_policy / set_value / set_cost_value / set_q)")
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
        if k == _lib.GS_LEARNER_POLICY or k >= _lib.GS_LEARNER_Q:
            raise ValueError("DeviceLearner.value: a state critic is meant (policy() / q(which) for the others)")
        meta = self._meta(k)
        W, b = self.parameters(k)
        return MLPValue(W, b, activation=self.env.handle.learner_info(k)["activation"], obs_mean=meta["obs_mean"], obs_std=meta["obs_std"])

    def set_signal(self, net, source: str) -> None:
        """"batch" or "q" for the policy's advantages / the reward critic's regression target, from the next step
        (``gs_learner_set_signal``); Adam's state stays."""
        k = self._id(net)
        if source not in _lib.SIGNALS:
            raise ValueError(f"DeviceLearner.set_signal: source = {source!r} must be one of {sorted(_lib.SIGNALS)}")
        if source == "q" and k not in (_lib.GS_LEARNER_POLICY, _lib.GS_LEARNER_VALUE):
            raise ValueError("DeviceLearner.set_signal: 'q' is for the policy and the reward critic")
        self.env.handle.learner_set_signal(k, source)
        if k == _lib.GS_LEARNER_POLICY:
            self.advantage_source = source
        else:
            self.value_target = source

    def signal(self, net) -> str:
        return self.env.handle.learner_get_signal(self._id(net))

    def set_q_target(self, source: str) -> None:
        """Which Bellman target the Q learners regress on from their next step (``gs_q_set_target_source``; state of the HANDLE,
        shared by every learner on it): "value", ``td_target`` of the last ``evaluate_rollout_q`` (``r' + gamma V(s')``), or
        "policy", ``td_target`` of the last ``evaluate_rollout_q_next`` (``r' + gamma (min Q_target(s', pi(s')) - alpha log pi)``)."""
        if source not in _lib.Q_TARGETS:
            raise ValueError(f"DeviceLearner.set_q_target: source = {source!r} must be one of {sorted(_lib.Q_TARGETS)}")
        if not any(k >= _lib.GS_LEARNER_Q for k in self._ids):
            raise ValueError(f"DeviceLearner.set_q_target: no Q network among this learner's nets {self.nets}")
        self.env.handle.q_set_target_source(source)
        self.q_target = source

    def update_targets(self, tau: float = 0.005) -> None:
        """The target networks of every installed twin move towards the online ones, ``t = tau p + (1 - tau) t`` in float32 on the
        device (``gs_q_target_update``, asynchronous; ``polyak_np`` restates it)."""
        tau = float(tau)
        if not (math.isfinite(tau) and 0.0 <= tau <= 1.0):
            raise ValueError(f"DeviceLearner.update_targets: tau = {tau} must lie in [0, 1]")
        self.env.handle.q_target_update(tau)

    def _q_object(self, k: int, flat) -> MLPQ:
        meta = self._meta(k)
        info = self.env.handle.learner_info(k)
        W, b = split_parameters(flat, info["dims"])
        return MLPQ(W, b, meta["obs_dim"], activation=info["activation"], obs_mean=meta["obs_mean"], obs_std=meta["obs_std"])

    def q(self, which) -> MLPQ:
        """A current ``MLPQ`` of twin ``which`` (0 / 1 / "q1" / "q2") from the device's master parameters, as ``policy()``."""
        k = self._id(_lib.Q_NETS[_lib.q_which(which)])
        return self._q_object(k, self.env.handle.learner_download(k, ("params",))["params"])

    def target_q(self, which) -> MLPQ:
        """The TARGET network of twin ``which`` as an ``MLPQ`` (``gs_q_target_download``)."""
        w = _lib.q_which(which)
        k = self._id(_lib.Q_NETS[w])
        return self._q_object(k, self.env.handle.q_target_download(w, self.env.handle.learner_info(k)["param_count"]))

    def views(self, net="policy", stream=None) -> dict:
        """The last step's per-sample arrays as zero-copy ``DeviceArray`` views: ``log_probs_new``, ``ratio`` (float64), ``clipped``
        (int32), ``loss_terms`` and ``entropy_terms`` (float64) [n]; None where the network has none (a critic has ``loss_terms``).
        Under "awr" / "bc" ``ratio`` holds the weights, ``clipped`` the cap flags and ``loss_terms`` weight x log-probability; under
        "expectile" ``loss_terms`` holds q (v - ret)^2."""
        k = self._id(net)
        return self.env.handle.learner_view(k, stream)

    # -- parameter anchors ----------------------------------------------------------------------------------
    def anchor_here(self, net="policy", params=None) -> None:
        """The PROX centre of ``net`` (``gs_learner_anchor_here``): ``params`` (flat float32 in torch order), or by default a device
        copy of the learner's current master parameters -- after a federated round, the global model."""
        self.env.handle.learner_anchor_here(self._id(net), params)

    def set_anchor(self, net="policy", prox_mu: Optional[float] = None, ewc_lambda: Optional[float] = None) -> None:
        """The coefficients of the terms on ``net``'s parameters from its next step (``gs_learner_anchor_set``): FedProx's
        ``prox_mu / 2 |w - a|^2`` (it needs ``anchor_here`` first) and EWC's ``ewc_lambda / 2 sum A (w - c)^2`` (it needs a
        ``consolidate`` first).  What is not given stays as it is; 0 turns a term off, and with both at 0 a step is, launch for
        launch and bit for bit, a step of a learner without anchors."""
        k = self._id(net)
        now = self.env.handle.learner_anchor_get(k)
        cfg = dict(prox_mu=now["prox_mu"] if prox_mu is None else float(prox_mu), ewc_lambda=now["ewc_lambda"] if ewc_lambda is None else float(ewc_lambda))
        for key, x in cfg.items():
            if not math.isfinite(x) or x < 0.0:
                raise ValueError(f"DeviceLearner.set_anchor: {key} = {x} must be finite and >= 0")
        self.env.handle.learner_anchor_set(k, _lib.anchor_config(**cfg))

    def anchor(self, net="policy") -> dict:
        """``prox_mu`` and ``ewc_lambda`` of ``net`` in force (``gs_learner_anchor_get``)."""
        return self.env.handle.learner_anchor_get(self._id(net))

    def consolidate(self, net, batches, min_importance: float = 1e-3, decay: float = 1.0, stream=None) -> int:
        """The end of a task for ``net`` (elastic weight consolidation): the per-sample Fisher diagonal of ``net``'s own loss over the
        minibatches of the iterable ``batches`` (dicts as ``step`` takes them; ``gs_learner_fisher_begin`` / ``_accumulate``), then
        ``gs_learner_fisher_commit``: ``F = max(mean, min_importance)`` is merged into the consolidated importance with the CURRENT
        parameters as the task's optimum (``decay`` 1: the sum over tasks; below 1: online EWC).  No parameter, moment or statistic
        changes.  Returns the number of samples."""
        k = self._id(net)
        if (k == _lib.GS_LEARNER_POLICY and self._pathwise is not None) or (k >= _lib.GS_LEARNER_Q and self._conservative is not None):
            raise ValueError("DeviceLearner.consolidate: the pathwise and the conservative step couple the samples of a batch; no per-sample Fisher is offered for them")
        min_importance, decay = float(min_importance), float(decay)
        if not math.isfinite(min_importance) or min_importance < 0.0:
            raise ValueError(f"DeviceLearner.consolidate: min_importance = {min_importance} must be finite and >= 0")
        if not 0.0 < decay <= 1.0:
            raise ValueError(f"DeviceLearner.consolidate: decay = {decay} must lie in (0, 1]")
        h = self.env.handle
        h.learner_fisher_begin(k)
        samples = 0
        for batch in batches:
            n = int(batch["observations"].shape[0])
            h.learner_fisher_accumulate(k, batch, n, stream)
            samples += n
        h.learner_fisher_commit(k, _lib.fisher_config(min_importance, decay))
        return samples

    def clear_anchor(self, net="policy", which: str = "both") -> None:
        """Drops the "prox" slot, the "ewc" slot or "both" of ``net``; a cleared slot's coefficient becomes 0."""
        self.env.handle.learner_anchor_clear(self._id(net), which)

    def anchor_stats(self, net="policy") -> dict:
        """Of ``net``'s last step with a non-zero coefficient (waits for it): ``penalty_prox``, ``penalty_ewc`` (at the parameters
        before Adam), ``grad_norm_loss`` (the norm before the terms; ``stats(net)["grad_norm"]`` is the total gradient's), the
        step's ``prox_mu`` / ``ewc_lambda``, ``tasks`` and ``fisher_samples``."""
        return self.env.handle.learner_anchor_stats(self._id(net))

    def anchor_arrays(self, net="policy", want=_lib.ANCHOR_ARRAYS) -> dict:
        """Flat host copies in torch order of ``prox``, ``ewc_importance``, ``ewc_centre`` (float32) and ``fisher_pending`` (float64,
        the open or last task's sum over ``fisher_samples`` samples)."""
        return self.env.handle.learner_anchor_download(self._id(net), want)
