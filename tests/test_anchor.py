"""CPU-only: parameter anchors (include/gridstep.h "parameter anchors") -- the NumPy restatements
``anchor_term_np``, ``fisher_np`` and ``ewc_merge_np`` against torch autograd in float64, the centre form of the merge against the
explicit sum over tasks, the value rules of ``gs_learner_anchor_check``, and the new symbols and struct layouts.

Bounds, by reasoning:
  the term        ``anchor_term_np`` works in float32 on a float32 gradient: the input's rounding and at most five rounded operations
                  per element, each 2^-24 relative to a quantity no larger than |g| + |mu d| + |lambda A d|: 6 x 2^-24 of that sum.
  the Fisher      float64 against float64 on the same float32-rounded operands: 1e-10 relative to the tensor's largest entry (sums of
                  at most a few hundred non-negative terms); the float32 form within 1e-4 of the largest entry.
  the merge       in float64 (``exact=True``) ``A (p - c)`` against ``sum_k F_k (p - p_k)``: 1e-12 relative to ``sum_k F_k |p - p_k|``,
                  the magnitude the cancellation works on; the float32 form is that result rounded once: 2^-24 relative per array."""
import ctypes
import inspect
import math

import numpy as np
import pytest

import grid_fed_rl_gym_amd as P
from grid_fed_rl_gym_amd import _lib
from grid_fed_rl_gym_amd.learner import (anchor_penalty_terms_np, anchor_term_np, ewc_merge_np, fisher_importance_np, fisher_np, value_grad_np,
                                         expectile_grad_np)

import torch

U32 = 2.0 ** -24


def _mlp(dims, seed):
    rng = np.random.default_rng(seed)
    ws = [rng.normal(0.0, 1.0 / math.sqrt(dims[l]), (dims[l + 1], dims[l])).astype(np.float32) for l in range(len(dims) - 1)]
    bs = [rng.normal(0.0, 0.1, dims[l + 1]).astype(np.float32) for l in range(len(dims) - 1)]
    return ws, bs


def _flat(ws, bs):
    return np.concatenate([np.concatenate([w.reshape(-1), b]) for w, b in zip(ws, bs)])


def _torch_forward(params, x, act=torch.tanh):
    for l, (w, b) in enumerate(params):
        x = x @ w.T + b
        if l < len(params) - 1:
            x = act(x)
    return x


def _torch_params(ws, bs):
    return [(torch.tensor(w.astype(np.float64), requires_grad=True), torch.tensor(b.astype(np.float64), requires_grad=True)) for w, b in zip(ws, bs)]


def _flat_grads(params):
    return np.concatenate([np.concatenate([w.grad.numpy().reshape(-1), b.grad.numpy()]) for w, b in params])


def test_the_term_is_the_gradient_of_both_penalties_added_to_a_loss():
    dims, n = [7, 12, 9, 1], 23
    ws, bs = _mlp(dims, 0)
    rng = np.random.default_rng(1)
    x = rng.normal(0.0, 1.0, (n, dims[0])).astype(np.float32)
    ret = rng.normal(0.0, 1.0, n).astype(np.float32)
    w = _flat(ws, bs)
    a = (w + rng.normal(0.0, 0.05, w.shape)).astype(np.float32)
    c = (w + rng.normal(0.0, 0.05, w.shape)).astype(np.float32)
    F = np.abs(rng.normal(0.0, 1.0, w.shape)).astype(np.float32)
    mu, lam = 0.3, 40.0

    def grads(with_terms):
        params = _torch_params(ws, bs)
        v = _torch_forward(params, torch.tensor(x.astype(np.float64)))[:, 0]
        loss = torch.mean((v - torch.tensor(ret.astype(np.float64))) ** 2)
        if with_terms:
            p = torch.cat([torch.cat([wl.reshape(-1), bl]) for wl, bl in params])
            loss = loss + mu / 2.0 * torch.sum((p - torch.tensor(a.astype(np.float64))) ** 2)
            loss = loss + lam / 2.0 * torch.sum(torch.tensor(F.astype(np.float64)) * (p - torch.tensor(c.astype(np.float64))) ** 2)
        loss.backward()
        return _flat_grads(params)

    g_loss, g_total = grads(False), grads(True)
    got = anchor_term_np(g_loss.astype(np.float32), w, prox=a, mu=mu, importance=F, centre=c, lam=lam)
    assert got.dtype == np.float32
    size = np.abs(g_loss) + mu * np.abs(w.astype(np.float64) - a) + lam * F * np.abs(w.astype(np.float64) - c)
    assert np.all(np.abs(got.astype(np.float64) - g_total) <= 6.0 * U32 * size)
    assert np.max(np.abs(g_total - g_loss)) > 1e-3                                   # the terms are there at all
    # each term alone, and none
    only_prox = anchor_term_np(g_loss.astype(np.float32), w, prox=a, mu=mu)
    only_ewc = anchor_term_np(g_loss.astype(np.float32), w, importance=F, centre=c, lam=lam)
    f = np.float32
    assert np.array_equal(only_prox, g_loss.astype(f) + f(mu) * (w - a))
    assert np.array_equal(only_ewc, g_loss.astype(f) + f(lam) * (F * (w - c)))
    assert np.array_equal(anchor_term_np(g_loss.astype(f), w), g_loss.astype(f))
    # a zero distance adds +0: the gradient's bits stay
    assert np.array_equal(anchor_term_np(g_loss.astype(f), w, prox=w, mu=mu).view(np.uint32), g_loss.astype(f).view(np.uint32))
    # the penalties' terms: the float32 difference, squared and weighted in float64
    tp, te = anchor_penalty_terms_np(w, prox=a, importance=F, centre=c)
    assert np.array_equal(tp, (w - a).astype(np.float64) ** 2) and np.array_equal(te, F.astype(np.float64) * ((w - c).astype(np.float64) ** 2))
    assert anchor_penalty_terms_np(w) == (None, None)


@pytest.mark.parametrize("loss", ["mse", "expectile"])
def test_the_fisher_diagonal_is_the_mean_of_per_sample_squared_gradients(loss):
    dims, n = [11, 20, 13, 1], 37                                                    # a 3-layer tanh MLP
    ws, bs = _mlp(dims, 3)
    rng = np.random.default_rng(4)
    x = rng.normal(0.0, 1.0, (n, dims[0])).astype(np.float32)
    ret = rng.normal(0.0, 1.0, n).astype(np.float32)
    layers = list(zip(ws, bs))
    tau = 0.7
    if loss == "mse":
        ex, lo = (value_grad_np(layers, x, ret, exact=e, activation="tanh") for e in (True, False))
    else:
        ex, lo = (expectile_grad_np(layers, x, ret, tau, exact=e, activation="tanh") for e in (True, False))
    assert ex["passes"]["exact"] and not lo["passes"]["exact"] and "backprop" not in lo
    want = None
    for i in range(n):
        params = _torch_params(ws, bs)
        v = _torch_forward(params, torch.tensor(x[i:i + 1].astype(np.float64)))[0, 0]
        d = v - float(ret[i])
        li = d * d if loss == "mse" else (tau if float(d.detach()) < 0.0 else 1.0 - tau) * d * d
        li.backward()
        g = _flat_grads(params)
        want = g * g if want is None else want + g * g
    want = want / n
    got = _flat([fw for fw, _ in fisher_np(ex, n, exact=True)], [fb for _, fb in fisher_np(ex, n, exact=True)]) / n
    got32 = _flat([fw for fw, _ in fisher_np(lo, n, exact=False)], [fb for _, fb in fisher_np(lo, n, exact=False)])
    assert got32.dtype == np.float32
    top = float(np.max(want))
    assert top > 0.0 and np.max(np.abs(got - want)) <= 1e-10 * top
    assert np.max(np.abs(got32.astype(np.float64) / n - want)) <= 1e-4 * top
    # at n = 1 the per-sample form IS the square of the batch's gradient, the reference's; beyond it is not
    one = value_grad_np(layers, x[:1], ret[:1], exact=True, activation="tanh")
    sq = _flat([gw * gw for gw, _ in one["grads"]], [gb * gb for _, gb in one["grads"]])
    f1 = _flat([fw for fw, _ in fisher_np(one, 1, exact=True)], [fb for _, fb in fisher_np(one, 1, exact=True)])
    assert np.allclose(f1, sq, rtol=1e-12, atol=0.0)
    with pytest.raises(ValueError):
        fisher_np(lo, n, exact=True)


def _tasks(K, P_, seed):
    rng = np.random.default_rng(seed)
    Fs = [np.abs(rng.normal(0.0, 1.0, P_)).astype(np.float32) * np.float32(10.0 ** rng.integers(-3, 3)) for _ in range(K)]
    ps = [rng.normal(0.0, 1.0, P_).astype(np.float32) for _ in range(K)]
    return Fs, ps, rng.normal(0.0, 1.0, P_)


@pytest.mark.parametrize("K", [2, 3])
@pytest.mark.parametrize("decay", [1.0, 0.9])
def test_the_centre_form_has_the_gradient_of_the_sum_over_tasks(K, decay):
    Fs, ps, p = _tasks(K, 501, 10 * K)
    A = c = None
    A32 = c32 = None
    for F, w in zip(Fs, ps):
        A, c = ewc_merge_np(A, c, F, w, decay, exact=True)
        A32, c32 = ewc_merge_np(A32, c32, F, w, decay)
    assert A.dtype == np.float64 and A32.dtype == np.float32 and c32.dtype == np.float32
    weights = [decay ** (K - 1 - k) for k in range(K)]                                # online EWC: older tasks fade
    explicit = sum(wk * F.astype(np.float64) * (p - w.astype(np.float64)) for wk, F, w in zip(weights, Fs, ps))
    size = sum(wk * F.astype(np.float64) * np.abs(p - w.astype(np.float64)) for wk, F, w in zip(weights, Fs, ps))
    assert np.all(np.abs(A * (p - c) - explicit) <= 1e-12 * size)
    assert np.allclose(A, sum(wk * F.astype(np.float64) for wk, F in zip(weights, Fs)), rtol=1e-14, atol=0.0)
    # the penalty value differs from the sum over tasks by a constant in p
    value = lambda q: 0.5 * np.sum(A * (q - c) ** 2) - 0.5 * sum(np.sum(wk * F.astype(np.float64) * (q - w.astype(np.float64)) ** 2) for wk, F, w in zip(weights, Fs, ps))
    q = p + np.random.default_rng(5).normal(0.0, 1.0, p.shape)
    assert abs(value(p) - value(q)) <= 1e-10 * (abs(value(p)) + np.sum(size))
    # the float32 form: the first merge exact, later ones within float32 roundings of the exact recursion
    assert np.all(np.abs(A32.astype(np.float64) - A) <= K * U32 * A)
    assert np.max(np.abs(c32.astype(np.float64) - c)) <= 8.0 * K * U32 * max(float(np.max(np.abs(w))) for w in ps)


def test_the_first_merge_is_the_task_and_an_empty_importance_keeps_the_optimum():
    F = np.array([0.5, 2.0, 0.0], dtype=np.float32)
    w = np.array([1.0, -3.0, 7.0], dtype=np.float32)
    A, c = ewc_merge_np(None, None, F, w)
    assert np.array_equal(A, F) and np.array_equal(c, w)
    A2, c2 = ewc_merge_np(A, c, np.array([0.5, 0.0, 0.0], dtype=np.float32), np.array([3.0, 9.0, 9.0], dtype=np.float32), 1.0)
    assert np.array_equal(A2, np.array([1.0, 2.0, 0.0], dtype=np.float32))
    assert np.array_equal(c2, np.array([2.0, -3.0, 9.0], dtype=np.float32))            # the mean; unchanged; w where A' is 0
    # the clamp of the commit
    Fi = fisher_importance_np(np.array([10.0, 1e-6, 0.0]), 5, 1e-3)
    assert Fi.dtype == np.float32 and np.array_equal(Fi, np.array([2.0, 1e-3, 1e-3], dtype=np.float32))


def test_value_rules_of_the_coefficients():
    ok = lambda **kw: _lib.anchor_check(_lib.anchor_config(**kw))
    assert ok() == (_lib.GS_OK, "") and ok(prox_mu=0.1, ewc_lambda=5000.0) == (_lib.GS_OK, "")
    for kw in (dict(prox_mu=-0.1), dict(ewc_lambda=-1.0), dict(prox_mu=float("nan")), dict(ewc_lambda=float("nan")), dict(prox_mu=float("inf")),
               dict(ewc_lambda=float("inf"))):
        rc, msg = ok(**kw)
        assert rc == _lib.GS_E_INVALID and "finite and >= 0" in msg, (kw, msg)
    rc, msg = ok(struct_size=16)
    assert rc == _lib.GS_E_INVALID and "struct_size" in msg
    rc, msg = _lib.anchor_check(None)
    assert rc == _lib.GS_E_INVALID and "NULL" in msg


def test_symbols_struct_sizes_and_python_surface():
    lib = _lib.load()
    names = {n for n, _, _ in _lib.SYMBOLS}
    for name in ("gs_learner_anchor_check", "gs_learner_anchor_here", "gs_learner_anchor_set", "gs_learner_anchor_get", "gs_learner_fisher_begin",
                 "gs_learner_fisher_accumulate", "gs_learner_fisher_commit", "gs_learner_anchor_clear", "gs_learner_anchor_stats",
                 "gs_learner_anchor_download"):
        assert name in names and hasattr(lib, name), name
    assert ctypes.sizeof(_lib.gs_learner_anchor_config) == 24 and ctypes.sizeof(_lib.gs_fisher_config) == 24
    assert ctypes.sizeof(_lib.gs_learner_anchor_stats_out) == 56
    assert (_lib.GS_ANCHOR_PROX, _lib.GS_ANCHOR_EWC) == (1, 2) and _lib.ANCHOR_SLOTS["both"] == 3
    for name in ("anchor_term_np", "anchor_penalty_terms_np", "fisher_np", "fisher_importance_np", "ewc_merge_np"):
        assert name in P.__all__ and callable(getattr(P, name)), name
    for name in ("anchor_here", "set_anchor", "anchor", "consolidate", "clear_anchor", "anchor_stats", "anchor_arrays"):
        assert callable(getattr(P.DeviceLearner, name)), name
    assert "prox_mu" in inspect.signature(P.FederatedLearners.round).parameters
    assert "prox_mu" in inspect.signature(P.FederatedLearners.aggregate).parameters
    with pytest.raises(ValueError):
        P.FederatedLearners._prox_mu(-1.0)
    assert P.FederatedLearners._prox_mu(None) is None and P.FederatedLearners._prox_mu(0.1) == 0.1
