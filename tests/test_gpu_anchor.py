"""GPU: parameter anchors (include/gridstep.h "parameter anchors") -- FedProx's proximal term and elastic
weight consolidation on the device learners, against the NumPy restatements of grid_fed_rl_gym_amd/learner.py.

Set-up and cases are those of tests/test_gpu_learner.py (the 13-bus feeder, B = 37, T = 5, hidden [64, 64] relu; [40, 40] tanh, a width
that is no multiple of 16; the B = 200, T = 33 collection for n = 513: two full weight-gradient segments and one row) and, for the Q
network, the AWR policy and the pathwise / conservative steps, of tests/test_gpu_q_critics.py (B = 5, T = 37).  Minibatch sizes 1, 33,
185 and 513.  Twin environments are two builds of one case: the same seeds give the same rollout, minibatches and parameters.

Bounds, none of them computed from the device:
  the term, Adam, images,    bit-equal: ``anchor_term_np`` on the twin's gradient, ``adam_np`` on the new gradient with the device's
  off-is-off, the merge      norm, ``ewc_merge_np`` / ``fisher_importance_np`` on the downloaded pending sums and parameters.
  grad_norm                  within P 2^-52 relative of ``math.fsum`` of the squares (tests/test_gpu_learner.py's bound).
  grad_norm_loss             the twin's grad_norm, by bits.
  penalties                  (blocks + 12) 2^-53 relative of ``math.fsum`` of the restated terms: four terms a thread in sequence, a tree
                             of depth eight over 256 threads, the workgroups' sums in sequence, one product.
  the Fisher diagonal        4 E_ref per tensor, E_ref = the largest absolute error of the float32 restatement against the exact one
                             on the same inputs -- the margin tests/test_gpu_learner.py gives gradients, for the same reason: only the
                             summation order differs.  The device's clip / cap flags are fed to both restatements.  A minibatch of ONE
                             row adds its E_ref in that file's ``_single_rows`` manner (32 minibatches of one row each, relative to the
                             exact tensor's largest entry); a tensor of ONE entry (a critic's last bias) has the floor 2^-24 sum_i of
                             its terms, what rounding the terms to float32 can cost any evaluation of that sum."""
import ctypes
import math

import numpy as np
import pytest

import grid_fed_rl_gym_amd as P
from grid_fed_rl_gym_amd import _lib
from grid_fed_rl_gym_amd.learner import (adam_np, anchor_penalty_terms_np, anchor_term_np, awr_grad_np, ewc_merge_np, fisher_importance_np,
                                         fisher_np, ppo_grad_np, split_parameters, value_grad_np)

import tests.test_gpu_federated as TF
import tests.test_gpu_learner as TL
import tests.test_gpu_q_critics as TQ

pytestmark = pytest.mark.gpu

S, I = _lib.GS_E_STATE, _lib.GS_E_INVALID
HYPER = TL.HYPER                       # (weight decay and the norm clip both on; tests/test_gpu_q_critics.py's are the same)
CLIP, ENT = TL.CLIP, TL.ENT
AWR = dict(temperature=1.0, weight_max=20.0)
MU, LAM = 0.1, 50.0
U = 2.0 ** -53
WORST = {}
EWC_ARRAYS = ("ewc_importance", "ewc_centre", "fisher_pending")      # (a learner without a PROX centre is refused the fourth)

_CASES = {}


def _case(kind, name, twin=0):
    """case ``name`` of tests/test_gpu_learner.py (kind "L") or tests/test_gpu_q_critics.py ("Q"); ``twin``: another build of it"""
    key = (kind, name, twin)
    if key not in _CASES:
        _CASES[key] = (TL if kind == "L" else TQ)._build(name)
    return _CASES[key]


@pytest.fixture(scope="module", autouse=True)
def _cleanup():
    yield
    for c in _CASES.values():
        c["env"].close()
    _CASES.clear()
    for envs in TF._POOL.values():
        for e in envs:
            e.close()
    TF._POOL.clear()
    print("largest device error / E_ref:", {k: round(v, 3) for k, v in WORST.items()})


def _fresh(kind, c, loss="default"):
    """the networks as first installed (every learner and anchor of the handle ends), then a learner for the case's trainable nets"""
    env = c["env"]
    if kind == "L":
        TL._install(c)
        return P.DeviceLearner(env, nets=("policy", "value"), **HYPER)
    TQ._install(c)
    TQ._evaluate(env)
    if loss == "awr":
        return P.DeviceLearner(env, nets=("policy",), policy_loss="awr", **AWR, **HYPER)
    return P.DeviceLearner(env, nets=("q1", "q2"), **HYPER)


def _step(learner, net, batch, n):
    learner.env.handle.learner_step(net, batch, n)


def _bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.uint32 if x.dtype == np.float32 else np.uint64 if x.dtype == np.float64 else x.dtype)


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _record(learner, net):
    """everything a call that must change nothing could change: the four arrays, the statistics, the step count"""
    out = dict(learner.download(net))
    out["stats"] = np.array([learner.stats(net)[k] for k in _lib.LEARNER_STATS], dtype=np.float64)
    out["step"] = np.array([learner.info(net)["step"]], dtype=np.int64)
    return out


def _equal_records(a, b):
    return [k for k in a if not _same(a[k], b[k])]


def _image(c, net):
    """the installed image of ``net`` as master parameters: what a learner created now snapshots (ends the learner that was there)"""
    return P.DeviceLearner(c["env"], nets=(net,), **HYPER).download(net, ("params",))["params"]


# ---- 1. off is off -----------------------------------------------------------------------------------------------------------------

def test_with_both_coefficients_zero_nothing_differs():
    c1, c2 = _case("L", "ieee13-relu"), _case("L", "ieee13-relu", 1)
    L1, L2 = _fresh("L", c1), _fresh("L", c2)
    h1, h2 = c1["env"].handle, c2["env"].handle
    for net in ("policy", "value"):
        L2.anchor_here(net)
        assert L2.consolidate(net, [h2.onpolicy_batch(5, 0, 0, 33)]) == 33
        assert L2.anchor(net) == dict(prox_mu=0.0, ewc_lambda=0.0)
    for s in range(2):
        L1.step(h1.onpolicy_batch(5, s, 0, 185))
        L2.step(h2.onpolicy_batch(5, s, 0, 185))
    for net in ("policy", "value"):
        assert _equal_records(_record(L1, net), _record(L2, net)) == [], net
        TL._refused(lambda: L2.anchor_stats(net), S, "no step with a non-zero coefficient")
    for c in (c1, c2):
        c["env"].reset(seed=21)
    assert _same(c1["env"].policy_actions(seed=9, t=2), c2["env"].policy_actions(seed=9, t=2))      # the policy image
    assert _same(_image(c1, "policy"), _image(c2, "policy")) and _same(_image(c1, "value"), _image(c2, "value"))


# ---- 2. the term, bit for bit --------------------------------------------------------------------------------------------------------

def _check_term_step(tag, L1, L2, net, before, arrays, mu, lam, t, clip_engaged=False):
    """a step that has just run on both twins from the state ``before`` (the second twin's, equal to the first's), the second under
    (mu, lam) on the slots ``arrays``; t: Adam's step number"""
    g1 = L1.download(net, ("grads",))["grads"]
    after = L2.download(net)
    want = anchor_term_np(g1, before["params"], prox=arrays.get("prox"), mu=mu, importance=arrays.get("ewc_importance"),
                          centre=arrays.get("ewc_centre"), lam=lam)
    assert _same(after["grads"], want), tag
    assert not _same(after["grads"], g1), tag                                    # the terms are there at all
    st1, st2, an = L1.stats(net), L2.stats(net), L2.anchor_stats(net)
    assert _same(np.float64(an["grad_norm_loss"]), np.float64(st1["grad_norm"])), (tag, an["grad_norm_loss"], st1["grad_norm"])
    assert an["prox_mu"] == mu and an["ewc_lambda"] == lam
    g2 = after["grads"]
    norm = math.sqrt(math.fsum(float(x) * float(x) for x in g2))
    assert abs(st2["grad_norm"] - norm) <= g2.size * 2.0 ** -52 * norm, (tag, st2["grad_norm"], norm)
    assert HYPER["max_grad_norm"] > 0.0                                              # Adam's clip is on, and scales by the TOTAL gradient's norm
    if clip_engaged:
        assert st2["grad_norm"] > HYPER["max_grad_norm"]
    p, m, v = adam_np(before["params"], g2, before["m"], before["v"], t, HYPER, st2["grad_norm"])
    assert _same(after["params"], p) and _same(after["m"], m) and _same(after["v"], v), tag
    blocks = -(-g2.size // 1024)
    tp, te = anchor_penalty_terms_np(before["params"], arrays.get("prox"), arrays.get("ewc_importance"), arrays.get("ewc_centre"))
    for what, terms, coef in (("penalty_prox", tp, mu), ("penalty_ewc", te, lam)):
        if coef == 0.0:
            assert an[what] == 0.0
            continue
        ref = coef / 2.0 * math.fsum(terms)
        print(f"{tag} {what}: device {an[what]:.17g} fsum {ref:.17g}")
        assert ref > 0.0 and abs(an[what] - ref) <= (blocks + 12) * U * ref, (tag, what, an[what], ref)
    return after


TERM = [("L", "ieee13-relu", "policy", "default", 185), ("L", "ieee13-relu", "value", "default", 33), ("L", "ieee13-tanh40", "policy", "default", 1),
        ("L", "ieee13-segments", "value", "default", 513), ("Q", "ieee13-relu", "policy", "awr", 185), ("Q", "ieee13-relu", "q1", "default", 33)]


@pytest.mark.parametrize("kind,name,net,loss,n", TERM, ids=[f"{k}-{a}-{b}-{l}-n{n}" for k, a, b, l, n in TERM])
def test_the_terms_on_the_gradient_bit_for_bit(kind, name, net, loss, n):
    c1, c2 = _case(kind, name), _case(kind, name, 1)
    L1, L2 = _fresh(kind, c1, loss), _fresh(kind, c2, loss)
    h1, h2 = c1["env"].handle, c2["env"].handle
    tag = f"{name} {net} {loss} n={n}"
    # an anchor and a task placed BEFORE the first step, so that w differs from both centres afterwards
    L2.anchor_here(net)
    L2.consolidate(net, [h2.onpolicy_batch(5, 0, 0, n)])
    _step(L1, net, h1.onpolicy_batch(5, 0, 0, n), n)
    _step(L2, net, h2.onpolicy_batch(5, 0, 0, n), n)
    before = L2.download(net)
    assert _equal_records(L1.download(net), before) == [], tag
    L2.set_anchor(net, prox_mu=MU, ewc_lambda=LAM)
    assert L2.anchor(net) == dict(prox_mu=MU, ewc_lambda=LAM)
    arrays = L2.anchor_arrays(net, ("prox", "ewc_importance", "ewc_centre"))
    assert not _same(arrays["prox"], before["params"]) and _same(arrays["prox"], arrays["ewc_centre"])
    _step(L1, net, h1.onpolicy_batch(5, 1, 0, n), n)
    _step(L2, net, h2.onpolicy_batch(5, 1, 0, n), n)
    after = _check_term_step(tag, L1, L2, net, before, arrays, MU, LAM, 2, clip_engaged=(kind, name, net) == ("L", "ieee13-relu", "policy"))
    an = L2.anchor_stats(net)
    assert an["tasks"] == 1 and an["fisher_samples"] == n
    # the installed image is the parameters
    assert _same(_image(c2, net), after["params"]), tag


@pytest.mark.parametrize("which", ["pathwise", "conservative"])
def test_the_other_steps_get_the_term_from_the_shared_reduction(which):
    cs = _case("Q", "ieee13-relu"), _case("Q", "ieee13-relu", 1)
    net = "policy" if which == "pathwise" else "q1"
    n, pairs = 65, []
    for c in cs:
        TQ._install(c)
        TQ._evaluate(c["env"])
        pl = P.DeviceLearner(c["env"], nets=("policy",), policy_loss="pathwise", alpha=0.2, bc_coef=0.5, pathwise_seed=0x5EED0123456789, **HYPER)
        ql = P.DeviceLearner(c["env"], nets=("q1", "q2"), conservative_weight=5.0, conservative_seed=0x5EED0123456789, **HYPER)
        pairs.append(pl if which == "pathwise" else ql)
    L1, L2 = pairs
    step = (lambda L, b: L.step_pathwise(b)) if which == "pathwise" else (lambda L, b: L.step_conservative(b, "q1"))
    L2.anchor_here(net)
    for L, c in zip(pairs, cs):
        step(L, c["env"].handle.onpolicy_batch(5, 0, 0, n))
    before = L2.download(net)
    assert _equal_records(L1.download(net), before) == []
    L2.set_anchor(net, prox_mu=MU)
    arrays = L2.anchor_arrays(net, ("prox",))
    for L, c in zip(pairs, cs):
        step(L, c["env"].handle.onpolicy_batch(5, 1, 0, n))
    _check_term_step(f"{which} n={n}", L1, L2, net, before, arrays, MU, 0.0, 2)
    with pytest.raises(ValueError):
        L2.consolidate(net, [])                                                  # no per-sample Fisher for these steps


# ---- 3. zero distance --------------------------------------------------------------------------------------------------------------

def test_the_step_right_after_anchor_here_has_the_gradient_of_a_step_without_the_term():
    c1, c2 = _case("L", "ieee13-relu"), _case("L", "ieee13-relu", 1)
    L1, L2 = _fresh("L", c1), _fresh("L", c2)
    h1, h2 = c1["env"].handle, c2["env"].handle
    L2.anchor_here("policy")
    L2.set_anchor("policy", prox_mu=MU)
    _step(L1, "policy", h1.onpolicy_batch(5, 0, 0, 185), 185)
    _step(L2, "policy", h2.onpolicy_batch(5, 0, 0, 185), 185)
    a, b = _record(L1, "policy"), _record(L2, "policy")
    assert _equal_records(a, b) == []
    an = L2.anchor_stats("policy")
    assert an["penalty_prox"] == 0.0 and _same(np.float64(an["grad_norm_loss"]), np.float64(L2.stats("policy")["grad_norm"]))
    before = L2.download("policy")
    arrays = L2.anchor_arrays("policy", ("prox",))
    _step(L1, "policy", h1.onpolicy_batch(5, 1, 0, 185), 185)
    _step(L2, "policy", h2.onpolicy_batch(5, 1, 0, 185), 185)
    _check_term_step("zero distance, next step", L1, L2, "policy", before, arrays, MU, 0.0, 2)


# ---- 4. the Fisher diagonal ----------------------------------------------------------------------------------------------------------

def _restate(kind, c, net, loss, layers, hb, rows, exact, flags, td=None):
    idx = hb["indices"][rows]
    obs = hb["observations"][rows]
    if kind == "L" and net == "policy":
        return ppo_grad_np(layers, obs, c["actions"][idx], c["logp"][idx], hb["advantages"][rows], CLIP, ENT, exact=exact, clipped=flags,
                           activation=c["activation"])
    if kind == "L":
        return value_grad_np(layers, obs, hb["returns"][rows], exact=exact, activation=c["activation"])
    act = c["data"]["actions"].reshape(c["B"] * c["T"], -1)[idx]
    if loss == "awr":
        return awr_grad_np(layers, obs, act, hb["advantages"][rows], AWR["temperature"], AWR["weight_max"], ENT, exact=exact, capped=flags,
                           activation="relu")
    sa = np.concatenate([obs, act.astype(np.float32)], axis=1)
    return value_grad_np(layers, sa, td[idx].astype(np.float32), exact=exact, activation=c["activation"])


def _flags_of(res):
    return res.get("clipped", res.get("capped"))


FISHER = [("L", "ieee13-relu", "policy", "default", (33, 185)), ("L", "ieee13-relu", "value", "default", (1, 33)),
          ("L", "ieee13-tanh40", "policy", "default", (185, 1)), ("L", "ieee13-tanh40", "value", "default", (33, 185)),
          ("L", "ieee13-segments", "policy", "default", (513, 33)), ("L", "ieee13-segments", "value", "default", (1, 513)),
          ("Q", "ieee13-relu", "policy", "awr", (185, 33)), ("Q", "ieee13-relu", "q1", "default", (1, 185))]


@pytest.mark.parametrize("kind,name,net,loss,sizes", FISHER, ids=[f"{k}-{a}-{b}-{l}-n{'+'.join(map(str, s))}" for k, a, b, l, s in FISHER])
def test_the_fisher_diagonal_against_the_restatements_and_nothing_else_moves(kind, name, net, loss, sizes):
    """Observed on the MI355X: the largest device error / E_ref per kind of tensor is printed at the end of the module."""
    c = _case(kind, name)
    learner = _fresh(kind, c, loss)
    env, h = c["env"], c["env"].handle
    tag = f"{name} {net} {loss} n={sizes}"
    td = h.rollout_q_download(("td_target",))["td_target"].reshape(-1) if kind == "Q" else None
    host = TL._host if kind == "L" else TQ._host
    _step(learner, net, h.onpolicy_batch(5, 0, 0, sizes[0]), sizes[0])           # (statistics and a gradient exist; Adam's state is not zero)
    rec0 = _record(learner, net)
    acts0 = env.policy_actions(seed=9, t=2) if net == "policy" else None
    layers = list(zip(*learner.parameters(net)))
    dims = learner.info(net)["dims"]
    L = len(layers)
    ex_sum, lo_sum = [[0.0, 0.0] for _ in range(L)], [[0.0, 0.0] for _ in range(L)]
    single, floor = [[0.0, 0.0] for _ in range(L)], 0.0
    h.learner_fisher_begin(net)
    for j, n in enumerate(sizes):
        batch = h.onpolicy_batch(5, 1 + j, 0, n)
        hb = host(batch)
        h.learner_fisher_accumulate(net, batch, n)
        views = learner.views(net)
        flags = views["clipped"].to_host() if views["clipped"] is not None else None
        ex = _restate(kind, c, net, loss, layers, hb, slice(None), True, flags, td)
        lo = _restate(kind, c, net, loss, layers, hb, slice(None), False, flags, td)
        fex, flo = fisher_np(ex, n, exact=True), fisher_np(lo, n, exact=False)
        floor += 2.0 ** -24 * math.fsum(((n * ex["passes"]["deltas"][-1]) ** 2).reshape(-1))
        rel = {}
        if n < 32:                                                               # tests/test_gpu_learner.py's _single_rows, for the Fisher
            hb32 = host(h.onpolicy_batch(5, 1 + j, 0, 32))
            assert hb32["indices"][0] == hb["indices"][0]
            for r in range(32):
                e1 = _restate(kind, c, net, loss, layers, hb32, slice(r, r + 1), True, None, td)
                l1 = _restate(kind, c, net, loss, layers, hb32, slice(r, r + 1), False, _flags_of(e1), td)
                for l, (fe, fl) in enumerate(zip(fisher_np(e1, 1, exact=True), fisher_np(l1, 1, exact=False))):
                    for k in range(2):
                        top = float(np.max(np.abs(fe[k])))
                        if top > 0.0:
                            rel[(l, k)] = max(rel.get((l, k), 0.0), TL._err(fl[k], fe[k]) / top)
        for l in range(L):
            for k in range(2):
                ex_sum[l][k] = ex_sum[l][k] + fex[l][k]
                lo_sum[l][k] = lo_sum[l][k] + flo[l][k].astype(np.float64)         # (the device widens every minibatch's float32 sums)
                if n < 32:
                    single[l][k] += rel.get((l, k), 0.0) * float(np.max(np.abs(fex[l][k])))
    samples = sum(sizes)
    h.learner_fisher_commit(net, _lib.fisher_config(1e-3, 1.0))
    pending = learner.anchor_arrays(net, ("fisher_pending",))["fisher_pending"]
    dW, db = split_parameters(pending, dims)
    missed = []
    for l in range(L):
        for k, what, dev in ((0, f"FW[{l}]", dW[l]), (1, f"Fb[{l}]", db[l])):
            exact = ex_sum[l][k] / samples
            e_ref = (TL._err(lo_sum[l][k], ex_sum[l][k]) + single[l][k]) / samples
            if exact.size == 1:
                e_ref = max(e_ref, floor / samples)
            e_dev = TL._err(dev / samples, exact)
            ratio = e_dev / e_ref if e_ref > 0.0 else (0.0 if e_dev == 0.0 else math.inf)
            print(f"{tag} {what}: E_ref {e_ref:.3e} device {e_dev:.3e} ratio {ratio:.2f} largest {float(np.max(np.abs(exact))):.3e}")
            WORST[what.split("[")[0]] = max(WORST.get(what.split("[")[0], 0.0), ratio if math.isfinite(ratio) else 1e9)
            if not e_dev <= 4.0 * e_ref:                                         # (every tensor is looked at before the test fails)
                missed.append((what, e_dev, e_ref))
    assert float(np.max(pending)) > 0.0 and float(np.min(pending)) >= 0.0
    assert not missed, (tag, missed)
    # nothing of the learner moved
    assert _equal_records(rec0, _record(learner, net)) == [], tag
    if net == "policy":
        assert _same(acts0, env.policy_actions(seed=9, t=2))
    an = learner.anchor_arrays(net, ("ewc_centre",))
    assert _same(an["ewc_centre"], rec0["params"])


# ---- 5. commit and merge -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("net", ["policy", "value"])
def test_commits_merge_as_ewc_merge_np_bit_for_bit(net):
    c = _case("L", "ieee13-relu")
    learner = _fresh("L", c)
    h = c["env"].handle
    f = np.float32
    # task 1 through the entries: the clamp placed at the median of the positive means, so that it is active and inactive
    h.learner_fisher_begin(net)
    h.learner_fisher_accumulate(net, h.onpolicy_batch(5, 0, 0, 185), 185)
    raw = (learner.anchor_arrays(net, ("fisher_pending",))["fisher_pending"] / 185.0).astype(f)
    m1 = float(np.median(raw[raw > 0.0]))
    h.learner_fisher_commit(net, _lib.fisher_config(m1, 1.0))
    w1 = learner.download(net, ("params",))["params"]
    arr = learner.anchor_arrays(net, EWC_ARRAYS)
    F1 = fisher_importance_np(arr["fisher_pending"], 185, m1)
    assert (raw < f(m1)).any() and (raw > f(m1)).any()                               # the clamp is active on some entries, inactive on others
    assert (F1 == f(m1)).any() and (F1 > f(m1)).any() and float(F1.min()) == float(f(m1))
    A, ctr = ewc_merge_np(None, None, F1, w1)
    assert _same(arr["ewc_importance"], A) and _same(arr["ewc_centre"], ctr) and _same(ctr, w1)
    # steps in between, pulled back by the first task
    learner.set_anchor(net, ewc_lambda=LAM)
    for s in range(2):
        _step(learner, net, h.onpolicy_batch(5, s, 0, 185), 185)
    an = learner.anchor_stats(net)
    assert an["tasks"] == 1 and an["fisher_samples"] == 185 and an["penalty_ewc"] > 0.0 and an["penalty_prox"] == 0.0
    # task 2 through consolidate: two minibatches of different size, the sum over tasks
    assert learner.consolidate(net, (h.onpolicy_batch(5, 3 + j, 0, n) for j, n in enumerate((33, 65))), min_importance=m1, decay=1.0) == 98
    w2 = learner.download(net, ("params",))["params"]
    arr2 = learner.anchor_arrays(net, EWC_ARRAYS)
    assert not _same(w2, w1) and not _same(arr2["fisher_pending"], arr["fisher_pending"])
    A2, c2 = ewc_merge_np(A, ctr, fisher_importance_np(arr2["fisher_pending"], 98, m1), w2, 1.0)
    assert _same(arr2["ewc_importance"], A2) and _same(arr2["ewc_centre"], c2)
    assert (A2 >= A).all() and (A2 > A).any() and not _same(c2, w2) and not _same(c2, ctr)
    # a decayed third (online EWC), the clamp off
    _step(learner, net, h.onpolicy_batch(5, 2, 0, 185), 185)
    assert learner.consolidate(net, [h.onpolicy_batch(5, 5, 0, 185)], min_importance=0.0, decay=0.9) == 185
    w3 = learner.download(net, ("params",))["params"]
    arr3 = learner.anchor_arrays(net, EWC_ARRAYS)
    F3 = fisher_importance_np(arr3["fisher_pending"], 185, 0.0)
    A3, c3 = ewc_merge_np(A2, c2, F3, w3, 0.9)
    assert _same(arr3["ewc_importance"], A3) and _same(arr3["ewc_centre"], c3)
    _step(learner, net, h.onpolicy_batch(5, 3, 0, 185), 185)
    assert learner.anchor_stats(net)["tasks"] == 3
    # clearing the slot turns the term off and forgets the tasks
    learner.clear_anchor(net, "ewc")
    assert learner.anchor(net)["ewc_lambda"] == 0.0
    TL._refused(lambda: learner.anchor_arrays(net, ("ewc_importance",)), S, "no task has been committed")
    TL._refused(lambda: h.learner_anchor_set(net, _lib.anchor_config(0.0, 1.0)), S, "no task has been committed")


# ---- 6. the federation ---------------------------------------------------------------------------------------------------------------

def test_a_round_with_prox_mu_anchors_every_client_at_the_global_model():
    envs = TF._envs("ieee13", 6)
    feds = [TF._scatter("h64", 3, nets=("policy", "value"), envs=envs[:3]), TF._scatter("h64", 3, nets=("policy", "value"), envs=envs[3:])]      # twins: the second never hears of prox_mu
    try:
        for c in feds:
            c["fed"].set_global("policy")
            for k, (e, l) in enumerate(zip(c["envs"], c["learners"])):
                TF._collect(e, c["installed"][0]["policy"], k)
                for s in range(2):
                    l.step(e.handle.onpolicy_batch(5, s, 0, 33))
        feds[0]["fed"].round(prox_mu=MU)
        feds[1]["fed"].round()
        g = feds[0]["fed"].global_parameters("policy")
        assert _same(g, feds[1]["fed"].global_parameters("policy"))
        for l, twin in zip(feds[0]["learners"], feds[1]["learners"]):
            assert _same(l.anchor_arrays("policy", ("prox",))["prox"], g) and _same(l.download("policy", ("params",))["params"], g)
            assert l.anchor("policy") == dict(prox_mu=MU, ewc_lambda=0.0)
            assert twin.anchor("policy") == dict(prox_mu=0.0, ewc_lambda=0.0)
            TL._refused(lambda: twin.anchor_arrays("policy", ("prox",)), S, "no PROX centre")
        # the first local step: a zero distance, the twin's gradient by bits; the next one is pulled back
        for s in (2, 3):
            for c in feds:
                for e, l in zip(c["envs"], c["learners"]):
                    l.step(e.handle.onpolicy_batch(5, s, 0, 33))
            for l, twin in zip(feds[0]["learners"], feds[1]["learners"]):
                same = _same(l.download("policy", ("grads",))["grads"], twin.download("policy", ("grads",))["grads"])
                assert same == (s == 2), s
        # a round without prox_mu leaves the anchors alone: the centre stays the OLD global model
        feds[0]["fed"].round()
        g2 = feds[0]["fed"].global_parameters("policy")
        assert not _same(g2, g)
        for l in feds[0]["learners"]:
            assert _same(l.anchor_arrays("policy", ("prox",))["prox"], g) and l.anchor("policy")["prox_mu"] == MU
    finally:
        for c in feds:
            c["fed"].close()


# ---- 7. the rules ----------------------------------------------------------------------------------------------------------------------

def test_every_refusal_comes_before_any_launch_and_create_and_install_drop_the_anchors():
    c = _case("L", "ieee13-relu")
    learner = _fresh("L", c)
    env, h = c["env"], c["env"].handle
    lib, hh = h._lib, h._h
    batch = h.onpolicy_batch(5, 0, 0, 185)
    learner.step(batch)
    rec = {net: _record(learner, net) for net in ("policy", "value")}
    cfg, fcfg = _lib.anchor_config(0.0, 0.0), _lib.fisher_config()
    bstruct = _lib.gs_onpolicy_batch_out()
    stats, out = _lib.gs_learner_anchor_stats_out(), _lib.gs_learner_anchor_config()
    raw = lambda rc: h._check(rc)
    without = lambda *keys: {k: v for k, v in batch.items() if k not in keys}
    nan, inf = float("nan"), float("inf")
    refusals = [
        # an unknown net, entry by entry
        (lambda: raw(lib.gs_learner_anchor_here(hh, 7, None)), I, "unknown net"),
        (lambda: raw(lib.gs_learner_anchor_set(hh, -1, ctypes.byref(cfg))), I, "unknown net"),
        (lambda: raw(lib.gs_learner_anchor_get(hh, 7, ctypes.byref(out))), I, "unknown net"),
        (lambda: raw(lib.gs_learner_fisher_begin(hh, 7)), I, "unknown net"),
        (lambda: raw(lib.gs_learner_fisher_accumulate(hh, 7, ctypes.byref(bstruct), 185, None)), I, "unknown net"),
        (lambda: raw(lib.gs_learner_fisher_commit(hh, 7, ctypes.byref(fcfg))), I, "unknown net"),
        (lambda: raw(lib.gs_learner_anchor_clear(hh, 7, 3)), I, "unknown net"),
        (lambda: raw(lib.gs_learner_anchor_stats(hh, 7, ctypes.byref(stats))), I, "unknown net"),
        (lambda: raw(lib.gs_learner_anchor_download(hh, 7, None, None, None, None)), I, "unknown net"),
        # a net without a learner
        (lambda: h.learner_anchor_here("thermal"), S, "no learner"),
        (lambda: h.learner_anchor_set("thermal", cfg), S, "no learner"),
        (lambda: h.learner_fisher_begin("thermal"), S, "no learner"),
        (lambda: h.learner_fisher_accumulate("thermal", batch, 185), S, "no learner"),
        # the coefficients
        (lambda: h.learner_anchor_set("policy", _lib.anchor_config(nan, 0.0)), I, "finite and >= 0"),
        (lambda: h.learner_anchor_set("policy", _lib.anchor_config(-0.1, 0.0)), I, "finite and >= 0"),
        (lambda: h.learner_anchor_set("policy", _lib.anchor_config(inf, 0.0)), I, "finite and >= 0"),
        (lambda: h.learner_anchor_set("policy", _lib.anchor_config(0.0, nan)), I, "finite and >= 0"),
        (lambda: h.learner_anchor_set("policy", _lib.anchor_config(0.0, -1.0)), I, "finite and >= 0"),
        (lambda: h.learner_anchor_set("policy", _lib.anchor_config(0.0, inf)), I, "finite and >= 0"),
        (lambda: h.learner_anchor_set("policy", _lib.anchor_config(struct_size=16)), I, "struct_size"),
        (lambda: h.learner_anchor_set("policy", _lib.anchor_config(MU, 0.0)), S, "no PROX centre"),
        (lambda: h.learner_anchor_set("policy", _lib.anchor_config(0.0, LAM)), S, "no task has been committed"),
        # the task
        (lambda: h.learner_fisher_accumulate("policy", batch, 185), S, "no task is open"),
        (lambda: h.learner_fisher_commit("policy", fcfg), S, "no task is open"),
        (lambda: h.learner_anchor_stats("policy"), S, "no step with a non-zero coefficient"),
        (lambda: h.learner_anchor_download("policy", ("prox",)), S, "no PROX centre"),
        (lambda: h.learner_anchor_download("policy", ("ewc_centre",)), S, "no task has been committed"),
        (lambda: h.learner_anchor_download("policy", ("fisher_pending",)), S, "no pending Fisher sum"),
        (lambda: h.learner_anchor_clear("policy", 0), I, "which = 0"),
        (lambda: h.learner_anchor_clear("policy", 4), I, "which = 4"),
    ]
    for call, code, text in refusals:
        TL._refused(call, code, text)
    h.learner_fisher_begin("policy")
    open_task = [
        (lambda: h.learner_fisher_commit("policy", fcfg), S, "holds no samples"),
        (lambda: h.learner_fisher_accumulate("policy", without("observations"), 185), I, "observations"),
        (lambda: h.learner_fisher_accumulate("policy", without("advantages"), 185), I, "advantages"),
        (lambda: h.learner_fisher_accumulate("policy", without("indices"), 185), I, "indices"),
        (lambda: h.learner_fisher_accumulate("policy", batch, 0), I, "n = 0"),
        (lambda: h.learner_fisher_accumulate("value", batch, 185), S, "no task is open"),
        (lambda: h.learner_fisher_commit("policy", _lib.fisher_config(struct_size=16)), I, "struct_size"),
        (lambda: h.learner_fisher_commit("policy", _lib.fisher_config(-1.0, 1.0)), I, "min_importance"),
        (lambda: h.learner_fisher_commit("policy", _lib.fisher_config(nan, 1.0)), I, "min_importance"),
        (lambda: h.learner_fisher_commit("policy", _lib.fisher_config(1e-3, 0.0)), I, "decay"),
        (lambda: h.learner_fisher_commit("policy", _lib.fisher_config(1e-3, 1.5)), I, "decay"),
        (lambda: h.learner_fisher_commit("policy", _lib.fisher_config(1e-3, nan)), I, "decay"),
    ]
    for call, code, text in open_task:
        TL._refused(call, code, text)
    assert not learner.anchor_arrays("policy", ("fisher_pending",))["fisher_pending"].any()      # nothing was accumulated
    for net in ("policy", "value"):
        assert _equal_records(rec[net], _record(learner, net)) == [], net
    # gs_learner_create drops the anchors ...
    learner.anchor_here("policy")
    assert learner.consolidate("policy", [h.onpolicy_batch(5, 1, 0, 33)]) == 33
    learner.set_anchor("policy", prox_mu=MU, ewc_lambda=LAM)
    again = P.DeviceLearner(env, nets=("policy", "value"), **HYPER)
    assert again.anchor("policy") == dict(prox_mu=0.0, ewc_lambda=0.0)
    TL._refused(lambda: again.anchor_arrays("policy", ("prox",)), S, "no PROX centre")
    TL._refused(lambda: again.anchor_arrays("policy", ("ewc_importance",)), S, "no task has been committed")
    TL._refused(lambda: again.set_anchor("policy", prox_mu=MU), S, "no PROX centre")
    # ... and so does installing the network again
    again.anchor_here("policy")
    again.set_anchor("policy", prox_mu=MU)
    env.set_policy(c["pol"], stochastic=True)
    TL._refused(lambda: h.learner_anchor_get("policy"), S, "no learner")
    TL._refused(lambda: h.learner_anchor_download("policy", ("prox",)), S, "no learner")
    assert again.anchor("value") == dict(prox_mu=0.0, ewc_lambda=0.0)                # the value network's learner lives on
