"""GPU: the federation (include/gridstep.h "the federation") -- ``gs_fed_measure`` / ``gs_fed_aggregate`` against
the NumPy restatements of grid_fed_rl_gym_amd/federated.py: the Gram matrix, the round bit for bit, the noise, the refreshed images,
Adam's state across a round, determinism, the refusals, non-interference and the outlier filter.

Set-up as tests/test_gpu_learner.py: the 13-bus feeder, B = 8, ``episode_length`` 7, the normalisation from a short random rollout.
Clients get DIFFERENT parameters by installing networks drawn from different seeds before their learners are created: client k holds
base + 0.01 k noise_k, so client 0 is the global model (create snapshots it; an update of norm 0) and the norms grow with k.

Shapes (name: feeder, network, hidden widths, activation):
  one      obs_dim -> 2 A: ONE layer, no transposed image, P < 1024: one ragged block of the reductions
  h64      -> 64 -> 64 ->: several blocks, the last one ragged
  tanh40   -> 40 -> 40 -> with tanh: padding inside every tile
  four     four layers
  critic   a value network, last width 1 (net 1: another Philox counter)
  ieee123  the 123-bus feeder, -> 256 -> 256 ->, K = 2
No reachable shape gives more than 1024 blocks (P <= ~3.1e5 at the widest network the library installs, 303 blocks): the second lap of
the ONE-workgroup sum over the blocks' sums (thread t taking block t + 1024) cannot be exercised, and no shape is invented for it.

Bounds, none of them computed from the device:
  Gram        |G_ik - fsum| <= (P + 2) 2^-53 sum_j |d_i[j] d_k[j]|, fsum over the EXACT products (Dekker's two-product in float64) of
              the float64 differences d = p - g.  The differences themselves are rounded only where the exponents of p and g lie 29 or
              more apart, each by 2^-53 relative: inside the bound's two extra units.
  rounds      noise off: bit-equal to ``fedavg_np`` on the downloaded inputs and the device's reported norms.  Noise on: within one
              float32 ulp, at least 99.9 % bit-equal (the draw agrees with NumPy's to ~1e-13 relative, the figure
              tests/test_gpu_policy_tiling.py pins; only a rounding boundary can differ); the CPU check that ``fedavg_np`` under
              z (1 +- 1e-13) stays inside that cap runs on the test's own inputs.
  noise       g' - (the noise-off result) has mean within 5 noise_std / sqrt(P) of 0 and a standard deviation within
              5 noise_std / sqrt(2 P) of noise_std (float32 rounding of g' adds ~1e-8 to a noise_std of 0.01).
  everything else bit-equal."""
import ctypes
import math

import numpy as np
import pytest

import grid_fed_rl_gym_amd as P
from grid_fed_rl_gym_amd import _lib
from grid_fed_rl_gym_amd.components import PowerFlowError
from grid_fed_rl_gym_amd.federated import fedavg_np, filter_outliers_np
from grid_fed_rl_gym_amd.learner import adam_np, split_parameters
from grid_fed_rl_gym_amd.rollout import OnPolicyBatches, rollout_device

pytestmark = pytest.mark.gpu

FEEDERS = {"ieee13": lambda: P.ieee13_like("epsilon"), "ieee123": P.ieee123_like}
SHAPES = {
    "one": ("ieee13", "policy", [], "relu"),
    "h64": ("ieee13", "policy", [64, 64], "relu"),
    "tanh40": ("ieee13", "policy", [40, 40], "tanh"),
    "four": ("ieee13", "policy", [48, 32, 24], "elu"),
    "critic": ("ieee13", "value", [64, 64], "relu"),
    "ieee123": ("ieee123", "policy", [256, 256], "relu"),
}
B = 8
HYPER = dict(lr=3e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-5, clip=0.2, ent_coef=0.01, max_grad_norm=0.5)
S, I = _lib.GS_E_STATE, _lib.GS_E_INVALID
U = 2.0 ** -53


def _env(feeder):
    fs = FEEDERS[feeder]()
    return P.BatchedGridEnvironment(fs, num_envs=B, solver="fbs", stochastic_loads=True, weather_variation=True, jacobian="exact", tolerance=1e-9,
                                    max_iterations=100, power_base=fs.base_power_va, episode_length=7)


_NORM, _POOL = {}, {}


def _normalisation(feeder):
    if feeder not in _NORM:
        env = _env(feeder)
        obs = P.collect_random_data(env, 4, seed=11)["observations"]
        env.close()
        mean, std = obs.mean(axis=0), obs.std(axis=0)
        constant = std <= 1e-12 * np.maximum(1.0, np.abs(mean))
        _NORM[feeder] = (mean, np.where(constant, 1.0, std + 1e-6))
    return _NORM[feeder]


@pytest.fixture(scope="module", autouse=True)
def _pool():
    yield
    for envs in _POOL.values():
        for e in envs:
            e.close()
    _POOL.clear()


def _envs(feeder, K):
    pool = _POOL.setdefault(feeder, [])
    while len(pool) < K:
        pool.append(_env(feeder))
    return pool[:K]


def _layers(dims, k, seed0):
    """client k's layers: base + 0.01 k noise_k (client 0 is the base: what the federation snapshots as the global model)"""
    rng = np.random.default_rng(seed0)
    ws = [rng.normal(0.0, 1.0 / math.sqrt(dims[l]), (dims[l + 1], dims[l])) for l in range(len(dims) - 1)]
    bs = [rng.normal(0.0, 0.1, dims[l + 1]) for l in range(len(dims) - 1)]
    if k:
        rk = np.random.default_rng(seed0 + 1000 + k)
        ws = [w + 0.01 * k * rk.normal(size=w.shape) for w in ws]
        bs = [b + 0.01 * k * rk.normal(size=b.shape) for b in bs]
    return ws, bs


def _policy(feeder, ws, bs, activation):
    mean, std = _normalisation(feeder)
    return P.MLPPolicy(ws, bs, activation=activation, head="gaussian_tanh", obs_mean=mean, obs_std=std, compute="float32")


def _value(feeder, ws, bs, activation):
    mean, std = _normalisation(feeder)
    return P.MLPValue(ws, bs, activation=activation, obs_mean=mean, obs_std=std)


def _install(env, feeder, hidden, activation, k, nets, seed0):
    nets_built = {}
    if "policy" in nets:
        ws, bs = _layers([env.obs_dim] + hidden + [2 * env.action_dim], k, seed0)
        nets_built["policy"] = _policy(feeder, ws, bs, activation)
        env.set_policy(nets_built["policy"], stochastic=True)
    if "value" in nets:
        ws, bs = _layers([env.obs_dim] + hidden + [1], k, seed0 + 7)
        nets_built["value"] = _value(feeder, ws, bs, activation)
        env.set_value(nets_built["value"])
    return nets_built


def _scatter(shape, K, nets=None, seed0=100, envs=None, federate=True):
    """K clients of `shape` with freshly installed, different networks, their learners and (federate) their federation"""
    feeder, net, hidden, activation = SHAPES[shape]
    nets = (net,) if nets is None else tuple(nets)
    envs = _envs(feeder, K) if envs is None else envs
    installed = [_install(e, feeder, hidden, activation, k, nets, seed0) for k, e in enumerate(envs)]
    learners = [P.DeviceLearner(e, nets=nets, **HYPER) for e in envs]
    fed = P.FederatedLearners(learners) if federate else None
    return dict(envs=envs, learners=learners, fed=fed, nets=nets, feeder=feeder, hidden=hidden, activation=activation, installed=installed, K=K)


def _params(c, net):
    return [l.download(net, ("params",))["params"] for l in c["learners"]]


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _two_product_sum(a, b):
    """fsum of the exact products a[j] b[j] of float64 vectors (Dekker: a b = p + e exactly), and sum |a b|"""
    split = 134217729.0
    ca, cb = split * a, split * b
    ah, bh = ca - (ca - a), cb - (cb - b)
    al, bl = a - ah, b - bh
    p = a * b
    e = ((ah * bh - p) + ah * bl + al * bh) + al * bl
    return math.fsum(np.concatenate([p, e])), math.fsum(np.abs(p))


# ---- the Gram matrix ----------------------------------------------------------------------------------------------------------------
GRAM = [("one", 3), ("h64", 5), ("tanh40", 2), ("four", 3), ("critic", 3), ("ieee123", 2), ("h64", 1), ("one", 32)]


@pytest.mark.parametrize("shape,K", GRAM, ids=[f"{s}-K{k}" for s, k in GRAM])
def test_gram_matrix_within_the_summation_bound_symmetric_and_its_diagonal_the_rounds_norms(shape, K):
    c = _scatter(shape, K)
    fed, net = c["fed"], c["nets"][0]
    try:
        info = fed.info(net)
        Pn = info["param_count"]
        assert info["n_clients"] == K and info["block_params"] == 1024 and info["rounds"] == 0
        if shape == "one":
            assert Pn < 1024
        else:
            assert Pn > 1024 and Pn % 1024
        g = fed.global_parameters(net)
        ps = _params(c, net)
        assert _same(g, ps[0])
        d = [p.astype(np.float64) - g.astype(np.float64) for p in ps]
        lists = [list(range(K))]
        if K >= 3:
            lists += [[K - 1, 1], [2]]                       # a strict subset, permuted; a single member
            lists += [list(range(K - 1, -1, -1))]            # all of them, permuted
        worst = 0.0
        for part in lists:
            G = fed.measure(net, part)
            assert G.shape == (len(part), len(part)) and _same(G.view(np.float32), G.T.copy().view(np.float32))
            for a, i in enumerate(part):
                for b, k in enumerate(part):
                    if b < a:
                        continue
                    ref, mag = _two_product_sum(d[i], d[k])
                    bound = (Pn + 2) * U * mag
                    assert abs(G[a, b] - ref) <= bound, (shape, part, i, k, G[a, b], ref, bound)
                    if mag:
                        worst = max(worst, abs(G[a, b] - ref) / (U * mag))
        print(f"{shape} K={K} P={Pn}: largest |G - fsum| / (2^-53 sum|d d|) = {worst:.2f} (allowed {Pn + 2})")
        # the same entries whatever the list: the bits of G are a function of the parameters alone
        full = fed.measure(net, lists[0])
        for part in lists[1:]:
            G = fed.measure(net, part)
            assert _same(G.view(np.float32), full[np.ix_(part, part)].copy().view(np.float32))
        # measuring changed nothing, and the next round reports the diagonal's roots
        assert _same(fed.global_parameters(net), g) and all(_same(a, b) for a, b in zip(_params(c, net), ps))
        part = lists[1] if K >= 3 else lists[0]
        fed.aggregate(net, part, [1.0] * len(part), clip_norm=0.5)
        st = fed.stats(net)
        assert st["n"] == len(part) and st["rounds"] == 1
        assert _same(st["norms"].view(np.float32), np.sqrt(np.diag(full)[part]).view(np.float32))
    finally:
        fed.close()


# ---- a round, noise off -------------------------------------------------------------------------------------------------------------
# (shape, K, participants, weights, clip: None = off / "mid" = between the smallest and the largest norm, server_lr)
ROUNDS = [
    ("one", 3, None, None, None, 1.0), ("one", 3, [2, 0], [1.0, 3.0], "mid", 0.5),
    ("h64", 5, None, [5.0, 1.0, 0.0, 33.0, 2.5], "mid", 1.0), ("h64", 5, [4, 1, 2], None, None, 0.5), ("h64", 5, [3], None, "mid", 0.5),
    ("tanh40", 2, None, None, "mid", 0.5), ("four", 3, [2, 1], [1.0, 2.0], "mid", 1.0), ("critic", 3, None, None, "mid", 0.5),
    ("ieee123", 2, None, [3.0, 1.0], "mid", 0.5), ("h64", 1, None, None, None, 1.0), ("one", 32, None, None, "mid", 1.0),
]


def _round_reference(c, net, part, weights, clip, lr):
    """(clip_norm, what fedavg_np makes of the downloaded inputs given the device's norms) -- the norms from a measure, which the
    round must report again bit for bit"""
    fed = c["fed"]
    g, ps = fed.global_parameters(net), _params(c, net)
    norms = np.sqrt(np.diag(fed.measure(net, part)))
    clip_norm = 0.0
    if clip == "mid":
        inner = sorted(set(norms))
        clip_norm = float(0.5 * (inner[0] + inner[-1])) if len(inner) > 1 else float(0.5 * inner[0])
    return g, ps, norms, clip_norm


@pytest.mark.parametrize("shape,K,part,weights,clip,lr", ROUNDS, ids=[f"{r[0]}-K{r[1]}-{i}" for i, r in enumerate(ROUNDS)])
def test_a_round_without_noise_is_fedavg_np_bit_for_bit_in_every_client(shape, K, part, weights, clip, lr):
    c = _scatter(shape, K)
    fed, net = c["fed"], c["nets"][0]
    try:
        part = list(range(K)) if part is None else part
        weights = [1.0] * len(part) if weights is None else weights
        g, ps, norms, clip_norm = _round_reference(c, net, part, weights, clip, lr)
        before = [l.download(net) for l in c["learners"]]
        fed.aggregate(net, part, weights, clip_norm=clip_norm, server_lr=lr, seed=3, round=0)
        st = fed.stats(net)
        assert _same(st["norms"].view(np.float32), norms.view(np.float32))
        if clip == "mid" and len(part) > 1:
            assert (st["clip_scales"] < 1.0).any() and (st["clip_scales"] == 1.0).any()      # norms above and below the clip
        elif clip == "mid":
            assert (st["clip_scales"] < 1.0).all()
        else:
            assert (st["clip_scales"] == 1.0).all()
        W = 0.0
        for x in weights:
            W += x
        for k in range(len(part)):
            ck = min(1.0, clip_norm / (norms[k] + 1e-6)) if clip_norm > 0.0 else 1.0
            assert st["clip_scales"][k] == ck and st["coefficients"][k] == (lr * (weights[k] / W)) * ck
        want = fedavg_np(g, [ps[k] for k in part], weights, norms=st["norms"], clip_norm=clip_norm, server_lr=lr)
        assert not _same(want, g) or len(part) == 1 and part == [0] or K == 1
        assert _same(fed.global_parameters(net), want)
        for k, l in enumerate(c["learners"]):                  # every client, participant or not; Adam's state untouched
            got = l.download(net)
            assert _same(got["params"], want), (shape, k)
            assert _same(got["m"], before[k]["m"]) and _same(got["v"], before[k]["v"]) and l.info(net)["step"] == 0
        if len(part) == 1 and lr == 1.0 and clip is None:
            assert _same(want, ps[part[0]])
    finally:
        fed.close()


def test_the_two_exactness_consequences_on_the_device():
    c = _scatter("h64", 3)
    fed = c["fed"]
    try:
        ps = _params(c, "policy")
        fed.aggregate("policy", [2], [1.0])                    # one participant, weight 1, server_lr 1: a bit-exact copy of client 2
        assert _same(fed.global_parameters("policy"), ps[2]) and all(_same(p, ps[2]) for p in _params(c, "policy"))
        fed.aggregate("policy", [0, 1, 2], [1.0, 5.0, 0.5], clip_norm=0.3, server_lr=0.7, round=1)      # clients all equal to g
        assert _same(fed.global_parameters("policy"), ps[2]) and all(_same(p, ps[2]) for p in _params(c, "policy"))
        assert not fed.stats("policy")["norms"].any()
    finally:
        fed.close()


# ---- a round, noise on --------------------------------------------------------------------------------------------------------------
def _noisy(shape, K, net, seed, rnd, noise_std=0.01):
    c = _scatter(shape, K, nets=("policy", "value"))
    fed = c["fed"]
    try:
        part, weights = list(range(K)), [1.0 + k for k in range(K)]
        g, ps = fed.global_parameters(net), _params(c, net)
        fed.aggregate(net, part, weights, clip_norm=0.05, noise_std=noise_std, seed=seed, round=rnd)
        st = fed.stats(net)
        got = fed.global_parameters(net)
        assert all(_same(p, got) for p in _params(c, net))
        return dict(g=g, ps=ps, weights=weights, norms=st["norms"], got=got, noise_std=st["noise_std"], round=st["round"])
    finally:
        fed.close()


def _ulps(a, b):
    ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    ia, ib = np.where(ia < 0, -(ia & 0x7FFFFFFF), ia), np.where(ib < 0, -(ib & 0x7FFFFFFF), ib)
    return np.abs(ia - ib)


@pytest.mark.parametrize("net", ["policy", "value"])
def test_a_round_with_noise_is_fedavg_np_to_a_rounding_boundary_and_the_noise_is_gaussian(net):
    noise_std, seed, rnd = 0.01, 0x1234567890AB, 5
    r = _noisy("h64", 3, net, seed, rnd, noise_std)
    assert r["noise_std"] == noise_std and r["round"] == rnd
    kw = dict(norms=r["norms"], clip_norm=0.05, server_lr=1.0)
    net_id = _lib.learner_net(net)
    want = fedavg_np(r["g"], r["ps"], r["weights"], noise_std=noise_std, seed=seed, round=rnd, net=net_id, **kw)
    Pn = want.size
    d = _ulps(r["got"], want)
    print(f"{net}: {int(np.count_nonzero(d))} of {Pn} parameters differ from fedavg_np, at most {int(d.max())} ulp")
    assert d.max() <= 1 and np.count_nonzero(d) <= 1e-3 * Pn
    # the CPU check of that cap: the restatement under a draw perturbed by 1e-13 relative, on these inputs
    z = P.fed_noise_np(seed, rnd, net_id, Pn)
    for sign in (1.0, -1.0):
        moved = fedavg_np(r["g"], r["ps"], r["weights"], noise_std=noise_std, z=z * (1.0 + sign * 1e-13), **kw)
        dm = _ulps(moved, want)
        assert dm.max() <= 1 and np.count_nonzero(dm) <= 1e-3 * Pn
    quiet = fedavg_np(r["g"], r["ps"], r["weights"], **kw)
    diff = r["got"].astype(np.float64) - quiet.astype(np.float64)
    mean, std = float(diff.mean()), float(diff.std())
    print(f"{net}: noise mean {mean:.3e} (5 standard errors {5 * noise_std / math.sqrt(Pn):.3e}), std {std:.5e} against {noise_std}")
    assert abs(mean) <= 5.0 * noise_std / math.sqrt(Pn) and abs(std - noise_std) <= 5.0 * noise_std / math.sqrt(2.0 * Pn)
    # the same (seed, round) twice: the same bits; another round number or another network: another draw
    again = _noisy("h64", 3, net, seed, rnd, noise_std)
    assert _same(again["got"], r["got"])
    other = _noisy("h64", 3, net, seed, rnd + 1, noise_std)
    assert np.count_nonzero(_bits(other["got"]) != _bits(r["got"])) > 0.99 * Pn
    zo = P.fed_noise_np(seed, rnd, 1 - net_id, Pn)
    assert np.count_nonzero(np.abs(diff / noise_std - zo) > 1e-3) > 0.99 * Pn      # not the other network's draw ...
    assert np.count_nonzero(np.abs(diff / noise_std - z) > 1e-3) == 0              # ... but this one's


# ---- the images ---------------------------------------------------------------------------------------------------------------------
def _behaviour(e):
    e.reset(seed=21)
    a = e.policy_actions(seed=9, t=2)
    rollout_device(e, 5, seed=13, reset=False, policy=True)
    P.evaluate_rollout(e, gamma=0.99, lam=0.95, bootstrap=("terminated", "truncated"))
    d = e.handle.rollout_download(want=("observations", "actions", "rewards"))
    o = e.handle.rollout_onpolicy_download(("log_probs", "values", "advantages"))
    return dict(a=a, **d, **o)


@pytest.mark.parametrize("shape,K,part", [("one", 3, [1, 2]), ("h64", 3, [2, 1]), ("tanh40", 2, None), ("four", 3, [0, 2]), ("ieee123", 2, None)])
def test_after_a_round_every_client_acts_and_evaluates_as_a_fresh_twin_with_the_aggregate_installed(shape, K, part):
    """the twin pattern of tests/test_gpu_learner.py: a fresh environment with MLPPolicy / MLPValue built from ``fedavg_np``'s result
    -- which also proves that the padding stayed zero and that the clients outside the list were written"""
    c = _scatter(shape, K, nets=("policy", "value"))
    fed = c["fed"]
    twin = _env(c["feeder"])
    try:
        part = list(range(K)) if part is None else part
        weights = [2.0 + k for k in range(len(part))]
        want = {}
        for net in ("policy", "value"):
            g, ps = fed.global_parameters(net), _params(c, net)
            norms = np.sqrt(np.diag(fed.measure(net, part)))
            want[net] = (g, ps, norms)
        out = fed.round(weights=weights, participants=part, clip_norm=float(want["policy"][2].max()) * 0.75, server_lr=0.5)
        agg = {}
        for net in ("policy", "value"):
            g, ps, norms = want[net]
            assert _same(out[net]["norms"].view(np.float32), norms.view(np.float32)) and out[net]["participants"] == part and out[net]["filtered"] == []
            agg[net] = fedavg_np(g, [ps[k] for k in part], weights, norms=norms, clip_norm=float(want["policy"][2].max()) * 0.75, server_lr=0.5)
            assert _same(fed.global_parameters(net), agg[net])
        dims_p = c["learners"][0].info("policy")["dims"]
        dims_v = c["learners"][0].info("value")["dims"]
        twin.set_policy(_policy(c["feeder"], *split_parameters(agg["policy"], dims_p), c["activation"]), stochastic=True)
        twin.set_value(_value(c["feeder"], *split_parameters(agg["value"], dims_v), c["activation"]))
        ref = _behaviour(twin)
        for k, e in enumerate(c["envs"]):
            got = _behaviour(e)
            for key in ref:
                assert np.array_equal(ref[key], got[key]), (shape, k, key)
    finally:
        twin.close()
        fed.close()


# ---- Adam's state -------------------------------------------------------------------------------------------------------------------
FIELDS = ["observations", "actions", "log_probs", "advantages", "returns", "values", "indices"]


def _collect(env, pol, k):
    env.reset(seed=3 + k)
    rollout_device(env, 5, seed=7 + k, reset=False, policy=True)
    P.evaluate_rollout(env, gamma=0.99, lam=0.95, bootstrap=("terminated", "truncated"))
    OnPolicyBatches(env, B * 5, policy=pol, adv_norm="rollout", seed=5, fields=FIELDS).prepare()


@pytest.mark.parametrize("reset_moments", [False, True])
def test_adams_moments_and_step_count_survive_a_round_unless_reset(reset_moments):
    """two clients share a start through set_global, take two real steps each on their own rollouts, a round runs, and the next step
    is ``adam_np`` from (the aggregated parameters, the kept m and v, t = 3) -- or, with reset_moments, from (m = v = 0, t = 1)"""
    c = _scatter("h64", 2, nets=("policy", "value"))
    fed = c["fed"]
    try:
        for net in c["nets"]:
            fed.set_global(net)                                # client 1 takes client 0's parameters
            ps = _params(c, net)
            assert _same(ps[0], ps[1]) and _same(ps[0], fed.global_parameters(net))
        for k, (e, l) in enumerate(zip(c["envs"], c["learners"])):
            _collect(e, c["installed"][0]["policy"], k)        # (every client's normalisation is client 0's)
            for s in range(2):
                l.step(e.handle.onpolicy_batch(5, s, 0, 33))
        g0 = {net: fed.global_parameters(net) for net in c["nets"]}
        kept = {net: [l.download(net) for l in c["learners"]] for net in c["nets"]}
        for net in c["nets"]:
            assert not _same(kept[net][0]["params"], kept[net][1]["params"]) and kept[net][0]["m"].any() and kept[net][1]["v"].any()
            assert not _same(kept[net][0]["params"], g0[net])  # here EVERY client's update is non-zero
        out = fed.round(weights=[40.0, 25.0], clip_norm=0.02, reset_moments=reset_moments)
        for net in c["nets"]:
            assert (out[net]["norms"] > 0.0).all()
            agg = fedavg_np(g0[net], [kept[net][k]["params"] for k in range(2)], [40.0, 25.0], norms=out[net]["norms"], clip_norm=0.02)
            for k, l in enumerate(c["learners"]):
                got = l.download(net)
                assert _same(got["params"], agg)
                if reset_moments:
                    assert not got["m"].any() and not got["v"].any() and l.info(net)["step"] == 0
                else:
                    assert _same(got["m"], kept[net][k]["m"]) and _same(got["v"], kept[net][k]["v"]) and l.info(net)["step"] == 2
        for k, (e, l) in enumerate(zip(c["envs"], c["learners"])):
            l.step(e.handle.onpolicy_batch(5, 2, 0, 33))
            for net in c["nets"]:
                got, st = l.download(net), l.stats(net)
                agg = fedavg_np(g0[net], [kept[net][j]["params"] for j in range(2)], [40.0, 25.0], norms=out[net]["norms"], clip_norm=0.02)
                zero = np.zeros_like(agg)
                m0, v0, t = (zero, zero, 1) if reset_moments else (kept[net][k]["m"], kept[net][k]["v"], 3)
                assert st["step"] == t
                p, m, v = adam_np(agg, got["grads"], m0, v0, t, HYPER, st["grad_norm"])
                assert _same(got["params"], p) and _same(got["m"], m) and _same(got["v"], v), (net, k)
    finally:
        fed.close()


# ---- determinism --------------------------------------------------------------------------------------------------------------------
def test_two_twin_federations_end_with_the_same_bits():
    envs = _envs("ieee13", 6)
    a = _scatter("four", 3, nets=("policy", "value"), envs=envs[:3])
    b = _scatter("four", 3, nets=("policy", "value"), envs=envs[3:])
    try:
        start = a["fed"].global_parameters("policy")
        for c in (a, b):
            c["fed"].round(weights=[1.0, 2.0, 3.0], clip_norm=0.1, noise_std=0.003, seed=77)
            for k, (e, l) in enumerate(zip(c["envs"], c["learners"])):      # the clients move apart again: a step each
                _collect(e, c["installed"][0]["policy"], k)
                l.step(e.handle.onpolicy_batch(5, 0, 0, 33))
            c["fed"].round(participants=[2, 0], server_lr=0.5, noise_std=0.003, seed=77)
        ga, gb = a["fed"].global_parameters("policy"), b["fed"].global_parameters("policy")
        assert _same(ga, gb) and not _same(ga, start)
        assert all(_same(p, ga) for c in (a, b) for p in _params(c, "policy"))
        assert a["fed"].rounds == 2 and a["fed"].info("policy")["rounds"] == 2
    finally:
        for c in (a, b):
            c["fed"].close()


# ---- the refusals -------------------------------------------------------------------------------------------------------------------
def _raw_create(lib, envs, net=0):
    f = ctypes.c_void_p()
    hs = (ctypes.c_void_p * len(envs))(*[e.handle._h for e in envs])
    return lib.gs_fed_create(hs, len(envs), net, ctypes.byref(f)), f


def _refused(lib, rc, code, text):
    assert rc == code, (rc, lib.gs_last_error(None).decode())
    assert text in lib.gs_last_error(None).decode(), lib.gs_last_error(None).decode()


def _valid_round(c):
    c["fed"].aggregate("policy", [1, 2, 0], [1.0, 2.0, 3.0], clip_norm=0.1, noise_std=0.002, seed=9, round=4)
    return c["fed"].global_parameters("policy")


def test_refusals_change_nothing_and_a_dead_federation_can_still_be_destroyed():
    lib = _lib.load()
    envs = _envs("ieee13", 3)
    c = _scatter("h64", 3)
    expected = _valid_round(c)                                 # what the valid round gives without any refusal before it
    c["fed"].close()

    # gs_fed_create
    c = _scatter("h64", 3, federate=False)
    rc, _ = _raw_create(lib, [envs[0], envs[1], envs[0]])
    _refused(lib, rc, I, "one handle")
    rc, _ = _raw_create(lib, envs, net=9)
    _refused(lib, rc, I, "unknown net")
    rc, _ = _raw_create(lib, envs * 11)
    _refused(lib, rc, I, "outside 1")
    for e in envs:
        e.set_value(None)                                      # (a value network an earlier test left ends with its learner)
    rc, _ = _raw_create(lib, envs, net=1)                      # no learner for the value network
    _refused(lib, rc, S, "holds no learner")
    odd = _env("ieee13")
    try:
        _install(odd, "ieee13", [64, 48], "relu", 0, ("policy",), 100)
        P.DeviceLearner(odd, nets=("policy",), **HYPER)
        rc, _ = _raw_create(lib, [envs[0], odd])
        _refused(lib, rc, I, "layers, widths or activation")
        _install(odd, "ieee13", [64, 64], "tanh", 0, ("policy",), 100)
        P.DeviceLearner(odd, nets=("policy",), **HYPER)
        rc, _ = _raw_create(lib, [envs[0], odd])
        _refused(lib, rc, I, "layers, widths or activation")
        mean, std = _normalisation("ieee13")
        ws, bs = _layers([odd.obs_dim, 64, 64, 2 * odd.action_dim], 0, 100)
        shifted = mean.copy(); shifted[0] = np.nextafter(shifted[0], np.inf)
        odd.set_policy(P.MLPPolicy(ws, bs, activation="relu", head="gaussian_tanh", obs_mean=shifted, obs_std=std, compute="float32"), stochastic=True)
        P.DeviceLearner(odd, nets=("policy",), **HYPER)
        rc, _ = _raw_create(lib, [envs[0], odd])
        _refused(lib, rc, I, "normalisation")
    finally:
        odd.close()
    before = _params(c, "policy")

    # gs_fed_aggregate / gs_fed_measure on a live federation: refused, nothing changed
    c["fed"] = fed = P.FederatedLearners(c["learners"])
    bad = [(dict(weights=[1.0, -1.0, 1.0]), "not finite or negative"), (dict(weights=[1.0, math.nan, 1.0]), "not finite or negative"),
           (dict(weights=[0.0, 0.0, 0.0]), "sum to"), (dict(clip_norm=-0.5), "finite and >= 0"), (dict(noise_std=math.inf), "finite and >= 0"),
           (dict(noise_std=math.nan), "finite and >= 0"), (dict(server_lr=-1.0), "finite and >= 0"), (dict(participants=[0, 3, 1]), "outside 0"),
           (dict(participants=[0, 1, 0]), "named twice"), (dict(participants=[], weights=[]), "participants outside 1"), (dict(struct_size=8), "struct_size")]
    for kw, text in bad:
        args = dict(participants=[0, 1, 2], weights=[1.0, 1.0, 1.0])
        args.update(kw)
        with pytest.raises(PowerFlowError, match=text) as ei:
            fed.aggregate("policy", args.pop("participants"), args.pop("weights"), **args)
        assert f"error {I}:" in str(ei.value)
    rc = lib.gs_fed_measure(fed._feds[0], (ctypes.c_int32 * 2)(1, 1), 2, (ctypes.c_double * 4)())
    _refused(lib, rc, I, "named twice")
    rc = lib.gs_fed_measure(fed._feds[0], (ctypes.c_int32 * 2)(1, 3), 2, (ctypes.c_double * 4)())
    _refused(lib, rc, I, "outside 0")
    with pytest.raises(PowerFlowError, match="no round has run"):
        fed.stats("policy")
    assert all(_same(a, b) for a, b in zip(_params(c, "policy"), before)) and _same(fed.global_parameters("policy"), before[0])
    assert fed.info("policy")["rounds"] == 0
    assert _same(_valid_round(c), expected)                    # the bits it gave before
    fed.close()

    # a learner created again, a network installed again: GS_E_STATE from every call, and gs_fed_destroy still succeeds
    for how in ("created again", "installed again"):
        c = _scatter("h64", 3)
        fed = c["fed"]
        if how == "created again":
            c["learners"][1] = P.DeviceLearner(envs[1], nets=("policy",), **HYPER)
            text = "learner of client 1 was created again"
        else:
            envs[2].set_policy(c["installed"][2]["policy"], stochastic=True)
            text = "client 2 holds no learner"
        calls = [lambda: fed.aggregate("policy", [0, 1, 2], [1.0, 1.0, 1.0]), lambda: fed.measure("policy"), lambda: fed.set_global("policy"),
                 lambda: fed.global_parameters("policy"), lambda: fed.info("policy"), lambda: fed.stats("policy")]
        for call in calls:
            with pytest.raises(PowerFlowError, match=text) as ei:
                call()
            assert f"error {S}:" in str(ei.value)
        f = fed._feds.pop(0)
        assert lib.gs_fed_destroy(f) == _lib.GS_OK
        c = _scatter("h64", 3)
        assert _same(_valid_round(c), expected)
        c["fed"].close()

    # a client destroyed
    doomed = [_env("ieee13") for _ in range(2)]
    c = _scatter("h64", 2, envs=doomed)
    fed = c["fed"]
    doomed[1].close()
    with pytest.raises(PowerFlowError, match="client 1 was destroyed") as ei:
        fed.aggregate("policy", [0, 1], [1.0, 1.0])
    assert f"error {S}:" in str(ei.value)
    with pytest.raises(PowerFlowError, match="client 1 was destroyed"):
        fed.measure("policy")
    assert lib.gs_fed_destroy(fed._feds.pop(0)) == _lib.GS_OK
    doomed[0].close()                                          # (after its federation: the handle's list no longer names it)
    survivor = [_env("ieee13") for _ in range(2)]
    c = _scatter("h64", 2, envs=survivor)
    survivor[0].close(); survivor[1].close()                   # both clients first, the federation last
    assert lib.gs_fed_destroy(c["fed"]._feds.pop(0)) == _lib.GS_OK
    c = _scatter("h64", 3)
    assert _same(_valid_round(c), expected)
    c["fed"].close()


# ---- non-interference ---------------------------------------------------------------------------------------------------------------
def test_a_learner_in_a_federation_that_never_runs_a_round_behaves_as_one_outside():
    envs = _envs("ieee13", 3)
    c = _scatter("h64", 2, nets=("policy", "value"), seed0=300)              # envs[0] and envs[1] join a federation ...
    lone = _scatter("h64", 1, nets=("policy", "value"), seed0=300, envs=[envs[2]], federate=False)      # ... envs[2], the same client 0, joins none
    try:
        outs = []
        for e, l in ((c["envs"][0], c["learners"][0]), (lone["envs"][0], lone["learners"][0])):
            _collect(e, c["installed"][0]["policy"], 0)
            d = e.handle.rollout_download(want=("observations", "actions", "rewards"))
            o = e.handle.rollout_onpolicy_download(("log_probs", "values", "advantages"))
            l.step(e.handle.onpolicy_batch(5, 0, 0, 33))
            outs.append(dict(**d, **o, **{f"{net}.{k}": v for net in ("policy", "value") for k, v in l.download(net).items()}))
        for key in outs[0]:
            assert np.array_equal(outs[0][key], outs[1][key]), key
        assert outs[0]["policy.m"].any()
    finally:
        c["fed"].close()


# ---- the outlier filter through the Python class ------------------------------------------------------------------------------------
def test_round_with_byzantine_tolerance_drops_the_client_whose_update_is_negated():
    feeder, _, hidden, activation = SHAPES["h64"]
    envs = _envs(feeder, 5)
    rng = np.random.default_rng(5)
    dims = [envs[0].obs_dim] + hidden + [2 * envs[0].action_dim]
    ws0, bs0 = _layers(dims, 0, 100)
    dw, db = [0.02 * rng.normal(size=w.shape) for w in ws0], [0.02 * rng.normal(size=b.shape) for b in bs0]
    learners = []
    for k, e in enumerate(envs):
        sign = 0.0 if k == 0 else -1.0 if k == 3 else 1.0                    # client 0 is the global model, client 3 pulls the other way
        rk = np.random.default_rng(50 + k)
        ws = [w + sign * d + (0.002 * rk.normal(size=w.shape) if k else 0.0) for w, d in zip(ws0, dw)]
        bs = [b + sign * d + (0.002 * rk.normal(size=b.shape) if k else 0.0) for b, d in zip(bs0, db)]
        e.set_policy(_policy(feeder, ws, bs, activation), stochastic=True)
        learners.append(P.DeviceLearner(e, nets=("policy",), **HYPER))
    fed = P.FederatedLearners(learners)
    try:
        g = fed.global_parameters("policy")
        ps = [l.download("policy", ("params",))["params"] for l in learners]
        G = fed.measure("policy")
        assert filter_outliers_np(G, 1) == [3]
        out = fed.round(weights=[1.0, 2.0, 3.0, 50.0, 4.0], byzantine_tolerance=1)["policy"]
        assert out["filtered"] == [3] and out["participants"] == [0, 1, 2, 4] and out["n"] == 4
        want = fedavg_np(g, [ps[k] for k in (0, 1, 2, 4)], [1.0, 2.0, 3.0, 4.0])
        assert _same(fed.global_parameters("policy"), want)
        for l in learners:                                                   # the dropped client receives the global model too
            assert _same(l.download("policy", ("params",))["params"], want)
        assert fed.round(byzantine_tolerance=3)["policy"]["filtered"] == []  # n <= 2 tolerance: nobody is dropped
    finally:
        fed.close()
