"""CPU: the NumPy restatements of the federation (grid_fed_rl_gym_amd/federated.py; include/gridstep.h "the federation") and the
host logic of ``FederatedLearners``.

``fedavg_np`` against the reference's form (federated/core.py, ``FedAvgAggregator.aggregate``): sum_k (w_k / W) p_k in float64.
Both are float64 sums of at most K + 2 roundings before the ONE rounding to float32 -- relative to the float32 grid the float64
error is 2^-29 (K + 2), so the two can differ only where a result lies that close to a rounding boundary: by one float32 ulp."""
import math

import numpy as np
import pytest

import grid_fed_rl_gym_amd as P
from grid_fed_rl_gym_amd import federated as F
from oracle import oracle_np as O


def _clients(K, n=4099, seed=0):
    rng = np.random.default_rng(seed)
    g = rng.normal(0.0, 0.3, n).astype(np.float32)
    ps = [(g + rng.normal(0.0, 0.02, n).astype(np.float32)).astype(np.float32) for _ in range(K)]
    return g, ps


def _ulps(a, b):
    """distance in float32 grid steps (same-sign finite values and zeros)"""
    ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    ia, ib = np.where(ia < 0, -(ia & 0x7FFFFFFF), ia), np.where(ib < 0, -(ib & 0x7FFFFFFF), ib)
    return np.abs(ia - ib)


@pytest.mark.parametrize("K,weights", [(1, [3.0]), (2, [1.0, 1.0]), (2, [120.0, 7.0]), (5, [5.0, 1.0, 0.0, 33.0, 2.5]), (5, [1.0] * 5)])
def test_fedavg_without_clip_and_noise_is_the_references_weighted_mean(K, weights):
    g, ps = _clients(K, seed=K)
    got = F.fedavg_np(g, ps, weights)
    W = float(sum(weights))
    ref = np.zeros(g.size, dtype=np.float64)
    for w, p in zip(weights, ps):
        ref = ref + (w / W) * p.astype(np.float64)
    ref32 = ref.astype(np.float32)
    d = _ulps(got, ref32)
    print(f"K={K}: {int(np.count_nonzero(d))} of {g.size} parameters differ from the reference's form, at most {int(d.max())} ulp")
    assert got.dtype == np.float32 and d.max() <= 1


def test_the_two_exactness_consequences():
    g, ps = _clients(3, seed=9)
    # clients all equal to g: g' == g bit for bit -- with and without a clip, whatever the weights and the server's rate
    same = F.fedavg_np(g, [g.copy(), g.copy(), g.copy()], [1.0, 5.0, 0.5], norms=[0.0, 0.0, 0.0], clip_norm=0.3, server_lr=0.7)
    assert np.array_equal(same.view(np.uint32), g.view(np.uint32))
    # one participant, weight 1, server_lr 1, no clip, no noise: a bit-exact copy of that client (p - g is exact in float64 here)
    assert float(np.min(np.abs(ps[1]))) > 0.0 and float(np.max(np.abs(np.log2(np.abs(ps[1])) - np.log2(np.abs(g))))) < 28.0
    one = F.fedavg_np(g, [ps[1]], [1.0])
    assert np.array_equal(one.view(np.uint32), ps[1].view(np.uint32))


def test_clip_scales_and_coefficients_below_at_and_above_the_clip():
    clip = 0.5
    norms = [0.25, 0.5 - 1e-6, 0.5, 2.0]
    c, a = F.fed_coefficients_np([1.0, 1.0, 2.0, 4.0], norms, clip_norm=clip, server_lr=0.5)
    assert c[0] == 1.0 and c[1] == 1.0                       # below the clip, and where norm + 1e-6 reaches it
    assert c[2] == clip / (0.5 + 1e-6) < 1.0                 # at the clip: Adam's form shrinks by the 1e-6
    assert c[3] == clip / (2.0 + 1e-6)
    W = 1.0 + 1.0 + 2.0 + 4.0
    for k, w in enumerate([1.0, 1.0, 2.0, 4.0]):
        assert a[k] == (0.5 * (w / W)) * c[k]
    c, a = F.fed_coefficients_np([1.0, 3.0], [7.0, 1e9], clip_norm=0.0)
    assert list(c) == [1.0, 1.0] and list(a) == [0.25, 0.75]
    # the clipped update has the clip's norm: g + c d moves by at most clip_norm
    g, ps = _clients(1, seed=4)
    d = ps[0].astype(np.float64) - g.astype(np.float64)
    norm = math.sqrt(math.fsum(d * d))
    out = F.fedavg_np(g, ps, [1.0], norms=[norm], clip_norm=0.1 * norm)
    moved = out.astype(np.float64) - g.astype(np.float64)
    assert abs(math.sqrt(math.fsum(moved * moved)) / (0.1 * norm) - 1.0) < 1e-5
    with pytest.raises(ValueError):
        F.fedavg_np(g, ps, [1.0], clip_norm=0.1)             # a clip needs the norms
    with pytest.raises(ValueError):
        F.fedavg_np(g, ps, [1.0, 2.0])


def test_noise_is_the_oracles_normal_quad_recipe():
    """With the environment's tag in place of 'FEDN' the counter (q, round, net, tag) is rng_normal_quad's (instance, step, draw):
    the words are equal, the normals agree to the few ulp that separate NumPy's log / cos / sin from libm's."""
    for seed, rnd, net in ((0, 0, 0), (5, 3, 17), (0xDEADBEEFCAFE, 41, 4)):
        words = F.fed_noise_words(seed, rnd, net, 6, tag=0x47535450)
        z = F.fed_noise_np(seed, rnd, net, 23, tag=0x47535450)
        assert z.shape == (23,)
        for q in range(6):
            assert tuple(int(x) for x in words[q]) == O.philox4x32((q, rnd, net, 0x47535450), (seed & 0xFFFFFFFF, seed >> 32))
            ref = O.rng_normal_quad(seed, q, rnd, net)
            for comp in range(4):
                if 4 * q + comp < 23:
                    assert abs(z[4 * q + comp] - ref[comp]) <= 1e-14, (q, comp)
    a, b = F.fed_noise_np(7, 2, 0, 64), F.fed_noise_np(7, 2, 0, 61)
    assert np.array_equal(a[:61], b)                          # a prefix: z[j] depends on j alone
    assert not np.array_equal(a, F.fed_noise_np(7, 3, 0, 64)) and not np.array_equal(a, F.fed_noise_np(7, 2, 1, 64))
    assert not np.array_equal(a, F.fed_noise_np(7, 2, 0, 64, tag=0x47535450))


def test_noise_has_zero_mean_and_unit_variance():
    n = 1 << 16
    z = F.fed_noise_np(11, 0, 0, n)
    mean, var = float(z.mean()), float(z.var())
    print(f"2^16 draws: mean {mean:.3e} (standard error {1 / math.sqrt(n):.3e}), variance {var:.5f} (standard error {math.sqrt(2 / n):.3e})")
    assert abs(mean) <= 5.0 / math.sqrt(n)
    assert abs(var - 1.0) <= 5.0 * math.sqrt(2.0 / n)


def _gram(vectors):
    v = np.asarray(vectors, dtype=np.float64)
    return v @ v.T


def test_filter_drops_the_anti_aligned_client_and_respects_the_reference_rule():
    rng = np.random.default_rng(3)
    base = rng.normal(size=50)
    good = [base + 0.1 * rng.normal(size=50) for _ in range(4)]
    vs = good[:2] + [-base] + good[2:]
    G = _gram(vs)
    assert F.filter_outliers_np(G, 1) == [2]
    # nothing is dropped at n <= 2 tolerance (5 <= 6), nor with tolerance 0
    assert F.filter_outliers_np(G, 3) == [] and F.filter_outliers_np(G, 0) == []
    assert F.filter_outliers_np(_gram(vs[:2]), 1) == []
    # ties at the threshold are kept: four identical updates have equal means, none is STRICTLY below their percentile
    assert F.filter_outliers_np(_gram([base] * 4), 1) == []
    # the index-order cap: of eight clients two are anti-aligned, the 25th percentile lies above both; tolerance 1 drops the first
    eight = [good[0], -base, good[1], good[2], -base + 0.05 * rng.normal(size=50), good[3], good[0] * 2.0, good[1] * 0.5]
    G8 = _gram(eight)
    nrm = np.sqrt(np.diag(G8))
    sim = G8 / (nrm[:, None] * nrm[None, :] + 1e-8)
    np.fill_diagonal(sim, 0.0)
    avg = sim.mean(axis=1)
    below = [int(i) for i in np.where(avg < np.percentile(avg, 25))[0]]
    assert below == [1, 4]
    assert F.filter_outliers_np(G8, 1) == [1] and F.filter_outliers_np(G8, 2) == [1, 4] and F.filter_outliers_np(G8, 3) == [1, 4]
    with pytest.raises(ValueError):
        F.filter_outliers_np(np.zeros((2, 3)), 1)


def test_gaussian_sigma_is_the_references_formula():
    for eps, delta, sens in ((1.0, 1e-5, 1.0), (0.5, 1e-6, 0.25), (8.0, 1e-3, 2.0)):
        assert F.gaussian_sigma(eps, delta, sens) == math.sqrt(2.0 * math.log(1.25 / delta)) * sens / eps
    for bad in ((0.0, 1e-5, 1.0), (1.0, 0.0, 1.0), (1.0, 1.0, 1.0), (1.0, 1e-5, -1.0)):
        with pytest.raises(ValueError):
            F.gaussian_sigma(*bad)


class _FakeLearner:
    def __init__(self, env, nets):
        self.env, self.nets = env, tuple(nets)


def _bare(K):
    """a FederatedLearners without a library behind it: what ``round`` checks on the host comes before any call"""
    f = object.__new__(P.FederatedLearners)
    f.K, f.nets, f._feds, f._rounds, f.learners = K, (), {}, 0, []
    return f


def test_every_value_error_of_the_host_logic():
    env_a, env_b = object(), object()
    with pytest.raises(ValueError, match="outside 1"):
        P.FederatedLearners([])
    with pytest.raises(ValueError, match="outside 1"):
        P.FederatedLearners([_FakeLearner(object(), ("policy",)) for _ in range(33)])
    with pytest.raises(ValueError, match="share an environment"):
        P.FederatedLearners([_FakeLearner(env_a, ("policy",)), _FakeLearner(env_a, ("policy",))])
    with pytest.raises(ValueError, match="no network in common"):
        P.FederatedLearners([_FakeLearner(env_a, ("policy",)), _FakeLearner(env_b, ("value",))])
    f = _bare(4)
    for kwargs, text in ((dict(participants=[]), "no participant"), (dict(participants=[0, 4]), "outside 0"), (dict(participants=[-1]), "outside 0"),
                         (dict(participants=[1, 2, 1]), "named twice"), (dict(weights=[1.0, 2.0]), "weights for 4"),
                         (dict(weights=[1.0, -1.0, 1.0, 1.0]), "finite and >= 0"), (dict(weights=[1.0, math.nan, 1.0, 1.0]), "finite and >= 0"),
                         (dict(weights=[1.0, math.inf, 1.0, 1.0]), "finite and >= 0"), (dict(clip_norm=-1.0), "clip_norm"),
                         (dict(noise_std=math.inf), "noise_std"), (dict(noise_std=math.nan), "noise_std"), (dict(server_lr=-0.5), "server_lr"),
                         (dict(byzantine_tolerance=-1), "byzantine_tolerance")):
        with pytest.raises(ValueError, match=text):
            f.round(**kwargs)
    assert f.rounds == 0 and f.round() == {} and f.rounds == 1      # (no network: nothing to call)
    with pytest.raises(ValueError, match="not one of the federation's networks"):
        f.measure("policy")
    with pytest.raises(ValueError, match="unknown network"):
        f.global_parameters("actor")
    f.nets = ("policy",)
    with pytest.raises(ValueError, match="sum to 0"):
        f.round(weights=[0.0, 0.0, 0.0, 0.0])
    f.nets = ()
    f.close()
