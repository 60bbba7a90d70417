"""GPU: on-policy minibatch epochs on the device (include/gridstep.h "on-policy minibatch epochs") --
gs_k_opb_index against ``permutation_np``, gs_k_opb_gather_f64 / _f32 against ``onpolicy_batch_np`` bit for bit, the rollout's and
the minibatch's advantage statistics against long-double / ``math.fsum`` references within the bounds of their reduction orders, the
state and argument rules, caller buffers and non-interference.

Every case runs with ``ConstraintLimits.of(env, voltage=(0.97, 1.03), thermal=0.5)`` and cost critics on voltage and thermal.  On the
13-bus feeder these limits leave transitions with a cost (asserted).  On the 123-bus feeder, B = 37, T = 5, they leave NONE -- 0 of
185 transitions in every channel (observed on the MI355X) -- so that case cannot assert non-zero costs; its cost advantages are still
non-zero (the critics' values are not), which is what the combined advantage reads, and that is asserted for every case.

Policies, critics and the normalisation are built as in tests/test_gpu_onpolicy.py (weights N(0, 1 / fan_in), statistics from a
short random rollout, std = 1 on the columns that do not vary).  Every case is prepared once and shared by the tests that read it.

Bounds, none of them computed from the device:
  rollout statistics    section 14's: eps (max|x| + sqrt(N) log2(N) max|x - mean|) for the mean, eps sqrt(N) log2(N) max|x - mean|
                        for the deviation, eps = 2^-52, against long double on the data shifted by its first entry.
  minibatch statistics  section 17's with d = ceil(n / 1024) - 1 + 10: (d + 2) u sum|x| / n for the mean and
                        (d / 2 + 3) u std + (d + 2) u sum|x| / n for the deviation, u = 2^-53, against ``math.fsum``."""
import ctypes
import math

import numpy as np
import pytest

import grid_fed_rl_gym_amd as P
from grid_fed_rl_gym_amd import _lib
from grid_fed_rl_gym_amd.components import PowerFlowError
from grid_fed_rl_gym_amd.rollout import OnPolicyBatches, onpolicy_batch_np, permutation_np, rollout_device

pytestmark = pytest.mark.gpu

FEEDERS = {"ieee13": lambda: P.ieee13_like("epsilon"), "ieee123": P.ieee123_like}
# name: (feeder, B, T)
CASES = {"ieee13-37x5": ("ieee13", 37, 5), "ieee123-37x5": ("ieee123", 37, 5), "ieee13-1x257": ("ieee13", 1, 257),
         "ieee13-200x33": ("ieee13", 200, 33)}
CHANNELS = {"voltage": 0, "thermal": 2}
LAMBDAS = {"voltage": 0.7, "thermal": 1.3}
LAM3 = (0.7, 0.0, 1.3)
SCALARS = ("log_probs", "advantages", "returns", "values")
EPS, U = 2.0 ** -52, 2.0 ** -53
S, I = _lib.GS_E_STATE, _lib.GS_E_INVALID


def _env(feeder, B, episode_length=7):
    fs = FEEDERS[feeder]()
    return P.BatchedGridEnvironment(fs, num_envs=B, solver="fbs", stochastic_loads=True, weather_variation=True, jacobian="exact", tolerance=1e-9,
                                    max_iterations=100, power_base=fs.base_power_va, episode_length=episode_length)


_NORM = {}


def _normalisation(feeder):
    """(mean, std) per observation column over a 4-step random rollout of 64 instances; once per feeder"""
    if feeder not in _NORM:
        env = _env(feeder, 64, episode_length=5)
        obs = P.collect_random_data(env, 4, seed=11)["observations"]
        env.close()
        mean, std = obs.mean(axis=0), obs.std(axis=0)
        constant = std <= 1e-12 * np.maximum(1.0, np.abs(mean))
        _NORM[feeder] = (mean, np.where(constant, 1.0, std + 1e-6))
    return _NORM[feeder]


def _layers(dims, seed):
    rng = np.random.default_rng(seed)
    ws = [rng.normal(0.0, 1.0 / math.sqrt(dims[l]), (dims[l + 1], dims[l])) for l in range(len(dims) - 1)]
    bs = [rng.normal(0.0, 0.1, dims[l + 1]) for l in range(len(dims) - 1)]
    return ws, bs


def _policy(env, feeder, seed=0, head="gaussian_tanh"):
    ws, bs = _layers([env.obs_dim, 64, 64, 2 * env.action_dim if head == "gaussian_tanh" else env.action_dim], seed)
    mean, std = _normalisation(feeder)
    return P.MLPPolicy(ws, bs, activation="relu", head=head, obs_mean=mean, obs_std=std, compute="float32")


def _value(env, feeder, seed):
    ws, bs = _layers([env.obs_dim, 64, 64, 1], seed)
    mean, std = _normalisation(feeder)
    return P.MLPValue(ws, bs, activation="relu", obs_mean=mean, obs_std=std)


def _collect(env, feeder, T, seed=3, policy_seed=7, costs=True, stochastic=True):
    """reset, a stochastic float32 policy rollout, the reward critic and (costs) the cost critics on voltage and thermal"""
    pol = _policy(env, feeder, seed=1, head="gaussian_tanh" if stochastic else "tanh")
    env.set_policy(pol, stochastic=stochastic)
    env.set_value(_value(env, feeder, 2))
    env.reset(seed=seed)
    rollout_device(env, T, seed=policy_seed, reset=False, policy=True)
    _evaluate(env, feeder, costs)
    return pol


def _evaluate(env, feeder, costs=True):
    P.evaluate_rollout(env, gamma=0.99, lam=0.95, bootstrap=("terminated", "truncated"))
    if costs:
        for name, c in CHANNELS.items():
            env.set_cost_value(name, _value(env, feeder, 10 + c))
        P.rollout_costs(env, P.ConstraintLimits.of(env, voltage=(0.97, 1.03), thermal=0.5), kinds="excess")
        P.evaluate_rollout_costs(env, gamma=0.99, lam=0.95, bootstrap=("terminated", "truncated"))


def _host(env, T, costs=True):
    """the host downloads ``onpolicy_batch_np`` is fed"""
    h = env.handle
    N = T * env.num_envs
    d = h.rollout_download(want=("observations", "actions", "terminals"))
    o = h.rollout_onpolicy_download(("log_probs", "values", "advantages", "returns"))
    out = dict(N=N, obs=d["observations"].reshape(N, -1), act=d["actions"].reshape(N, -1), terminals=d["terminals"], logp=o["log_probs"].reshape(N),
               val=o["values"][:T].reshape(N), adv=o["advantages"].reshape(N), ret=o["returns"].reshape(N), cadv=[None] * 3, cret=[None] * 3)
    if costs:
        cd = h.rollout_costs_download(("costs", "advantages", "returns"), channels=tuple(CHANNELS.values()))
        out["costs"] = cd["costs"]
        for c in CHANNELS.values():
            out["cadv"][c], out["cret"][c] = cd["advantages"][c].reshape(N), cd["returns"][c].reshape(N)
    return out


_PREPARED = {}


@pytest.fixture(scope="module")
def prepared():
    """name -> dict(env, pol, host arrays ...) of CASES, built on first use, closed when the module is done"""
    def get(name):
        if name not in _PREPARED:
            feeder, B, T = CASES[name]
            env = _env(feeder, B)
            pol = _collect(env, feeder, T)
            c = dict(env=env, pol=pol, feeder=feeder, B=B, T=T, **_host(env, T))
            assert c["terminals"].any() == (T >= 7)           # episode_length = 7: the longer rollouts hold episode ends
            print(f"{name}: transitions with a cost, per channel: {[(int((c['costs'][ch] > 0).sum())) for ch in range(3)]} of {B * T}")
            # the tightened limits leave costs on the 13-bus feeder; on the 123-bus feeder no transition of 37 x 5 has one (see the
            # module's docstring), so what the combination reads -- the cost ADVANTAGES of both channels -- is held to be non-zero everywhere
            if feeder == "ieee13":
                assert (c["costs"] > 0).any()
            assert all(np.any(c["cadv"][ch] != 0.0) for ch in CHANNELS.values())
            if feeder == "ieee13":
                assert env.obs_dim == 71                      # odd: the 8-byte path
            else:
                assert env.obs_dim == 684
            _PREPARED[name] = c
        return _PREPARED[name]
    yield get
    for c in _PREPARED.values():
        c["env"].close()
    _PREPARED.clear()


def _down(batch):
    """a batch's DeviceArray views as host arrays (None stays None; the cost fields stay lists of three)"""
    out = {}
    for k, v in batch.items():
        out[k] = [None if x is None else x.to_host() for x in v] if isinstance(v, list) else v.to_host()
    return out


def _same(got, want, keys=None):
    for k in keys or want:
        g, w = got[k], want[k]
        if isinstance(w, list):
            for c in range(3):
                assert (g[c] is None) == (w[c] is None), (k, c)
                if w[c] is not None:
                    assert g[c].dtype == w[c].dtype and np.array_equal(g[c], w[c]), (k, c)
        else:
            assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w, equal_nan=True), k


def _restate(c, idx, adv_norm, dtype, stats, lambdas=LAM3, shift=None, scale=None, costs=True):
    return onpolicy_batch_np(idx, c["obs"], c["act"], c["logp"], c["adv"], c["ret"], c["val"], c["cadv"] if costs else None,
                             c["cret"] if costs else None, lambdas=lambdas, adv_norm=adv_norm, adv_stats=stats, dtype=dtype, obs_shift=shift,
                             obs_scale=scale)


# ---- 1. the permutation ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(CASES))
def test_an_epochs_indices_are_the_permutation_and_cover_the_rollout(prepared, name):
    c = prepared(name)
    N = c["N"]
    for minibatch, epoch, seed in ((64, 3, 5), (N, 0, 2 ** 40 + 9)):
        b = OnPolicyBatches(c["env"], minibatch, fields=["indices"], seed=seed)
        b.prepare()
        want = permutation_np(seed, epoch, N)
        got = [x["indices"].to_host() for x in b.epoch(epoch)]
        assert len(got) == len(b) == -(-N // minibatch)
        assert all(g.dtype == np.int32 for g in got)
        assert [len(g) for g in got] == [minibatch] * (N // minibatch) + ([N % minibatch] if N % minibatch else [])      # the ragged last batch
        flat = np.concatenate(got)
        assert np.array_equal(flat, want)
        assert np.array_equal(np.sort(flat), np.arange(N))
    # minibatch size 1: the first three batches
    b = OnPolicyBatches(c["env"], 1, fields=["indices"], seed=5)
    b.prepare()
    assert len(b) == N
    want = permutation_np(5, 3, N)
    for k, x in zip(range(min(3, N)), b.epoch(3)):
        assert x["indices"].to_host().tolist() == [want[k]]


# ---- 2. every field, bit for bit -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("normalised", [False, True])
@pytest.mark.parametrize("adv_norm", ["none", "rollout", "minibatch"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("name", list(CASES))
def test_fields_are_bit_equal_to_the_restatement(prepared, name, dtype, adv_norm, normalised):
    c = prepared(name)
    N, pol = c["N"], c["pol"]
    minibatch = 1025 if N > 1025 else 64
    b = OnPolicyBatches(c["env"], minibatch, policy=pol if normalised else None, lambdas=LAMBDAS, adv_norm=adv_norm, dtype=dtype, seed=11)
    b.prepare()
    roll = b.stats
    assert roll.n == N
    perm = permutation_np(11, 1, N)
    shift, scale = (pol.obs_mean, 1.0 / pol.obs_std) if normalised else (None, None)
    seen = 0
    for first, batch in zip(range(0, N, minibatch), b.epoch(1)):
        got = _down(batch)
        assert np.array_equal(got["indices"], perm[first:first + minibatch])
        if adv_norm == "rollout":
            assert got["adv_stats"].tolist() == [roll.adv_mean, roll.adv_std]
        want = _restate(c, got["indices"], adv_norm, dtype, got["adv_stats"], shift=shift, scale=scale)
        _same(got, want)
        assert set(got) == set(want)
        seen += len(got["indices"])
    assert seen == N
    # the multipliers count: the combined advantage is not the reward's
    plain = _restate(c, perm[:minibatch], "none", np.float64, None, lambdas=(0.0, 0.0, 0.0))
    comb = _restate(c, perm[:minibatch], "none", np.float64, None)
    assert not np.array_equal(plain["advantages"], comb["advantages"])


# ---- 3. the statistics -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(CASES))
def test_rollout_statistics_within_the_bound_of_the_tree(prepared, name):
    c = prepared(name)
    N = c["N"]
    b = OnPolicyBatches(c["env"], 64, lambdas=LAMBDAS, fields=["advantages"])
    b.prepare()
    s = b.stats
    again = b.stats
    b.prepare()
    assert (s.adv_mean, s.adv_std) == (again.adv_mean, again.adv_std) == (b.stats.adv_mean, b.stats.adv_std)      # a second call: the same bits
    comb = c["adv"] - LAM3[0] * c["cadv"][0]
    comb = comb - LAM3[2] * c["cadv"][2]
    L = comb.astype(np.longdouble)
    L0 = L - L[0]
    m0 = L0.mean()
    dev = L0 - m0
    ref_mean, ref_std = L[0] + m0, np.sqrt((dev * dev).mean())
    amax, dmax = np.abs(L).max(), np.abs(dev).max()
    growth = np.sqrt(np.longdouble(N)) * np.log2(np.longdouble(max(N, 2)))
    tol_mean, tol_std = EPS * (amax + growth * dmax), EPS * growth * dmax
    err_mean, err_std = abs(np.longdouble(s.adv_mean) - ref_mean), abs(np.longdouble(s.adv_std) - ref_std)
    print(f"{name}: rollout advantage statistics, observed error / bound: mean {float(err_mean / tol_mean):.3g}, std {float(err_std / tol_std):.3g}")
    assert err_mean <= tol_mean and err_std <= tol_std and s.adv_std > 0


@pytest.mark.parametrize("n", [1, 64, 1025])
def test_minibatch_statistics_within_the_bound_of_the_reduction_order(prepared, n):
    c = prepared("ieee13-200x33")
    N = c["N"]
    b = OnPolicyBatches(c["env"], n, lambdas=LAMBDAS, adv_norm="minibatch", dtype=np.float64, fields=["advantages", "indices"], seed=4)
    b.prepare()
    it = b.epoch(2)
    next(it)
    got = _down(next(it))                        # the second batch: positions n .. 2 n - 1
    assert np.array_equal(got["indices"], permutation_np(4, 2, N)[n:2 * n])
    comb = _restate(c, got["indices"], "none", np.float64, None)["advantages"]
    xs = comb.tolist()
    d = -(-n // 1024) - 1 + 10
    mean = math.fsum(xs) / n
    std = math.sqrt(math.fsum((x - mean) ** 2 for x in xs) / n)
    mean_bound = (d + 2) * U * math.fsum(abs(x) for x in xs) / n
    std_bound = (d / 2 + 3) * U * std + mean_bound
    dev_mean, dev_std = got["adv_stats"].tolist()
    ratios = [abs(dev_mean - mean) / mean_bound, abs(dev_std - std) / std_bound]
    print(f"minibatch statistics, n = {n}: observed error / bound {['%.3g' % x for x in ratios]}")
    assert max(ratios) <= 1.0, ratios
    assert np.array_equal(got["advantages"], (comb - dev_mean) / (dev_std + 1e-8))
    if n == 1:
        assert dev_mean == xs[0] and dev_std == 0.0 and got["advantages"].tolist() == [0.0]


# ---- 4. multipliers ------------------------------------------------------------------------------------------------------------------------

def test_all_multipliers_zero_need_no_costs():
    feeder, B, T = "ieee13", 37, 5
    env = _env(feeder, B)
    _collect(env, feeder, T, costs=False)                  # gs_rollout_costs never ran on this handle
    N = B * T
    on = env.handle.rollout_onpolicy_download(("advantages",))["advantages"].reshape(N)
    b = OnPolicyBatches(env, N, adv_norm="none", dtype=np.float64)
    b.prepare()
    got = _down(next(b.epoch(0)))
    assert np.array_equal(got["advantages"], on[got["indices"]])
    assert "cost_advantages" not in got and np.isnan(got["adv_stats"]).all()
    # a multiplier or a cost field on this handle: refused
    h = env.handle
    _refused(lambda: h.onpolicy_prepare(lambdas=(0.0, 0.0, 0.5)), S, "channel 2")
    _refused(lambda: h.onpolicy_prepare(fields=["cost_returns"]), S, "no channel")
    _same(_down(next(b.epoch(0))), got)
    env.close()


# ---- 5. the rules ----------------------------------------------------------------------------------------------------------------------------

def _refused(call, code, text):
    with pytest.raises(PowerFlowError) as e:
        call()
    assert f"libgridstep error {code}:" in str(e.value) and text in str(e.value), str(e.value)


def test_state_and_argument_rules_and_nothing_launched_on_refusal():
    """every GS_E_STATE / GS_E_INVALID rule of the header but one: N >= 2^31 needs more transitions than a test can collect"""
    feeder, B, T = "ieee13", 37, 5
    N = B * T
    env = _env(feeder, B)
    h = env.handle
    _refused(lambda: h.onpolicy_prepare(), S, "no rollout")
    pol = _collect(env, feeder, T)
    _refused(lambda: h.onpolicy_batch(0, 0, 0, 8), S, "gs_onpolicy_prepare has not run")
    _refused(lambda: h.onpolicy_stats(), S, "gs_onpolicy_prepare has not run")
    D = env.obs_dim
    shift, scale = pol.obs_mean, 1.0 / pol.obs_std
    b = OnPolicyBatches(env, 64, policy=pol, lambdas=LAMBDAS, adv_norm="minibatch", seed=3)
    b.prepare()
    before = _down(h.onpolicy_batch(3, 0, 64, 64))
    stats = b.stats
    bad = np.array(shift)
    bad[D - 1] = np.nan
    inf = np.array(scale)
    inf[0] = np.inf
    refusals = [
        (lambda: h.onpolicy_prepare(struct_size=60), I, "struct_size"),
        (lambda: h.onpolicy_prepare(adv_norm=3), I, "adv_norm"),
        (lambda: h.onpolicy_prepare(adv_norm=-1), I, "adv_norm"),
        (lambda: h.onpolicy_prepare(dtype=2), I, "dtype"),
        (lambda: h.onpolicy_prepare(fields=512), I, "field bits"),
        (lambda: h.onpolicy_prepare(lambdas=(0.0, np.nan, 0.0)), I, "lambda[1]"),
        (lambda: h.onpolicy_prepare(lambdas=(np.inf, 0.0, 0.0)), I, "lambda[0]"),
        (lambda: h.onpolicy_prepare(adv_eps=-1e-9), I, "adv_eps"),
        (lambda: h.onpolicy_prepare(adv_eps=np.nan), I, "adv_eps"),
        (lambda: h.onpolicy_prepare(obs_shift=shift), I, "go together"),
        (lambda: h.onpolicy_prepare(obs_scale=scale), I, "go together"),
        (lambda: h.onpolicy_prepare(obs_shift=bad, obs_scale=scale), I, f"column {D - 1}"),
        (lambda: h.onpolicy_prepare(obs_shift=shift, obs_scale=inf), I, "column 0"),
        (lambda: h.onpolicy_prepare(lambdas=(0.0, 0.25, 0.0)), S, "channel 1"),          # the frequency channel has no critic
        (lambda: h.onpolicy_batch(3, 0, 0, 0), I, "outside"),
        (lambda: h.onpolicy_batch(3, 0, 0, -4), I, "outside"),
        (lambda: h.onpolicy_batch(3, 0, -1, 8), I, "outside"),
        (lambda: h.onpolicy_batch(3, 0, N - 7, 8), I, "outside"),
        (lambda: h.onpolicy_batch(3, 0, N, 1), I, "outside"),
    ]
    for call, code, text in refusals:
        _refused(call, code, text)
        # nothing was launched and the prepared state stands: the same valid batch gives the same bits
        _same(_down(h.onpolicy_batch(3, 0, 64, 64)), before)
    again = b.stats
    assert (again.adv_mean, again.adv_std) == (stats.adv_mean, stats.adv_std)
    _same(_down(h.onpolicy_batch(3, 0, N - 8, 8)), _down(h.onpolicy_batch(3, 0, N - 8, 8)))       # the last valid positions
    # a cost field covers every evaluated channel and only those
    assert [x is None for x in before["cost_advantages"]] == [False, True, False]
    # a further rollout: everything refuses until evaluation and prepare have run again
    rollout_device(env, T, seed=8, reset=False, policy=True)
    _refused(lambda: h.onpolicy_batch(3, 0, 0, 8), S, "gs_onpolicy_prepare has not run")
    _refused(lambda: h.onpolicy_stats(), S, "gs_onpolicy_prepare has not run")
    _refused(lambda: b.prepare(), S, "gs_rollout_evaluate has not run")
    P.evaluate_rollout(env, bootstrap=("terminated", "truncated"))
    _refused(lambda: b.prepare(), S, "channel 0")                              # multipliers, but the costs were not evaluated again
    _refused(lambda: h.onpolicy_prepare(fields=["cost_advantages"]), S, "no channel")
    h.onpolicy_prepare(fields=["advantages", "indices"])                       # without them: fine
    assert sorted(_down(h.onpolicy_batch(3, 0, 0, N))["indices"].tolist()) == list(range(N))
    # a deterministic rollout records no log-probabilities
    env.set_policy(_policy(env, feeder, seed=1, head="tanh"), stochastic=False)
    rollout_device(env, T, seed=9, reset=False, policy=True)
    P.evaluate_rollout(env, bootstrap=("terminated", "truncated"))
    _refused(lambda: h.onpolicy_prepare(fields=["log_probs"]), S, "log-probabilities")
    h.onpolicy_prepare(fields=["observations", "returns"])
    assert set(h.onpolicy_batch(0, 0, 0, 8)) == {"observations", "returns"}
    env.close()


# ---- 6. caller buffers -----------------------------------------------------------------------------------------------------------------------

class _DeviceBlock:
    """device memory of the test's own (hipMalloc), seen as DeviceArray views"""

    def __init__(self):
        self.hip, self.ptrs = _lib._hip_runtime(), []

    def array(self, shape, dtype):
        p = ctypes.c_void_p()
        nbytes = max(int(np.prod(shape)) * np.dtype(dtype).itemsize, 8)
        assert self.hip.hipMalloc(ctypes.byref(p), ctypes.c_size_t(nbytes)) == 0
        self.ptrs.append(p)
        return _lib.DeviceArray(p.value, shape, np.dtype(dtype).str)

    def free(self):
        for p in self.ptrs:
            self.hip.hipFree(p)
        self.ptrs = []


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("name", ["ieee13-37x5", "ieee123-37x5"])
def test_caller_buffers_and_handle_buffers_hold_the_same_bits(prepared, name, dtype):
    c = prepared(name)
    env, h, n = c["env"], c["env"].handle, 50
    b = OnPolicyBatches(env, n, policy=c["pol"], lambdas=LAMBDAS, adv_norm="minibatch", dtype=dtype, seed=6)
    b.prepare()
    own = _down(h.onpolicy_batch(6, 5, 100, n))
    assert len(own) == 10
    _same(_down(h.onpolicy_batch(6, 5, 100, n)), own)            # a second identical call: the same bits
    mem = _DeviceBlock()
    try:
        out = {k: mem.array((n,), dtype) for k in SCALARS}
        out.update(observations=mem.array((n, env.obs_dim), dtype), actions=mem.array((n, env.action_dim), dtype),
                   indices=mem.array((n,), np.int32), adv_stats=mem.array((2,), np.float64),
                   cost_advantages=[mem.array((n,), dtype), None, mem.array((n,), dtype)], cost_returns=[mem.array((n,), dtype), None, None])
        got = h.onpolicy_batch(6, 5, 100, n, out=out)
        for k in SCALARS + ("observations", "actions", "indices", "adv_stats"):
            assert got[k].ptr == out[k].ptr                      # the caller's memory was used
        assert got["cost_advantages"][0].ptr == out["cost_advantages"][0].ptr and got["cost_returns"][2].ptr not in (0, None)
        _same(_down(got), own)
        if dtype == np.float32 and env.obs_dim % 2 == 0:
            # rows that start 4 bytes into an 8-byte word: the single-column path, the same bits
            raw = mem.array((n * env.obs_dim + 1,), np.float32)
            odd = _lib.DeviceArray(raw.ptr + 4, (n, env.obs_dim), "<f4")
            got = h.onpolicy_batch(6, 5, 100, n, out=dict(observations=odd))
            assert got["observations"].ptr == raw.ptr + 4
            _same(_down(got), own)
    finally:
        mem.free()


# ---- 7. non-interference ---------------------------------------------------------------------------------------------------------------------

def test_batches_leave_no_trace_on_the_environment():
    feeder, B, T = "ieee13", 37, 5
    envs = [_env(feeder, B), _env(feeder, B)]
    for env in envs:
        _collect(env, feeder, T)
    b = OnPolicyBatches(envs[0], 64, policy=_policy(envs[0], feeder, seed=1), lambdas=LAMBDAS, adv_norm="minibatch")
    b.prepare()
    assert sum(len(x["indices"].to_host()) for x in b.epoch(0)) == B * T
    results = []
    for env in envs:
        rollout_device(env, T, seed=21, reset=False, policy=True)
        _evaluate(env, feeder)
        d = env.handle.rollout_download(want=("observations", "actions", "rewards", "next_observations", "terminals", "final_observation"))
        d.update(env.handle.rollout_onpolicy_download(("log_probs", "values", "advantages", "returns")))
        d["state"] = env.get_state()
        results.append(d)
        env.close()
    assert set(results[0]) == set(results[1])
    for k in results[0]:
        assert np.array_equal(results[0][k], results[1][k]), k
