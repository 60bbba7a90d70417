"""The device-resident dataset on the GPU (gs_dataset_*, DeviceGridDataset): statistics against a long-double
reference built from the host download, exact constants, determinism, bit-equal gathers (uploaded and drawn indices, float64 and
float32, raw), the caller's buffers, the state rules, and that nothing of the environment or the rollout moves.

Every case uses episode_length = 7.  Shapes: R = rows_per_chunk is read from the library; N < R, N = R and N = R + 1 are built
from it (R + 1 = 257 is prime for R = 256: that case is B = 1, T = R + 1, which keeps episodes ending inside the rollout where
B = R + 1, T = 1 would not)."""
import ctypes

import numpy as np
import pytest

import grid_fed_rl_gym_amd as P
from grid_fed_rl_gym_amd import _lib

pytestmark = pytest.mark.gpu

FEEDERS = {"ieee13": lambda: P.ieee13_like("epsilon"), "ieee123": P.ieee123_like}
WANT = ("observations", "actions", "rewards", "next_observations", "terminals", "final_observation")
KEYS = ("observations", "actions", "rewards", "next_observations", "terminals")
EPS = 2.0 ** -52
R = 256          # GS_DS_ROWS_PER_CHUNK; every case asserts the library reports it


def _kw(fs, solver):
    return dict(solver=solver, stochastic_loads=True, weather_variation=True, jacobian="exact", tolerance=1e-9,
                max_iterations=100 if solver == "fbs" else 50, power_base=fs.base_power_va, episode_length=7)


# name: (feeder, solver, B, T, per-instance load powers)
CASES = {
    "ieee13-37x5": ("ieee13", "nr", 37, 5, False),                 # obs_dim 71 (odd: the 8-byte path), N = 185 < R
    "ieee123-37x5": ("ieee123", "fbs", 37, 5, False),              # obs_dim 684 (column pairs), N = 185 < R
    "ieee13-5x9": ("ieee13", "nr", 5, 9, False),                   # N = 45 < R with finished episodes
    "ieee13-R": ("ieee13", "nr", R // 8, 8, False),                # N = R exactly
    "ieee13-R+1": ("ieee13", "nr", 1, R + 1, False),               # N = R + 1: a second chunk of one row
    "ieee13-200x33": ("ieee13", "nr", 200, 33, False),             # 26 chunks, ragged tail (N = 6600 = 25 R + 200), two merge launches
    "ieee123-loads-37x9": ("ieee123", "fbs", 37, 9, True),         # load columns differ per instance, constant in time; two chunks
}
_cache = {}


def _case(name):
    """The case's environment after one rollout, its DeviceGridDataset and the host download (made once, shared, left unchanged)."""
    if name not in _cache:
        feeder, solver, B, T, loads = CASES[name]
        fs = FEEDERS[feeder]()
        extra = dict(load_powers=P.randomized_load_powers(fs, B, seed=4, per_load=True)) if loads else {}
        env = P.BatchedGridEnvironment(fs, num_envs=B, **extra, **_kw(fs, solver))
        P.rollout_device(env, T, seed=3)
        ds = P.DeviceGridDataset(env)
        d = env.handle.rollout_download(want=WANT)
        N = T * B
        flat = {k: d[k].reshape((N,) + d[k].shape[2:]) for k in KEYS}
        for v in flat.values():
            v.setflags(write=False)
        obs_full = np.concatenate([flat["observations"], d["final_observation"]], axis=0)       # obs_seq[0 .. T] as rows
        obs_full.setflags(write=False)
        assert ds.rows_per_chunk == R and ds.size == N
        _cache[name] = dict(env=env, ds=ds, flat=flat, obs_full=obs_full, N=N, B=B, T=T, n_terminal=d["n_terminal"])
    return _cache[name]


def _reference(x):
    """mean, population std, max |x| and max |x - mean| per column in long double, on the data shifted by its first row."""
    L = np.asarray(x, dtype=np.longdouble).reshape(x.shape[0], -1)
    L0 = L - L[0]
    m0 = L0.mean(axis=0)
    dev = L0 - m0
    return L[0] + m0, np.sqrt((dev * dev).mean(axis=0)), np.abs(L).max(axis=0), np.abs(dev).max(axis=0)


@pytest.mark.parametrize("name", list(CASES))
def test_statistics_against_the_long_double_reference(name):
    c = _case(name)
    raw, N = c["ds"].raw, c["N"]
    if name in ("ieee13-5x9", "ieee13-R", "ieee13-R+1", "ieee13-200x33", "ieee123-loads-37x9"):
        assert c["n_terminal"] > 0                      # episodes ended inside the rollout
    growth = np.sqrt(np.longdouble(N)) * np.log2(np.longdouble(N))
    for what, x, mean, std in (("observations", c["flat"]["observations"], raw["obs_mean"], raw["obs_std"]),
                               ("actions", c["flat"]["actions"], raw["act_mean"], raw["act_std"]),
                               ("rewards", c["flat"]["rewards"], np.atleast_1d(raw["reward_mean"]), np.atleast_1d(raw["reward_std"]))):
        ref_mean, ref_std, amax, dmax = _reference(x)
        assert mean.shape == ref_mean.shape and np.isfinite(mean).all() and np.isfinite(std).all() and (std >= 0).all()
        err_mean, err_std = np.abs(mean.astype(np.longdouble) - ref_mean), np.abs(std.astype(np.longdouble) - ref_std)
        tol_mean, tol_std = EPS * (amax + growth * dmax), EPS * growth * dmax
        with np.errstate(divide="ignore", invalid="ignore"):
            worst_m = np.nanmax(np.where(tol_mean > 0, err_mean / tol_mean, np.where(err_mean > 0, np.inf, 0)))
            worst_s = np.nanmax(np.where(tol_std > 0, err_std / tol_std, np.where(err_std > 0, np.inf, 0)))
        print(f"{name} {what}: worst mean error / bound {float(worst_m):.3f}, worst std error / bound {float(worst_s):.3f}")
        bad = np.flatnonzero(err_mean > tol_mean)
        assert bad.size == 0, (what, "mean", bad[:8], err_mean[bad[:8]], tol_mean[bad[:8]])
        bad = np.flatnonzero(err_std > tol_std)
        assert bad.size == 0, (what, "std", bad[:8], err_std[bad[:8]], tol_std[bad[:8]])


@pytest.mark.parametrize("name", list(CASES))
def test_constant_columns_are_exact(name):
    c = _case(name)
    obs, ds = c["flat"]["observations"], c["ds"]
    const = (obs.view(np.uint64) == obs[0].view(np.uint64)).all(axis=0)          # bit-equal down the column
    assert np.array_equal(ds.raw["obs_mean"][const].view(np.uint64), obs[0][const].view(np.uint64))
    assert (ds.raw["obs_std"][const] == 0.0).all()
    assert np.array_equal(ds.constant_columns, const)
    assert np.array_equal(ds.policy_obs_std, np.where(const, 1.0, ds.raw["obs_std"] + 1e-6))
    print(f"{name}: {int(const.sum())} of {const.size} columns are constant")
    if name == "ieee123-37x5":
        assert const.any()               # the shared static load powers are among them


@pytest.mark.parametrize("name", ["ieee13-200x33", "ieee123-loads-37x9"])
def test_a_second_build_gives_the_same_bits(name):
    c = _case(name)
    h = c["env"].handle
    first = h.dataset_stats()
    h.dataset_build()
    second = h.dataset_stats()
    for k in ("obs_mean", "obs_std", "act_mean", "act_std"):
        assert np.array_equal(first[k].view(np.uint64), second[k].view(np.uint64)), k
    assert first["reward_mean"] == second["reward_mean"] and first["reward_std"] == second["reward_std"]


def _expected(c, idx, normalize=True):
    """The batch NumPy makes of the download with the device's own statistics: (x - mean) / (std + 1e-6)."""
    f, raw = c["flat"], c["ds"].raw
    out = {k: f[k][idx] for k in ("observations", "actions", "rewards", "next_observations")}
    if normalize:
        out["observations"] = (out["observations"] - raw["obs_mean"]) / (raw["obs_std"] + 1e-6)
        out["next_observations"] = (out["next_observations"] - raw["obs_mean"]) / (raw["obs_std"] + 1e-6)
        out["actions"] = (out["actions"] - raw["act_mean"]) / (raw["act_std"] + 1e-6)
        out["rewards"] = (out["rewards"] - raw["reward_mean"]) / (raw["reward_std"] + 1e-6)
    out["terminals"] = ((f["terminals"][idx] & 3) != 0).astype(np.float64)
    return out


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _assert_batch(got, want, dtype=np.float64):
    for k in KEYS:
        g = got[k].to_host() if hasattr(got[k], "to_host") else got[k]
        w = want[k].astype(dtype)
        assert g.dtype == np.dtype(dtype) and g.shape == w.shape, (k, g.dtype, g.shape, w.shape)
        assert np.array_equal(_bits(g), _bits(w)), (k, int((_bits(g) != _bits(w)).sum()))


def _probe_indices(c):
    """0, N - 1, duplicates, every transition that ended an episode and each one's successor; a length that is no multiple of the
    gather's four rows per workgroup."""
    N, B = c["N"], c["B"]
    term = np.flatnonzero(c["flat"]["terminals"] != 0)
    assert term.size == c["n_terminal"] > 0
    succ = term + B
    idx = np.concatenate([[0, N - 1, 0, N - 1, N // 2, N // 2], term, succ[succ < N], term[:3]]).astype(np.int64)
    while idx.size % 4 != 3:
        idx = np.append(idx, idx.size % N)
    return idx, term


@pytest.mark.parametrize("name", ["ieee13-200x33", "ieee123-loads-37x9", "ieee13-R+1"])
def test_gather_with_uploaded_indices_is_bit_equal_to_numpy(name):
    c = _case(name)
    ds, N, B = c["ds"], c["N"], c["B"]
    idx, term = _probe_indices(c)
    _assert_batch(ds.sample_batch(idx.size, indices=idx), _expected(c, idx))
    _assert_batch(ds.sample_batch(idx.size, indices=idx, dtype=np.float32), _expected(c, idx), np.float32)
    _assert_batch(c["env"].handle.dataset_sample(idx.size, indices=idx, normalize=False), _expected(c, idx, normalize=False))
    _assert_batch(c["env"].handle.dataset_sample(idx.size, indices=idx, normalize=False, dtype=np.float32), _expected(c, idx, normalize=False), np.float32)
    # the terminal observation is NOT the row that follows in the sequence (the fresh observation after the reset): a gather without
    # the map would fail the comparison above
    raw = ds.raw
    nxt = ds.sample_batch(term.size, indices=term)["next_observations"].to_host()
    follows = (c["obs_full"][term + B] - raw["obs_mean"]) / (raw["obs_std"] + 1e-6)
    assert (nxt != follows).any(axis=1).all()
    for one in (0, N - 1, int(term[0])):
        _assert_batch(ds.sample_batch(1, indices=[one]), _expected(c, np.array([one])))


@pytest.mark.parametrize("name", ["ieee13-200x33", "ieee123-loads-37x9"])
def test_gather_with_drawn_indices_follows_the_philox_contract(name):
    c = _case(name)
    ds = P.DeviceGridDataset(c["env"])                 # a dataset of its own: the draw counter starts at 0
    for draw in range(3):
        for n in ((257, 5, 1)[draw],):
            got = ds.sample_batch(n, seed=5)
            idx = P.DeviceGridDataset.indices_np(5, draw, n, c["N"])
            _assert_batch(got, _expected(c, idx))
    assert np.array_equal(ds.raw["obs_mean"], c["ds"].raw["obs_mean"])
    got = c["env"].handle.dataset_sample(6, seed=(9 << 32) + 1, draw=(1 << 32) + 2, dtype=np.float32)      # high words of seed and draw
    _assert_batch(got, _expected(c, P.DeviceGridDataset.indices_np((9 << 32) + 1, (1 << 32) + 2, 6, c["N"])), np.float32)


@pytest.mark.parametrize("name", ["ieee13-200x33", "ieee123-loads-37x9"])
def test_the_callers_tensors_receive_the_batch(name):
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("torch without a GPU")
    c = _case(name)
    ds, env = c["ds"], c["env"]
    idx, _ = _probe_indices(c)
    n, D, A = idx.size, env.handle.obs_dim, env.handle.action_dim
    for dtype, tdtype in ((np.float64, torch.float64), (np.float32, torch.float32)):
        out = dict(observations=torch.full((n, D), 7.0, dtype=tdtype, device="cuda"), actions=torch.full((n, A), 7.0, dtype=tdtype, device="cuda"),
                   rewards=torch.full((n,), 7.0, dtype=tdtype, device="cuda"), next_observations=torch.full((n, D), 7.0, dtype=tdtype, device="cuda"),
                   terminals=torch.full((n,), 7.0, dtype=tdtype, device="cuda"))
        b = ds.sample_batch(n, indices=idx, dtype=dtype, out=out, stream=torch.cuda.current_stream().cuda_stream)
        assert all(b[k].ptr == out[k].data_ptr() for k in KEYS)
        _assert_batch({k: out[k].cpu().numpy() for k in KEYS}, _expected(c, idx), dtype)
    # some of the caller's, the rest the handle's; and a zero-copy view of the handle's buffer
    obs = torch.zeros((n, D), dtype=torch.float64, device="cuda")
    b = ds.sample_batch(n, indices=idx, out=dict(observations=obs))
    want = _expected(c, idx)
    assert b["observations"].ptr == obs.data_ptr() and b["rewards"].ptr != 0
    assert np.array_equal(obs.cpu().numpy(), want["observations"])
    assert np.array_equal(torch.as_tensor(b["next_observations"], device="cuda").cpu().numpy(), want["next_observations"])
    with pytest.raises(P.PowerFlowError):
        ds.sample_batch(n, indices=idx, out=dict(observations=obs[:, :-1]))
    with pytest.raises(P.PowerFlowError):
        ds.sample_batch(n, indices=idx, dtype=np.float32, out=dict(observations=obs))


def _sample_rc(h, n, idx=None):
    b = _lib.gs_dataset_batch()
    a = None if idx is None else np.ascontiguousarray(idx, dtype=np.int64)
    rc = h._lib.gs_dataset_sample(h._h, n, None if a is None else a.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), 0, 0, 0, 1, ctypes.byref(b), None)
    return rc, b


def test_state_rules():
    fs = FEEDERS["ieee13"]()
    B, T = 6, 9
    env = P.BatchedGridEnvironment(fs, num_envs=B, **_kw(fs, "nr"))
    h = env.handle
    env.reset(seed=1)
    assert h._lib.gs_dataset_build(h._h, 0) == _lib.GS_E_STATE                       # no rollout
    P.rollout_device(env, T, seed=1)
    assert _sample_rc(h, 4)[0] == _lib.GS_E_STATE and "gs_dataset_build" in h.last_error()   # before a build
    assert h._lib.gs_dataset_build(h._h, _lib.GS_DATASET_KEEP_STATS) == _lib.GS_E_STATE        # nothing to keep
    assert h._lib.gs_dataset_build(h._h, 2) == _lib.GS_E_INVALID
    ds = P.DeviceGridDataset(env)
    N = T * B
    first = ds.sample_batch(5, indices=[0, 1, 2, 3, N - 1])
    before = {k: first[k].to_host() for k in KEYS}
    for bad in (N, -1):                                                             # refused before anything is launched
        rc, _ = _sample_rc(h, 5, [0, 1, bad, 3, 4])
        assert rc == _lib.GS_E_INVALID and "outside" in h.last_error()
        for k in KEYS:
            assert np.array_equal(first[k].to_host(), before[k]), k
    # refused statistics leave the installed ones in place
    raw = dict(ds.raw)
    args = [raw["obs_mean"], raw["obs_std"], raw["act_mean"], raw["act_std"], raw["reward_mean"], raw["reward_std"]]
    with pytest.raises(P.PowerFlowError, match="do not match"):
        h.dataset_set_stats(args[0][:-1], args[1][:-1], *args[2:])
    with pytest.raises(P.PowerFlowError, match="do not match"):
        h.dataset_set_stats(args[0], args[1], args[2][:-1], args[3][:-1], *args[4:])
    nan = raw["obs_std"].copy(); nan[3] = np.nan
    with pytest.raises(P.PowerFlowError, match="not finite"):
        h.dataset_set_stats(args[0], nan, *args[2:])
    with pytest.raises(P.PowerFlowError, match="not finite"):
        h.dataset_set_stats(*args[:5], np.inf)
    again = h.dataset_stats()
    for k in ("obs_mean", "obs_std", "act_mean", "act_std"):
        assert np.array_equal(again[k].view(np.uint64), raw[k].view(np.uint64)), k
    assert again["reward_mean"] == raw["reward_mean"] and again["reward_std"] == raw["reward_std"]
    for k in KEYS:
        assert np.array_equal(ds.sample_batch(5, indices=[0, 1, 2, 3, N - 1])[k].to_host(), before[k]), k
    # a further rollout: the dataset is stale until it is rebuilt; keep_stats keeps the statistics bit for bit and serves the new terminals
    P.rollout_device(env, T, seed=2, reset=False)
    assert _sample_rc(h, 4)[0] == _lib.GS_E_STATE and "earlier rollout" in h.last_error()
    v = _lib.gs_dataset_stats_view(ctypes.sizeof(_lib.gs_dataset_stats_view))
    assert h._lib.gs_dataset_stats(h._h, ctypes.byref(v)) == _lib.GS_E_STATE
    ds.rebuild(keep_stats=True)
    for k in ("obs_mean", "obs_std", "act_mean", "act_std"):
        assert np.array_equal(ds.raw[k].view(np.uint64), raw[k].view(np.uint64)), k
    assert ds.raw["reward_mean"] == raw["reward_mean"] and ds.raw["reward_std"] == raw["reward_std"]
    d = h.rollout_download(want=WANT)
    flat = {k: d[k].reshape((N,) + d[k].shape[2:]) for k in KEYS}
    c = dict(flat=flat, ds=ds, N=N, B=B, n_terminal=d["n_terminal"])
    idx, term = _probe_indices(c)
    _assert_batch(ds.sample_batch(idx.size, indices=idx), _expected(c, idx))
    # installed statistics normalise the next batch; a rebuild replaces them with the new rollout's
    ds.set_stats(raw["obs_mean"] + 1.0, raw["obs_std"] * 2.0, raw["act_mean"], raw["act_std"], 0.5, 2.0)
    assert ds.raw["reward_mean"] == 0.5 and ds.raw["reward_std"] == 2.0 and np.array_equal(ds.raw["obs_mean"], raw["obs_mean"] + 1.0)
    _assert_batch(ds.sample_batch(idx.size, indices=idx), _expected(c, idx))
    ds.rebuild()
    assert ds.raw["reward_std"] != 2.0
    _assert_batch(ds.sample_batch(idx.size, indices=idx), _expected(c, idx))
    # a longer rollout reallocates the collection: the kept statistics survive it
    kept = dict(ds.raw)
    P.rollout_device(env, 2 * T, seed=3, reset=False)
    ds.rebuild(keep_stats=True)
    assert ds.size == 2 * N and np.array_equal(ds.raw["obs_std"].view(np.uint64), kept["obs_std"].view(np.uint64))
    env.close()


def test_nothing_else_moves():
    """A rollout followed by a build and samples leaves the environment's state and the rollout's buffers bit-identical to those of
    a handle that only rolled out."""
    fs = FEEDERS["ieee123"]()
    B, T = 9, 10
    envs = [P.BatchedGridEnvironment(fs, num_envs=B, **_kw(fs, "fbs")) for _ in range(2)]
    for env in envs:
        P.rollout_device(env, T, seed=6)
    ds = P.DeviceGridDataset(envs[0])
    ds.sample_batch(33, seed=1)
    ds.sample_batch(7, indices=np.arange(7), dtype=np.float32)
    ds.rebuild()
    a, b = (env.handle.rollout_download(want=WANT) for env in envs)
    for k in WANT:
        assert np.array_equal(a[k], b[k]), k
    assert a["n_terminal"] == b["n_terminal"] > 0
    assert np.array_equal(envs[0].handle.get_state().view(np.uint64), envs[1].handle.get_state().view(np.uint64))
    for env in envs:                                   # and both go on identically
        P.rollout_device(env, 3, seed=7, reset=False)
    a, b = (env.handle.rollout_download(want=WANT) for env in envs)
    for k in WANT:
        assert np.array_equal(a[k], b[k]), k
    for env in envs:
        env.close()
