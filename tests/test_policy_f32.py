"""CPU-only: the float32 compute path of the MLP policy (GS_COMPUTE_F32) as far as it lives on the host -- the rules of
gs_policy_mlp_opts (gs_policy_mlp_check_opts), the declared / exported / bound entry points, and MLPPolicy's NumPy restatement
of the device contract (forward_np(compute="float32")) against a torch float32 nn.Sequential built the way the reference builds
its actors (algorithms/base.py:157-177; head: algorithms/offline.py:69-76).

Tolerance rule.  E_ref is the largest absolute difference, on a test's own policy and observations, between two NumPy
evaluations: the float32 forward_np and the float64 evaluation of the SAME float32-rounded operands (forward_np(...,
exact=True)).  It is a property of float32 arithmetic on that data and is computed from NumPy alone.  Two float32 evaluations of
one network that differ only in the order of their sums (NumPy's matmul, torch's, the device's) are each about E_ref from the
exact value, with rounding errors of random sign, so they are held to 4 E_ref of the exact value or of each other; the same
factor 4 is the one the GPU tests use.  The size E_ref may have is bounded from the format: unit roundoff 2^-24 = 6e-8, random
signs over a chain of K <= 684 terms of size O(1 / sqrt(K)) ... O(1) grow like sqrt(K) <= 26, so 1.6e-6 per layer and, through three
1-Lipschitz layers, below 1e-5."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import grid_fed_rl_gym_amd as P
from grid_fed_rl_gym_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBS, A = 684, 8        # the 123-bus feeder's observation and action widths
E_REF_MAX = 1e-5       # (module docstring)


def _net(dims, seed=0):
    rng = np.random.default_rng(seed)
    ws = [rng.normal(0.0, 1.0 / np.sqrt(dims[l]), (dims[l + 1], dims[l])) for l in range(len(dims) - 1)]
    bs = [rng.normal(0.0, 0.1, dims[l + 1]) for l in range(len(dims) - 1)]
    return ws, bs


def _check(ws, bs, opts_kw=None, obs_dim=OBS, action_dim=A, **kw):
    p, keep = _lib.policy_struct(ws, bs, **kw)
    o, keep_o = (None, None) if opts_kw is None else _lib.policy_opts(**opts_kw)
    return _lib.policy_check_opts(p, o, obs_dim, action_dim)


def _e_ref(pol, obs, eps=None):
    return float(np.max(np.abs(pol.forward_np(obs, eps, compute="float32") - pol.forward_np(obs, eps, compute="float32", exact=True))))


def test_check_opts_accepts_the_reference_shaped_networks():
    shift, scale = np.linspace(-1.0, 1.0, OBS), np.linspace(0.5, 2.0, OBS)
    for dims, head in (([OBS, 256, 256, 2 * A], "gaussian_tanh"), ([OBS, 256, 256, 256, 2 * A], "gaussian_tanh"), ([OBS, 256, 256, A], "tanh")):
        for opts in (None, dict(compute="float64"), dict(compute="float32"), dict(compute="float32", obs_shift=shift, obs_scale=scale),
                     dict(compute="float32", obs_shift=shift), dict(compute="float32", obs_scale=scale)):
            rc, msg = _check(*_net(dims), opts_kw=opts, head=head)
            assert rc == _lib.GS_OK, (opts, msg)


def test_check_opts_refuses_what_the_rules_forbid():
    def refused(match, *a, **kw):
        rc, msg = _check(*a, **kw)
        assert rc == _lib.GS_E_INVALID and re.search(match, msg), (rc, msg)
    dims = [OBS, 256, 256, 2 * A]
    ones = np.ones(OBS)
    refused(r"gs_policy_mlp_opts struct_size 16", *_net(dims), opts_kw=dict(compute="float32", struct_size=16))
    refused(r"unknown compute 2", *_net(dims), opts_kw=dict(compute=2))
    refused(r"unknown compute -1", *_net(dims), opts_kw=dict(compute=-1))
    refused(r"GS_COMPUTE_F32.*fold", *_net(dims), opts_kw=dict(compute="float64", obs_shift=ones, obs_scale=ones))
    refused(r"GS_COMPUTE_F32.*fold", *_net(dims), opts_kw=dict(compute="float64", obs_scale=ones))
    bad = ones.copy()
    bad[17] = np.nan
    refused(r"obs_scale\[17\] is not finite", *_net(dims), opts_kw=dict(compute="float32", obs_shift=ones, obs_scale=bad))
    bad[17] = np.inf
    refused(r"obs_shift\[17\] is not finite", *_net(dims), opts_kw=dict(compute="float32", obs_shift=bad, obs_scale=ones))
    ws, bs = _net(dims)
    ws[1][3, 5] = 1e39                                                     # finite in float64, infinite in float32
    refused(r"weights\[1\].*not finite in float32.*row 3, column 5", ws, bs, opts_kw=dict(compute="float32"))
    assert _check(ws, bs, opts_kw=dict(compute="float64"))[0] == _lib.GS_OK       # (the float64 path takes it)
    ws, bs = _net(dims)
    bs[2][1] = -1e39
    refused(r"biases\[2\]\[1\] is not finite in float32", ws, bs, opts_kw=dict(compute="float32"))
    ws, bs = _net(dims)
    ws[0][0, 0] = float(np.finfo(np.float32).max) * (1.0 + 2.0 ** -26)     # rounds DOWN to FLT_MAX: still finite
    assert _check(ws, bs, opts_kw=dict(compute="float32"))[0] == _lib.GS_OK
    # the rules of gs_policy_mlp come first, with their own messages
    refused(r"dims\[0\]", *_net([OBS + 1, 256, 2 * A]), opts_kw=dict(compute="float32"))
    ws, bs = _net(dims)
    ws[1][3, 5] = np.nan
    refused(r"non-finite", ws, bs, opts_kw=dict(compute="float32"))


def test_null_opts_agree_with_gs_policy_mlp_check():
    lib = _lib.load()
    cases = [(_net([OBS, 256, 256, 2 * A]), dict()), (_net([OBS + 1, 256, 2 * A]), dict()), (_net([OBS, 256, A]), dict(head="tanh", stochastic=True)),
             (_net([OBS, 257, 2 * A]), dict()), (_net([OBS, 256, 2 * A]), dict(n_layers=5))]
    for (ws, bs), kw in cases:
        p, keep = _lib.policy_struct(ws, bs, **kw)
        rc0, msg0 = _lib.policy_check(p, OBS, A)
        rc1, msg1 = _lib.policy_check_opts(p, None, OBS, A)
        assert (rc0, msg0) == (rc1, msg1)
    assert lib.gs_policy_mlp_check_opts(None, None, OBS, A) == _lib.GS_E_INVALID


def test_header_exports_and_bindings_agree_on_the_new_entry_points():
    src = open(os.path.join(ROOT, "include", "gridstep.h")).read()
    lib = _lib.load()
    bound = {name: args for name, _, args in _lib.SYMBOLS}
    for name in ("gs_policy_mlp_check_opts", "gs_policy_mlp_set_opts"):
        assert re.search(r"\bint %s\s*\(" % name, src), name
        assert hasattr(lib, name) and name in bound, name
    assert len(bound["gs_policy_mlp_check_opts"]) == 4 and len(bound["gs_policy_mlp_set_opts"]) == 3
    for k, v in (("GS_COMPUTE_F64", 0), ("GS_COMPUTE_F32", 1)):
        assert re.search(r"\b%s\s*=\s*%d\b" % (k, v), src), k
    assert _lib.COMPUTE == {"float64": 0, "float32": 1}
    assert ctypes.sizeof(_lib.gs_policy_mlp_opts) == 24                    # 2 int32, then 2 pointers
    assert [f[0] for f in _lib.gs_policy_mlp_opts._fields_] == ["struct_size", "compute", "obs_shift", "obs_scale"]
    body = re.search(r"typedef struct gs_policy_mlp_opts \{(.*?)\} gs_policy_mlp_opts;", src, flags=re.S).group(1)
    assert re.findall(r"\b(struct_size|compute|obs_shift|obs_scale);", body) == ["struct_size", "compute", "obs_shift", "obs_scale"]
    assert ctypes.sizeof(_lib.gs_policy_mlp) == 10 * 4 + 8 * 8             # (unchanged)
    assert lib.gs_version() == _lib.GS_ABI_VERSION


def _torch_net(dims, act, seed):
    torch = pytest.importorskip("torch")
    nn = torch.nn
    torch.manual_seed(seed)
    layers = []
    for i in range(len(dims) - 1):                                         # _build_mlp, algorithms/base.py:166-177
        layers.append(nn.Linear(dims[i], dims[i + 1]))
        if i < len(dims) - 2:
            layers.append({"relu": nn.ReLU, "tanh": nn.Tanh, "elu": nn.ELU}[act]())
    return torch, nn.Sequential(*layers)                                   # the default dtype: float32


@pytest.mark.parametrize("act", ["relu", "tanh", "elu"])
@pytest.mark.parametrize("head", ["tanh", "gaussian_tanh"])
@pytest.mark.parametrize("normalise", [False, True])
def test_forward_np_float32_agrees_with_torch_float32(act, head, normalise):
    obs_dim, a, rows = 60, 5, 256
    torch, net = _torch_net([obs_dim, 48, 40, 2 * a if head == "gaussian_tanh" else a], act, seed=3)
    assert next(net.parameters()).dtype == torch.float32
    rng = np.random.default_rng(5)
    obs = rng.normal(2.0, 3.0, (rows, obs_dim))
    mean, std = (obs.mean(axis=0), obs.std(axis=0) + 1e-6) if normalise else (None, None)
    pol = P.MLPPolicy.from_sequential(net, head=head, obs_mean=mean, obs_std=std, compute="float32")
    assert (pol.obs_dim, pol.action_dim, pol.activation, pol.head, pol.compute) == (obs_dim, a, act, head, "float32")
    z = pol.normalise_f32(obs)
    assert z.dtype == np.float32
    if normalise:
        assert np.array_equal(z, ((obs - mean) * (1.0 / std)).astype(np.float32))
    eps = rng.normal(size=(rows, a))
    with torch.no_grad():
        out = net(torch.from_numpy(z)).double()                            # the head in float64 on the float32 pre-head values
        if head == "tanh":
            want_det, want_sto = torch.tanh(out).numpy(), None
        else:
            m, ls = torch.chunk(out, 2, dim=-1)                            # algorithms/offline.py:69-76
            want_det = torch.tanh(m).numpy()
            want_sto = torch.tanh(m + torch.clamp(ls, -20, 2).exp() * torch.from_numpy(eps)).numpy()
    e_ref = _e_ref(pol, obs)
    err = float(np.max(np.abs(pol.forward_np(obs) - want_det)))
    print("E_ref", e_ref, "max |forward_np float32 - torch float32|", err)
    assert 0.0 < e_ref <= E_REF_MAX
    assert err <= 4.0 * e_ref
    assert np.array_equal(pol.forward_np(obs), pol.forward_np(obs, compute="float32"))        # (compute defaults to the policy's own)
    if want_sto is not None:
        e_sto = _e_ref(pol, obs, eps)
        assert np.max(np.abs(pol.forward_np(obs, eps) - want_sto)) <= 4.0 * e_sto
    # the float64 restatement of the same policy is what it was: the folded float64 network
    p64 = P.MLPPolicy.from_sequential(net, head=head, obs_mean=mean, obs_std=std)
    assert p64.compute == "float64" and np.array_equal(p64.forward_np(obs), pol.forward_np(obs, compute="float64"))


def _constant_column_case(rows=512, seed=7):
    """An observation block like the 123-bus feeder's: 250 columns that do not vary at all and sit at 1e5 (the static load powers,
    in watts), normalised with std = 1 as tests/test_gpu_policy.py sets them; the others O(1) around O(1) means."""
    rng = np.random.default_rng(seed)
    dims = [OBS, 256, 256, 2 * A]
    ws, bs = _net(dims, seed=seed)
    const = np.zeros(OBS, dtype=bool)
    const[300:550] = True
    level = rng.uniform(0.5e5, 1.5e5, OBS)
    obs = rng.normal(1.0, 2.0, (rows, OBS))
    obs[:, const] = level[const]
    mean, std = obs.mean(axis=0), obs.std(axis=0)
    constant = std <= 1e-12 * np.maximum(1.0, np.abs(mean))
    assert np.array_equal(constant, const)
    std = np.where(constant, 1.0, std + 1e-6)
    # the rows the policy is asked about: the varying columns redrawn, the constant ones a few watts off their mean
    ask = rng.normal(1.0, 2.0, (rows, OBS))
    ask[:, const] = level[const] + rng.normal(0.0, 3.0, (rows, int(const.sum())))
    return ws, bs, mean, std, ask


def test_normalisation_stage_is_what_keeps_float32_accurate():
    ws, bs, mean, std, obs = _constant_column_case()
    pol = P.MLPPolicy(ws, bs, obs_mean=mean, obs_std=std, compute="float32")
    assert np.array_equal(pol.weight0, ws[0]) and np.array_equal(pol.obs_mean, mean) and np.array_equal(pol.obs_std, std)
    exact = pol.forward_np(obs, exact=True)
    e_ref = _e_ref(pol, obs)
    assert float(np.mean(np.abs(exact) < 0.99)) >= 0.5
    assert 0.0 < e_ref <= E_REF_MAX
    # (a) the explicit stage: rounding the OPERANDS to float32 moves the policy no further from the float64 network than the
    # float32 arithmetic itself does -- every rounding is relative 2^-24 on an O(1) quantity, the model E_ref is built on
    full = pol.forward_np(obs, compute="float64")
    err_stage = float(np.max(np.abs(pol.forward_np(obs) - full)))
    # (b) the fold pushed through float32: folded weights, raw observations, everything rounded to float32
    x = np.asarray(obs, dtype=np.float32)
    for l, (w, b) in enumerate(zip(pol.weights, pol.biases)):
        x = x @ w.astype(np.float32).T + b.astype(np.float32)
        if l < 2:
            x = np.maximum(x, np.float32(0))
    err_fold = float(np.max(np.abs(np.tanh(x[:, :A].astype(np.float64)) - full)))
    print("E_ref", e_ref, "explicit stage vs float64 network", err_stage, "folded through float32 vs float64 network", err_fold)
    assert err_stage <= 4.0 * e_ref
    assert err_fold > 4.0 * e_ref
    assert err_fold > 100.0 * err_stage        # a 1e5-watt entry rounds at 2^-24 * 1e5 = 6e-3 W: not a matter of a factor


def test_from_sequential_float32_widening_is_lossless():
    torch, net = _torch_net([20, 16, 12, 6], "tanh", seed=1)
    pol = P.MLPPolicy.from_sequential(net, head="gaussian_tanh", compute="float32")
    lin = [m for m in net if hasattr(m, "weight")]
    ws = [pol.weight0] + pol.weights[1:]
    bs = [pol.bias0] + pol.biases[1:]
    for w, b, m in zip(ws, bs, lin):
        assert w.dtype == np.float64
        assert np.array_equal(w.astype(np.float32), m.weight.detach().numpy()) and np.array_equal(w, m.weight.detach().numpy().astype(np.float64))
        assert np.array_equal(b.astype(np.float32), m.bias.detach().numpy()) and np.array_equal(b, m.bias.detach().numpy().astype(np.float64))
    # ... so the float32 path evaluates the module's own numbers: bit for bit the NumPy float32 evaluation of its arrays
    obs = np.random.default_rng(0).normal(size=(64, 20))
    x = obs.astype(np.float32)
    for l, m in enumerate(lin):
        x = x @ m.weight.detach().numpy().T + m.bias.detach().numpy()
        if l < len(lin) - 1:
            x = np.tanh(x)
    assert x.dtype == np.float32
    assert np.array_equal(pol.forward_np(obs), np.tanh(x[:, :3].astype(np.float64)))
    p, keep = pol.to_struct()
    o, keep_o = pol.to_opts()
    assert o.compute == 1 and not o.obs_shift and not o.obs_scale and o.struct_size == 24
    rc, msg = _lib.policy_check_opts(p, o, 20, 3)
    assert rc == _lib.GS_OK, msg


def test_policy_hands_over_unfolded_weights_and_the_normalisation():
    ws, bs, mean, std, obs = _constant_column_case(rows=8)
    p32 = P.MLPPolicy(ws, bs, obs_mean=mean, obs_std=std, compute="float32")
    p64 = P.MLPPolicy(ws, bs, obs_mean=mean, obs_std=std)
    # weights / biases keep their meaning (folded, float64) on both
    for a, b in zip(p32.weights + p32.biases, p64.weights + p64.biases):
        assert np.array_equal(a, b)
    assert np.array_equal(p64.weights[0], ws[0] / std[None, :]) and p64.to_opts() == (None, None)
    s32, keep32 = p32.to_struct()
    o32, keep_o = p32.to_opts()
    assert np.array_equal(keep32["w"][0], ws[0]) and np.array_equal(keep32["b"][0], bs[0])
    assert np.array_equal(keep_o["shift"], mean) and np.array_equal(keep_o["scale"], 1.0 / std)
    s64, keep64 = p64.to_struct()
    assert np.array_equal(keep64["w"][0], p64.weights[0])
    assert _lib.policy_check_opts(s32, o32, OBS, A)[0] == _lib.GS_OK
    with pytest.raises(ValueError, match="compute"):
        P.MLPPolicy(ws, bs, compute="bfloat16")
    with pytest.raises(ValueError, match="exact"):
        p64.forward_np(obs, exact=True)
    assert math.isfinite(float(np.max(np.abs(p32.forward_np(obs)))))
