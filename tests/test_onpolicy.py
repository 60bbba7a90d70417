"""CPU-only: the host side of on-policy rollouts (include/gridstep.h) -- the rules of gs_value_mlp_check one by
one, MLPPolicy.log_prob_np against torch.distributions, and gae_np against the definition of generalised advantage estimation."""
import math

import numpy as np
import pytest

import grid_fed_rl_gym_amd as P
from grid_fed_rl_gym_amd import _lib

OBS_DIM = 23


def _layers(dims, seed=0):
    rng = np.random.default_rng(seed)
    ws = [rng.normal(0.0, 1.0 / math.sqrt(dims[l]), (dims[l + 1], dims[l])) for l in range(len(dims) - 1)]
    bs = [rng.normal(0.0, 0.1, dims[l + 1]) for l in range(len(dims) - 1)]
    return ws, bs


def _value_struct(dims=(OBS_DIM, 17, 1), head=_lib.GS_HEAD_LINEAR, stochastic=False, poke=None):
    ws, bs = _layers(list(dims))
    if poke is not None:
        poke(ws, bs)
    return _lib.policy_struct(ws, bs, "relu", head, stochastic)


def test_value_check_accepts_a_critic_and_refuses_each_broken_rule():
    f32, keep32 = _lib.policy_opts("float32")
    f64, keep64 = _lib.policy_opts("float64")
    p, keep = _value_struct()
    assert _lib.value_check(p, f32, OBS_DIM) == (_lib.GS_OK, "")
    p1, keep1 = _value_struct(dims=(OBS_DIM, 1))                # a direct obs -> 1
    assert _lib.value_check(p1, f32, OBS_DIM)[0] == _lib.GS_OK

    def refused(p, o, word, obs_dim=OBS_DIM):
        rc, msg = _lib.value_check(p, o, obs_dim)
        assert rc == _lib.GS_E_INVALID and word in msg, (rc, msg)

    for head in ("tanh", "gaussian_tanh"):                      # wrong head
        q, k = _value_struct(head=head)
        refused(q, f32, "GS_HEAD_LINEAR")
    q, k = _value_struct(dims=(OBS_DIM, 17, 2))                 # last width != 1
    refused(q, f32, "last width")
    refused(p, f64, "GS_COMPUTE_F32")                           # float64 compute
    refused(p, None, "GS_COMPUTE_F32")                          # (no options: float64 is the default)

    def nan_weight(ws, bs):
        ws[1][0, 3] = np.nan
    q, k = _value_struct(poke=nan_weight)                       # a non-finite weight
    refused(q, f32, "non-finite")

    def inf_bias(ws, bs):
        bs[0][2] = np.inf
    q, k = _value_struct(poke=inf_bias)
    refused(q, f32, "not finite")
    q, k = _value_struct(stochastic=True)                       # stochastic = 1
    refused(q, f32, "stochastic")
    refused(p, f32, "obs_dim", obs_dim=OBS_DIM + 1)             # (and the policy's own rules still hold)
    # the policy slot keeps refusing the linear head
    rc, msg = _lib.policy_check_opts(p, f32, OBS_DIM, 1)
    assert rc == _lib.GS_E_INVALID and "head" in msg


def test_mlp_value_forward_and_struct():
    ws, bs = _layers([OBS_DIM, 9, 1], seed=3)
    rng = np.random.default_rng(1)
    mean, std = rng.normal(size=OBS_DIM), rng.uniform(0.5, 2.0, OBS_DIM)
    v = P.MLPValue(ws, bs, activation="tanh", obs_mean=mean, obs_std=std)
    obs = rng.normal(size=(4, 6, OBS_DIM))
    z = (obs - mean) * (1.0 / std)
    h = np.tanh(z.astype(np.float32).astype(np.float64) @ ws[0].astype(np.float32).astype(np.float64).T + bs[0].astype(np.float32))
    want = (h @ ws[1].astype(np.float32).astype(np.float64).T + bs[1].astype(np.float32))[..., 0]
    got = v.forward_np(obs, exact=True)
    assert got.shape == (4, 6) and got.dtype == np.float64
    np.testing.assert_allclose(got, want, rtol=1e-13, atol=1e-15)
    f32 = v.forward_np(obs)
    assert np.max(np.abs(f32 - got)) < 1e-5 and not np.array_equal(f32, got)
    p, keep = v.to_struct()
    o, keep_o = v.to_opts()
    assert p.head == _lib.GS_HEAD_LINEAR and o.compute == _lib.COMPUTE["float32"]
    assert _lib.value_check(p, o, OBS_DIM) == (_lib.GS_OK, "")
    with pytest.raises(ValueError):
        P.MLPValue(*_layers([OBS_DIM, 9, 2]))


def test_log_prob_np_is_the_normal_log_prob_with_the_tanh_correction():
    """Held to rtol 1e-12 of the torch result, row by row.  Looser only for rows where some |x| > 3: there 1 - a^2 < 1e-2
    cancels, and torch's tanh and NumPy's may each be an ulp (1.1e-16) off, which moves 1 - a^2 by up to 2 |a| 2.2e-16 and the
    logarithm by 4.4e-16 / (1 - a^2 + 1e-6); such a row gets that much more for each of its actions with |x| > 3, and nothing
    else."""
    torch = pytest.importorskip("torch")
    A = 6
    ws, bs = _layers([OBS_DIM, 32, 32, 2 * A], seed=5)
    pol = P.MLPPolicy(ws, bs, activation="tanh")
    rng = np.random.default_rng(2)
    obs, eps = rng.normal(size=(500, OBS_DIM)) * 2.0, rng.normal(size=(500, A))
    got = pol.log_prob_np(obs, eps)
    out = torch.from_numpy(pol.pre_head_np(obs))
    mean, log_std = torch.chunk(out, 2, dim=-1)
    std = torch.exp(torch.clamp(log_std, -20.0, 2.0))
    x = mean + std * torch.from_numpy(eps)
    per_action = torch.distributions.Normal(mean, std).log_prob(x) - torch.log(1.0 - torch.tanh(x) ** 2 + 1e-6)
    want = per_action.sum(dim=-1).numpy()
    far_action = (x.abs() > 3.0).numpy()
    far = far_action.any(axis=-1)
    assert 0 < far.sum() < len(far) / 2
    cancel = np.sum(np.where(far_action, 4.4e-16 / ((1.0 - np.tanh(x.numpy()) ** 2) + 1e-6), 0.0), axis=-1)
    assert np.all(cancel[~far] == 0.0) and cancel.max() <= A * 4.4e-10
    err = np.abs(got - want)
    print("max relative error, near rows:", float(np.max(err[~far] / np.abs(want[~far]))), " far rows:", float(np.max(err[far] / np.abs(want[far]))))
    assert np.all(err[~far] <= 1e-12 * np.abs(want[~far])), float(np.max(err[~far] / np.abs(want[~far])))
    assert np.all(err[far] <= 1e-12 * np.abs(want[far]) + cancel[far]), float(np.max(err[far] / np.abs(want[far])))
    # the action it belongs to is the one forward_np samples
    np.testing.assert_array_equal(pol.forward_np(obs, eps), np.tanh(x.numpy()))
    # a clamped log_std enters clamped
    bs[-1][A:] = 7.0
    ws[-1][A:] = 0.0
    hot = P.MLPPolicy(ws, bs, activation="tanh")
    e0 = np.zeros((3, A))
    np.testing.assert_allclose(hot.log_prob_np(obs[:3], e0) + np.sum(np.log((1.0 - hot.forward_np(obs[:3], e0) ** 2) + 1e-6), axis=-1),
                               A * (-2.0 - 0.5 * math.log(2.0 * math.pi)), rtol=1e-13)
    with pytest.raises(ValueError):
        P.MLPPolicy(*_layers([OBS_DIM, 8, A]), head="tanh").log_prob_np(obs, eps)


# ---- GAE ---------------------------------------------------------------------------------------------------------------------------
T_, B_ = 7, 4
#            b = 0: time limit at t = 2, then an unfinished tail;  1: truncated at t = 4, tail;  2: never done;  3: both kinds, and done at T - 1
FLAGS = np.array([[0, 0, 0, 0],
                  [0, 0, 0, 2],
                  [1, 0, 0, 0],
                  [0, 0, 0, 0],
                  [0, 2, 0, 1],
                  [0, 0, 0, 0],
                  [0, 0, 0, 3]], dtype=np.uint8)


def _hand_made(seed=0):
    rng = np.random.default_rng(seed)
    rewards, values = rng.normal(size=(T_, B_)), rng.normal(size=(T_ + 1, B_))
    tt, bb = np.nonzero(FLAGS)
    order = rng.permutation(len(tt))                          # "in no particular order"
    index = np.stack([tt[order], bb[order]], axis=1).astype(np.int32)
    return rewards, values, index, rng.normal(size=len(tt))


def _episodes(b):
    """[(t0, t1)]: the runs of steps of instance b that belong to one episode; t1 is its last step in the rollout"""
    out, t0 = [], 0
    for t in range(T_):
        if FLAGS[t, b] or t == T_ - 1:
            out.append((t0, t))
            t0 = t + 1
    return out


@pytest.mark.parametrize("mask", [0, 1, 2, 3])
def test_gae_np_is_the_discounted_sum_of_td_errors_per_episode(mask):
    rewards, values, index, term_values = _hand_made()
    assert {1, 2, 3} <= set(FLAGS.ravel().tolist()) and FLAGS[-1, 0] == 0      # both bits, both at once, and an unfinished tail
    gamma, lam, shift, scale = 0.97, 0.9, 0.3, 1.7
    adv, ret = P.gae_np(rewards, values, FLAGS, term_values, index, gamma, lam, mask, shift, scale)
    term_v = {(int(t), int(b)): float(v) for (t, b), v in zip(index, term_values)}
    want = np.empty((T_, B_))
    for b in range(B_):
        for t0, t1 in _episodes(b):
            delta = {}
            for t in range(t0, t1 + 1):
                if FLAGS[t, b]:
                    nxt = term_v[(t, b)] if FLAGS[t, b] & mask else 0.0
                else:
                    nxt = values[t + 1, b]
                delta[t] = (rewards[t, b] - shift) * scale + gamma * nxt - values[t, b]
            for t in range(t0, t1 + 1):
                want[t, b] = sum((gamma * lam) ** (k - t) * delta[k] for k in range(t, t1 + 1))
    np.testing.assert_allclose(adv, want, rtol=1e-12, atol=1e-14)
    np.testing.assert_array_equal(ret, adv + values[:T_])


@pytest.mark.parametrize("mask", [0, 1, 2, 3])
def test_gae_np_with_lambda_one_is_the_discounted_return_plus_bootstrap(mask):
    rewards, values, index, term_values = _hand_made(seed=1)
    gamma = 0.95
    adv, ret = P.gae_np(rewards, values, FLAGS, term_values, index, gamma, 1.0, mask)
    term_v = {(int(t), int(b)): float(v) for (t, b), v in zip(index, term_values)}
    for b in range(B_):
        for t0, t1 in _episodes(b):
            if FLAGS[t1, b]:
                boot = term_v[(t1, b)] if FLAGS[t1, b] & mask else 0.0
            else:
                boot = values[t1 + 1, b]                        # the unfinished tail: V(obs_seq[T])
                assert t1 == T_ - 1
            for t in range(t0, t1 + 1):
                g = sum(gamma ** (k - t) * rewards[k, b] for k in range(t, t1 + 1)) + gamma ** (t1 + 1 - t) * boot
                assert abs(ret[t, b] - g) <= 1e-12 * (1.0 + abs(g)), (t, b, ret[t, b], g)
    # the masks differ exactly where a masked flag ended an episode
    if mask:
        adv0, _ = P.gae_np(rewards, values, FLAGS, term_values, index, gamma, 1.0, 0)
        changed = np.zeros((T_, B_), dtype=bool)
        for b in range(B_):
            for t0, t1 in _episodes(b):
                if FLAGS[t1, b] & mask:
                    changed[t0:t1 + 1, b] = True
        assert np.array_equal(adv != adv0, changed)


def test_bootstrap_names_and_masks():
    from grid_fed_rl_gym_amd.rollout import _bootstrap_mask
    assert [_bootstrap_mask(x) for x in ((), "terminated", "truncated", ("truncated",), ("terminated", "truncated"), 3, 0)] == [0, 1, 2, 2, 3, 3, 0]
    with pytest.raises(ValueError, match="unknown episode end"):
        _bootstrap_mask("done")
    with pytest.raises(ValueError, match="unknown episode end"):
        _bootstrap_mask(("terminated", "timeout"))
