"""CPU-only: the shape table of tests/learner_cases.py reaches every branch of the training kernels it is there for (by the rules of
csrc/policy.h, csrc/train.h and csrc/pathwise.h restated in learner_cases.facts), holds the rows the issue names, and no row is
silently degenerate: the NumPy restatements (``exact=True``) on seeded synthetic inputs of every row's widths give a non-zero largest
entry in every gradient tensor.  No device is used."""
import os

import numpy as np
import pytest

import grid_fed_rl_gym_amd as P
from grid_fed_rl_gym_amd import _lib
from grid_fed_rl_gym_amd.learner import ppo_grad_np, pathwise_grad_np, value_grad_np
from tests import learner_cases as C

FEEDERS = {"ieee13": lambda: P.ieee13_like("epsilon"), "ieee123": P.ieee123_like}


def test_the_feeders_have_the_widths_the_table_counts_on():
    for name, make in FEEDERS.items():
        fs = make()
        assert (fs.obs_dim, fs.action_dim) == C.WIDTHS[name], name


def test_facts_restates_the_rules_of_the_headers():
    f = C.facts([71, 96, 40, 6], 513)
    assert f["layers"] == ((5, 6, False, (2, 2, 1, 1)), (6, 3, False, (1, 1, 1, 0)), (3, 1, False, (1, 0, 0, 0)))
    assert f["T"] == {1: (3, 6), 2: (1, 3)}
    assert [g["in_blocks"] for g in f["grad"]] == [2, 2, 1] and [g["out_blocks"] for g in f["grad"]] == [3, 2, 1]
    assert [g["half_empty_out"] for g in f["grad"]] == [False, True, True]
    assert [g["partial_in_past_64"] for g in f["grad"]] == [True, True, False]
    assert [g["n_in_below_padded"] for g in f["grad"]] == [False, False, True]
    assert (f["row_stride"], f["P"], f["segments"], f["row_tiles"]) == (160, 96 * 72 + 40 * 97 + 6 * 41, 3, 17)
    assert f["reduce_blocks"] == -(-f["P"] // 1024)
    g = C.facts([71, 256, 17, 256, 1])
    assert [l[1:] for l in g["layers"]] == [(16, True, (4, 4, 4, 4)), (2, False, (1, 1, 0, 0)), (16, True, (4, 4, 4, 4)), (1, False, (1, 0, 0, 0))]
    q = C.q_facts("ieee123", ())
    assert (q["H0"], q["panels"], q["linear"], q["layers"][0][0]) == (1, 3, True, 44)
    here = os.path.join(os.path.dirname(_lib.__file__), "csrc")
    for name, texts in (("policy.h", ("GS_POL_WAVES = 4", "GS_POL_MAX_WIDTH = 256", "GS_VAL_PANEL_KB = 21")),
                        ("train.h", ("GS_TR_ROWS = 32", "GS_TR_SEG = 256", "GS_TR_WT_OUT = 2, GS_TR_WT = 4", "GS_TR_RED_THREADS = 256, GS_TR_RED_PER_THREAD = 4")),
                        ("pathwise.h", ("GS_PW_JT = 64",))):
        src = open(os.path.join(here, name)).read()
        for text in texts:
            assert text in src, (name, text)
    assert C.GS_POLICY_MAX_LAYERS == _lib.GS_POLICY_MAX_LAYERS


def test_the_table_holds_the_rows_the_issue_names():
    assert [(r.hidden, r.activation) for r in C.TABLE] == [((), "relu"), ((17,), "tanh"), ((65,), "relu"), ((96, 40), "relu"), ((40, 96), "elu"),
                                                            ((256, 17, 256), "relu"), ((17, 240, 1), "tanh"), ((200, 24, 136), "elu")]
    for r in C.TABLE:
        assert r.feeder == "ieee13" and set(r.sizes) >= {33, 185}, r
        assert (513 in r.sizes) == (r.hidden == (96, 40))
    assert C.SEGMENT_ROLLOUT[0] * C.SEGMENT_ROLLOUT[1] >= 513 and C.ROLLOUT["ieee13"][0] * C.ROLLOUT["ieee13"][1] >= 185
    assert [t.name for t in C.TWINS] == ["A", "B", "C", "D", "E"]
    A, B, Cc, D, E = C.TWINS
    assert (A.policy, A.q1, A.q2) == ((96, 40), (65,), (40, 96, 17)) and (B.policy, B.q1, B.q2) == (A.policy, A.q2, A.q1)
    assert (Cc.policy, Cc.q1, Cc.q2, Cc.policy_activation, Cc.q_activation) == ((), (), (256, 17, 256), "elu", "elu")
    assert (D.policy, D.q1, D.q2, D.policy_activation, D.q_activation) == ((17, 240, 1), None, (200,), "tanh", "relu")
    assert (E.feeder, E.policy, E.q1, E.q2) == ("ieee123", (17,), (), (17,))
    # each activation meets a rectangular hidden-to-hidden layer
    rect = {r.activation for r in C.TABLE if len(r.hidden) >= 2 and any(-(-a // 16) != -(-b // 16) for a, b in zip(r.hidden, r.hidden[1:]))}
    assert rect == {"relu", "tanh", "elu"}


def test_the_table_reaches_every_branch():
    rows = [C.facts(C.policy_dims(r.feeder, r.hidden), n) for r in C.TABLE for n in r.sizes]
    rows += [C.facts(C.value_dims(r.feeder, r.hidden), n) for r in C.TABLE for n in r.sizes]
    assert {f["n_layers"] for f in rows} == {1, 2, 3, 4}                                     # every depth 1 .. 4
    hidden_T = [f["T"][l] for f in rows for l in f["T"] if l < f["n_layers"] - 1]            # T of hidden-to-hidden layers
    assert any(kb < nt for kb, nt in hidden_T) and any(kb > nt for kb, nt in hidden_T)       # kb != nt in both directions
    tiles = {l[1] for f in rows for l in f["layers"]}
    for group in ({1, 2}, {3, 4}, set(range(5, 16)), {16}):
        assert tiles & group, group
    assert tiles >= {1, 2, 5, 13, 15, 16}
    owned = {l[3] for f in rows for l in f["layers"]}
    assert any(len(set(o)) > 1 and min(o) >= 1 for o in owned)                               # wavefronts own unequal, non-zero tile counts
    assert any(min(o) == 0 for o in owned)                                                   # wavefronts that return early
    assert {l[2] for f in rows for l in f["layers"]} == {True, False}
    # a half-empty output block and a partial input block past the first, on a hidden-to-hidden layer (not the head)
    assert any(g["half_empty_out"] and g["partial_in_past_64"] for f in rows for g in f["grad"][1:-1])
    assert any(g["n_in_below_padded"] for f in rows for g in f["grad"])
    assert any(1 in C.policy_dims(r.feeder, r.hidden)[1:-1] for r in C.TABLE)                # a one-unit layer
    assert all(f["P"] % 1024 for f in rows)                                                  # P no multiple of the reduce width
    assert {f["reduce_blocks"] > 1 for f in rows} == {True, False}
    assert any(f["segments"] > 1 for f in rows) and any(f["row_tiles"] > 1 and f["segments"] == 1 for f in rows)
    # the twins
    strides = {t.name: [None if q is None else C.q_facts(t.feeder, q)["row_stride"] for q in (t.q1, t.q2)] for t in C.TWINS}
    both = [s for s in strides.values() if None not in s]
    assert any(a < b for a, b in both) and any(a > b for a, b in both)                       # different row_stride in both orders
    assert any(None in s for s in strides.values())                                          # one twin alone
    H0 = {C.q_facts(t.feeder, q)["H0"] for t in C.TWINS for q in (t.q1, t.q2) if q is not None}
    assert 1 in H0 and 65 in H0 and any(h % 4 and h != 65 and h != 1 for h in H0) and any(h >= 3 * C.GS_PW_JT for h in H0)
    assert any(C.q_facts(t.feeder, q)["linear"] and C.q_facts(t.feeder, q)["panels"] > 1 for t in C.TWINS for q in (t.q1, t.q2) if q is not None)
    assert any(t.policy_activation != t.q_activation for t in C.TWINS)
    qT = [C.q_facts(t.feeder, q)["T"] for t in C.TWINS for q in (t.q1, t.q2) if q is not None]
    assert any(kb != nt for T in qT for l, (kb, nt) in T.items())
    assert any(len(t.policy) != len(q) for t in C.TWINS for q in (t.q1, t.q2) if q is not None)


def _nonzero(tag, grads):
    for l, (dW, db) in enumerate(grads):
        assert float(np.max(np.abs(dW))) > 0.0, (tag, f"dW[{l}]")
        assert float(np.max(np.abs(db))) > 0.0, (tag, f"db[{l}]")


ROW_SIZES = [(r, n) for r in C.TABLE for n in (33, 185)]


@pytest.mark.parametrize("row,n", ROW_SIZES, ids=[f"{C.row_id(r)}-n{n}" for r, n in ROW_SIZES])
def test_no_policy_or_critic_row_is_degenerate(row, n):
    D, A = C.WIDTHS[row.feeder]
    x = C.synthetic(D, n, A, seed=n)
    layers = list(zip(*C.draw(C.policy_dims(row.feeder, row.hidden), C.SEEDS["policy"])))
    first = ppo_grad_np(layers, x["obs"], x["actions"], np.zeros(n), x["adv"], 0.2, 0.01, exact=True, activation=row.activation)
    out = ppo_grad_np(layers, x["obs"], x["actions"], first["log_probs_new"] + x["lp_shift"], x["adv"], 0.2, 0.01, exact=True, activation=row.activation)
    assert 0 < out["clipped"].sum() < n / 2
    _nonzero(("policy", row.hidden, n), out["grads"])
    assert len(out["backprop"]["deltas"]) == len(layers) and len(out["backprop"]["acts"]) == len(layers) + 1
    for l, (dW, db) in enumerate(out["grads"]):                                              # the extra key is what the gradients are made of
        d, a = out["backprop"]["deltas"][l], out["backprop"]["acts"][l]
        assert np.allclose(d.T @ a, dW, rtol=1e-12, atol=1e-300) and np.allclose(d.sum(axis=0), db, rtol=1e-12, atol=1e-300)
    for name in ("value", "thermal"):
        layers = list(zip(*C.draw(C.value_dims(row.feeder, row.hidden), C.SEEDS[name])))
        out = value_grad_np(layers, x["obs"], x["ret"], exact=True, activation=row.activation)
        _nonzero((name, row.hidden, n), out["grads"])
        assert "backprop" in out and "backprop" not in value_grad_np(layers, x["obs"], x["ret"], activation=row.activation)


@pytest.mark.parametrize("case", C.TWINS, ids=[t.name for t in C.TWINS])
def test_no_twin_row_is_degenerate(case):
    D, A = C.WIDTHS[case.feeder]
    n = 185
    x = C.synthetic(D, n, A, seed=7)
    layers = list(zip(*C.draw(C.policy_dims(case.feeder, case.policy), C.SEEDS["policy"])))
    qs = [list(zip(*C.draw(C.q_dims(case.feeder, q), C.q_seed(q)))) for q in (case.q1, case.q2) if q is not None]
    out = pathwise_grad_np(layers, qs, x["obs"], x["eps"], 0.2, 0.5, stored_actions=x["actions"], exact=True, activation=case.policy_activation,
                           q_activation=case.q_activation)
    _nonzero((case.name, "policy"), out["grads"])
    assert np.abs(out["dq_da"]).min(axis=(1, 2)).shape == (len(qs),) and all(np.abs(d).max() > 0.0 for d in out["dq_da"])
    assert np.std(out["q"]) > 1e-3
    if len(qs) == 2:                                                                         # both twins are the smaller one somewhere
        assert 0 < out["which"].sum() < n
    sa = np.concatenate([x["obs"], x["actions"].astype(np.float32)], axis=1)
    for w, q in enumerate(qs):                                                               # the twins' own regression steps
        _nonzero((case.name, "twin", w), value_grad_np(q, sa, x["ret"], exact=True, activation=case.q_activation)["grads"])
