"""CPU-only: the case table of tests/q_next_cases.py reaches every branch of the policy-action TD targets it is there for (by the
rules of csrc/policy.h, csrc/q_next.h and csrc/mlp_f32.h restated there), each branch by a row asked for BY NAME -- so that dropping
that row fails here --, the feeders have the widths the table counts on, the row counts of the wide feeders meet the yardstick, and
no row is silently degenerate: the NumPy restatements (``exact=True``) on seeded synthetic inputs of every row's widths give actions
that move and stay inside (-1, 1), twins that differ, and for the two policies of the head's extremes everything
tests/test_gpu_q_next_shapes.py asserts of them on the device.  No device is used."""
import os

import numpy as np
import pytest

import grid_fed_rl_gym_amd as P
from grid_fed_rl_gym_amd import _lib
from grid_fed_rl_gym_amd.rollout import policy_rows_np, q_rollout_np
from tests import learner_cases as L
from tests import q_next_cases as C


def test_the_feeders_have_the_widths_the_table_counts_on():
    for name, f in C.FEEDERS.items():
        fs = C.feeder(name)
        assert (fs.obs_dim, fs.action_dim) == (f.D, f.A), name
    for name in ("ieee13", "ieee123"):
        assert (C.FEEDERS[name].D, C.FEEDERS[name].A) == L.WIDTHS[name]


def test_the_rules_are_those_of_the_headers():
    here = os.path.join(os.path.dirname(_lib.__file__), "csrc")
    for name, texts in (("policy.h", ("GS_POL_WAVES = 4", "GS_VAL_ROWS = 64, GS_VAL_PANEL_KB = 21",
                                      "const int panels = (kb0 + GS_VAL_PANEL_KB - 1) / GS_VAL_PANEL_KB; return (kb0 + panels - 1) / panels;")),
                        ("q_next.h", ("inline int gs_qn_term_stride(int A) { return A | 1; }",)),
                        ("kernels_q_next.hip", ("fmin(fmax((double)l32, -20.0), 2.0)", "(uint32_t)(k >> 2), P.draw, P.tag, k & 3", "const int tile = wave + GS_POL_WAVES * c;",
                                                "if (P.D & 1) gq_stage<GS_VAL_ROWS, false>", "if (row0 >= rows) return;")),
                        ("gw_math.h", ("40.0",)),
                        ("mlp_f32.h", ("const int rows = rows_dev ? min(*rows_dev, P.rows) : P.rows;", "if (!FULL && wave >= L.nt) return;"))):
        src = open(os.path.join(here, name)).read()
        for text in texts:
            assert text in src, (name, text)
    assert (C.GS_POL_WAVES, C.GS_VAL_ROWS, C.GS_VAL_PANEL_KB) == (4, 64, 21)
    assert C.head_tiles(3) == dict(nt=1, owners=(0,), last_full=False) and C.head_tiles(8) == dict(nt=1, owners=(0,), last_full=True)
    assert C.head_tiles(11)["owners"] == (0, 1) and C.head_tiles(18) == dict(nt=3, owners=(0, 1, 2), last_full=False)
    assert [C.noise_quads(A) for A in (1, 2, 4, 5, 7, 8, 18)] == [(1, 1), (1, 2), (1, 4), (2, 1), (2, 3), (2, 4), (5, 2)]
    assert [C.term_stride(A) for A in (1, 2, 3, 8, 18)] == [1, 3, 3, 9, 19]
    assert [C.panel_kb(k) for k in (3, 20, 21, 22, 43, 62, 63, 64, 75)] == [3, 20, 21, 11, 15, 21, 21, 16, 19]
    assert C.panels(345) == (11, 11) and C.panels(684) == (15, 15, 13) and C.panels(1193) == (19, 19, 19, 18) and C.panels(320) == (20,)
    assert C.stage(320) == dict(even=True, whole=True, kb0=20, panels=(20,)) and C.stage(71) == dict(even=False, whole=False, kb0=5, panels=(5,))
    assert [C.tiles(n) for n in (0, 1, 64, 65, 128, 130, 185)] == [(0, None), (1, False), (1, True), (2, False), (2, True), (3, False), (3, False)]


def test_the_table_holds_the_rows_the_issue_names():
    assert list(C.HIDDEN) == [((), "relu"), ((17,), "tanh"), ((65,), "relu"), ((96, 40), "relu"), ((40, 96), "elu"), ((256, 17, 256), "relu"),
                              ((17, 240, 1), "tanh"), ((200, 24, 136), "elu")]
    assert list(C.TWINS) == ["A", "B", "C", "D", "E"]
    assert [s.name for s in C.SHAPES] == [L.row_id(r) for r in L.TABLE] + ["twins-" + n for n in C.TWINS] and len(C.SHAPE_CASES) == 13
    for s in C.SHAPES:
        assert s.data == ("ieee123" if s.name == "twins-E" else "ieee13"), s
    assert C.DATA["ieee13"] == ("ieee13", 5, 37, 14, (0.98, 1.02)) and C.DATA["ieee123"] == ("ieee123", 70, 3, 2, (0.98, 1.02))
    # a table row's twins share its hidden widths and differ; a twin case's twins are learner_cases'
    for s in C.SHAPES[:8]:
        assert [t[0] for t in s.twins] == [s.policy, s.policy] and s.twins[0][1] != s.twins[1][1] and s.q_activation == s.policy_activation
    assert C.SHAPE_CASES["twins-D"].twins[0] is None and C.SHAPE_CASES["twins-D"].twins[1][0] == (200,)
    assert [(h.feeder, C.FEEDERS[h.feeder].D, C.FEEDERS[h.feeder].A) for h in C.HEADS] == [("scal6", 40, 1), ("scal9", 82, 2), ("scal21", 345, 5),
                                                                                         ("scal20", 320, 7), ("scal48", 1193, 18)]
    assert all(C.head_rows(h)[0] >= 65 for h in C.HEADS)
    assert sorted(C.EXTREMES) == ["high", "low"] and all(len(m) == len(ls) == C.FEEDERS["ieee13"].A for m, ls in C.EXTREMES.values())
    assert C.BASE == ("ieee13", 65, 4, 2, (0.5, 1.5)) and C.replay_rows(C.Replay("base", C.BASE.T, C.BASE.B, True)) == (260, 130)
    assert [(r.name, r.stochastic) + C.replay_rows(r) for r in C.REPLAYS] == [("T3-B65", True, 195, 65), ("T4-B32", False, 128, 64), ("T2-B32", False, 64, 32),
                                                                               ("T1-B65", True, 65, 0), ("T1-B1", False, 1, 0)]
    assert all(r.stochastic == (r.B == C.BASE.B) for r in C.REPLAYS)      # the base's noise index only under the base's B
    assert C.REUSE == (("T4", "T1", "T4"), ("T1", "T4"))


def _shape_facts(name):
    s = C.SHAPE_CASES[name]
    d, f = C.DATA[s.data], C.FEEDERS[s.data]
    return C.facts(f.D, f.A, s.policy, d.B * d.T, 0)


def _head_facts(name):
    h, f = C.HEAD_CASES[name], C.FEEDERS[name]
    return C.facts(f.D, f.A, C.SQUARE, *C.head_rows(h))


def _replay_facts(name):
    f = C.FEEDERS[C.BASE.feeder]
    return C.facts(f.D, f.A, C.SQUARE, *C.replay_rows(C.REPLAY_CASES[name]))


def test_every_branch_is_reached_by_a_named_row():
    # ---- layer shapes: every layer of the policy kernel, the padded last one too, is gq_layer<4, FULL>
    owned = lambda name, l: _shape_facts(name)["layers"][l][3]
    assert owned("ieee13-17-tanh", 0) == (1, 1, 0, 0)                                       # a narrow layer: wavefronts 2 and 3 idle
    assert owned("ieee13-65-relu", 0) == (2, 1, 1, 1)                                       # nt = 5: wavefront 0 owns two tiles
    assert _shape_facts("ieee13-256x17x256-relu")["n_layers"] == 4
    assert [l[2] for l in _shape_facts("ieee13-256x17x256-relu")["layers"]] == [True, False, True, False]      # FULL, narrow, FULL, the head
    assert _shape_facts("ieee13-17x240x1-tanh")["layers"][2][:2] == (15, 1) and _shape_facts("ieee13-17x240x1-tanh")["layers"][3][0] == 1     # a one-unit layer
    a, b = _shape_facts("ieee13-96x40-relu")["layers"][1], _shape_facts("ieee13-40x96-elu")["layers"][1]
    assert a[:2] == (6, 3) and b[:2] == (3, 6)                                              # the rectangular pair, kb > nt and kb < nt
    assert _shape_facts("ieee13-single-relu")["n_layers"] == 1
    assert _shape_facts("ieee13-200x24x136-elu")["layers"][0][1] == 13
    # the head layer is never FULL and always leaves wavefronts idle below A = 25
    assert all(not _shape_facts(s.name)["layers"][-1][2] and _shape_facts(s.name)["layers"][-1][3][3] == 0 for s in C.SHAPES)
    # twins of different depth and row_stride in both orders, a linear policy and a linear twin, one twin alone, mixed activations
    stride = lambda t: None if t is None else L.facts([71 + 3, *t[0], 1])["row_stride"]
    sa, sb = ([stride(t) for t in C.SHAPE_CASES[n].twins] for n in ("twins-A", "twins-B"))
    assert sa[0] < sa[1] and sb == sa[::-1] and len(C.SHAPE_CASES["twins-A"].twins[0][0]) != len(C.SHAPE_CASES["twins-A"].twins[1][0])
    c, d, e = (C.SHAPE_CASES[n] for n in ("twins-C", "twins-D", "twins-E"))
    assert c.policy == () and c.twins[0][0] == () and c.twins[1][0] == (256, 17, 256)
    assert d.twins[0] is None and d.policy_activation != d.q_activation
    assert e.data == "ieee123" and C.q_panels(684, 8) == (15, 15, 14) and e.twins[0][0] == ()
    # ---- head width
    f = {n: _head_facts(n) for n in C.HEAD_CASES}
    assert f["scal6"]["term_stride"] == 1 and f["scal6"]["quads"] == (1, 1) and f["scal6"]["stage"]["kb0"] == 3            # A = 1
    assert f["scal9"]["quads"] == (1, 2) and f["scal9"]["term_stride"] == 3                                                   # A = 2
    assert f["scal21"]["quads"] == (2, 1) and f["scal20"]["quads"] == (2, 3)                                                  # a second quad, partly used
    assert f["scal48"]["head"] == dict(nt=3, owners=(0, 1, 2), last_full=False) and f["scal48"]["quads"] == (5, 2)            # wavefront 2 owns a head tile
    assert f["scal48"]["term_stride"] == 19
    # ---- observation staging
    assert f["scal6"]["stage"]["even"] and not f["scal6"]["stage"]["whole"]                 # EVEN with padded columns
    assert f["scal20"]["stage"] == dict(even=True, whole=True, kb0=20, panels=(20,))         # EVEN, no padded column at all
    assert not f["scal21"]["stage"]["even"] and f["scal21"]["stage"]["panels"] == (11, 11)   # two equal panels
    assert f["scal48"]["stage"]["panels"] == (19, 19, 19, 18)                                # four panels
    assert C.q_panels(1193, 18) == (19, 19, 19, 19) and C.q_panels(345, 5) == (11, 11) and C.q_panels(320, 7) == (21,)
    # ---- the sampling head's extremes: log_std beyond both clamp ends and a mean beyond gw_tanh's cap, in both orders
    for name, sign in (("high", 1.0), ("low", -1.0)):
        mean, ls = C.EXTREMES[name]
        assert sign * mean[0] > C.TANH_CAP + 2 and max(ls) > C.LOG_STD_MAX + 2 and min(ls) < C.LOG_STD_MIN - 2
    assert np.argmax(C.EXTREMES["high"][1]) != np.argmax(C.EXTREMES["low"][1])
    # ---- row and terminal-list tiles
    r = {n: _replay_facts(n) for n in C.REPLAY_CASES}
    base = C.facts(71, 3, C.SQUARE, 260, 130)
    assert base["row_tiles"] == (5, False) and base["terminal_tiles"] == (3, False)          # a list crossing 128
    assert r["T3-B65"]["terminal_tiles"] == (2, False) and C.replay_rows(C.REPLAY_CASES["T3-B65"])[1] == 65     # one full tile and one entry
    assert r["T4-B32"]["row_tiles"] == (2, True) and r["T4-B32"]["terminal_tiles"] == (1, True)                 # exactly 64 entries, 128 rows
    assert C.replay_rows(C.REPLAY_CASES["T4-B32"]) == (128, 64)
    assert r["T2-B32"]["row_tiles"] == (1, True) and r["T2-B32"]["terminal_tiles"] == (1, False)                # 64 rows, a short list
    assert r["T1-B65"]["row_tiles"] == (2, False) and r["T1-B65"]["terminal_tiles"] == (0, None)                # 65 rows, rows_dev = 0
    assert r["T1-B1"]["row_tiles"] == (1, False) and C.replay_rows(C.REPLAY_CASES["T1-B1"]) == (1, 0)           # one row, rows_dev = 0
    # ---- buffer reuse: a shorter rollout after a longer one on one handle, a longer one after a shorter one on another
    T = {"T4": 4, "T1": 1}
    assert any(T[a] > T[b] for seq in C.REUSE for a, b in zip(seq, seq[1:])) and any(T[a] < T[b] for seq in C.REUSE for a, b in zip(seq, seq[1:]))
    assert C.REUSE[1][0] == "T1" and C.REUSE[0][:2] == ("T4", "T1")
    assert C.BASE.T == T["T4"] and C.REPLAY_CASES["T1-B65"].T == T["T1"] and C.REPLAY_CASES["T1-B65"].B == C.BASE.B


@pytest.mark.parametrize("name", [h.feeder for h in C.HEADS if C.FEEDERS[h.feeder].D >= C.WIDE_D])
def test_the_wide_feeders_row_counts_meet_the_yardstick(name):
    """Section 25's yardstick, restated in q_next_cases.chain_yardstick: over the rollout rows and over the terminal rows of a wide
    feeder one plain float32 chain lies within 3.0 E_ref in every one of 20 draws -- what section 25 accepted at 81 rows under the
    bound of 4."""
    h = C.HEAD_CASES[name]
    assert h.limits == (0.5, 1.5) and h.T % h.episode_length == 0      # (only the time limit ends an episode: the terminal rows are counted here)
    for rows in C.head_rows(h):
        median, largest = C.chain_yardstick(C.FEEDERS[name].D, rows)
        print(f"{name} D = {C.FEEDERS[name].D}, {rows} rows: chain error / E_ref median {median:.2f}, largest {largest:.2f}")
        assert largest <= C.YARDSTICK_BOUND, (name, rows, largest)


def _synthetic(D, n, seed):
    return np.random.default_rng(seed).normal(0.0, 1.0, (n, D))


def _policy(D, A, hidden, activation, bias=None):
    return P.MLPPolicy(*C.policy_layers(D, A, hidden, bias), activation=activation, head="gaussian_tanh", compute="float32")


def _moves(tag, pol, qs, D, A, n=185):
    """the restatements on seeded rows: the pre-head values see float32 (E_ref > 0), the actions move and stay inside (-1, 1), the
    twins' values move and (two twins) each is the smaller one somewhere"""
    obs = _synthetic(D, n, 7)
    eps = np.random.default_rng(8).normal(0.0, 1.0, (n, A))
    exact, act, lp = policy_rows_np(pol, obs, eps, exact=True)
    assert float(np.max(np.abs(policy_rows_np(pol, obs, eps)[0] - exact))) > 0.0, tag
    assert np.std(act) > 1e-2 and (np.abs(act) < 1.0).all() and np.isfinite(lp).all() and np.std(lp) > 1e-2, tag
    assert (np.abs(exact[:, A:]) < 2.0).all(), tag            # log_std inside the clamp by far
    q = [q_rollout_np(net, obs[None], act[None], exact=True)[0] for net in qs]
    assert all(np.std(x) > 1e-3 for x in q), tag
    if len(q) == 2:
        assert 0 < (q[0] < q[1]).sum() < n, tag


@pytest.mark.parametrize("name", [s.name for s in C.SHAPES])
def test_no_network_shape_is_degenerate(name):
    s = C.SHAPE_CASES[name]
    f = C.FEEDERS[s.data]
    qs = [P.MLPQ(*C.q_layers(f.D, f.A, t[0], t[1]), f.D, activation=s.q_activation) for t in s.twins if t is not None]
    _moves(name, _policy(f.D, f.A, s.policy, s.policy_activation), qs, f.D, f.A)


@pytest.mark.parametrize("name", [h.feeder for h in C.HEADS])
def test_no_head_width_is_degenerate(name):
    f = C.FEEDERS[name]
    qs = [P.MLPQ(*C.q_layers(f.D, f.A, C.SQUARE, 20 + w), f.D, activation="relu") for w in range(2)]
    _moves(name, _policy(f.D, f.A, C.SQUARE, "relu"), qs, f.D, f.A, n=81)


@pytest.mark.parametrize("name", sorted(C.EXTREMES))
@pytest.mark.parametrize("stochastic", [True, False])
def test_the_extreme_policies_reach_the_clamp_the_cap_and_the_saturated_actions(name, stochastic):
    """what tests/test_gpu_q_next_shapes.py asserts of the device's pre-head values, on seeded rows"""
    f = C.FEEDERS["ieee13"]
    n = 185
    pol = _policy(f.D, f.A, C.SQUARE, "relu", C.EXTREMES[name])
    eps = np.random.default_rng(8).normal(0.0, 1.0, (n, f.A)) if stochastic else None
    pre, act, lp = policy_rows_np(pol, _synthetic(f.D, n, 7), eps)
    seen = C.extremes_reached(pre, np.zeros((n, f.A)) if eps is None else eps, act, lp)
    assert seen["above"] == n and seen["below"] == n and seen["capped"] > n // 2, seen
