"""CPU-only: the case table of tests/gs3_cases.py lands every row on the kernel form it names (by the selection rules restated in
plan_form), the table names all eight instantiations of the three-phase solver, and every row can see the mistakes it is there
for -- the NumPy oracle needs at least five sweeps, its iteration count does not sit on the tolerance, and transposing the line
impedances or swapping two of their phases moves the answer by 1000 times the bar the GPU is held to.  Neither the library nor a
device is loaded."""
import numpy as np
import pytest

from oracle import oracle3_np as O3
from tests import gs3_cases as G

TOL = 1e-9


def _ids(c):
    return c.name


@pytest.mark.parametrize("case", G.CASES, ids=_ids)
def test_every_row_lands_on_the_form_it_names(case):
    d = case.get()
    spec = d["spec"]
    p = G.plan_form(spec)
    K, MK, threads = case.form
    assert (p["positions_per_thread"], p["mutual_per_thread"], p["threads"]) == (K, MK, threads)
    assert p["kernel"] == ("fbs3_resident" if K else "fbs3")
    if case.ns is not None:
        assert p["conductors"] == case.ns
    if case.M is not None and K:
        assert p["mutual_entries"] == case.M
    if case.width is not None:
        assert p["max_level_width"] == case.width
    assert (p["level_lds_messages"] != 0) == case.lds and p["level_lds_messages"] in (0, 32 * p["max_level_width"])
    if K:       # padding positions: none where the row is there for that
        assert (K * threads == p["conductors"]) == (case.name in ("r3_full", "r9_no_padding", "r19_no_padding"))
        dense = G.plan_form(spec, dense=True)
        assert dense["mutual_per_thread"] == 0 and dense["threads"] == threads
    lv = G.plan_form(spec, no_resident=True)
    assert (lv["kernel"], lv["threads"], lv["positions_per_thread"], lv["mutual_entries"]) == ("fbs3", 256, 0, 0)
    assert d["P"].shape == (case.B, spec.n, 3) and d["Q"].shape == d["P"].shape


def test_the_selection_boundaries_are_in_the_table():
    plan = {c.name: G.plan_form(c.get()["spec"]) for c in G.CASES}
    at = lambda name: (plan[name]["conductors"], plan[name]["positions_per_thread"], plan[name]["threads"],       # noqa: E731
                       plan[name]["mutual_entries"], plan[name]["mutual_per_thread"])
    assert at("r3_padded") == (193, 3, 128, 60, 3)
    assert at("r3_full") == (1536, 3, 512, 500, 3) and at("r9_list_full") == (1537, 9, 192, 768, 4)      # ns 1536 | 1537; M = 4 x threads
    assert at("r9_list_sparse") == (1537, 9, 192, 40, 4) and at("r9_dense") == (1600, 9, 192, 769, 0)   # M = 4 x threads + 1
    assert at("r9_no_padding") == (4608, 9, 512, 1500, 4) and at("r19_list_full") == (4609, 19, 256, 1024, 4)   # ns 4608 | 4609
    assert at("r19_dense") == (4609, 19, 256, 1025, 0)
    assert at("r19_no_padding") == (9728, 19, 512, 2000, 4) and at("levels_by_default")[:3] == (9729, 0, 256)     # ns 9728 | 9729
    assert [plan[n]["max_level_width"] for n in ("w256", "w257", "w1216", "w1217")] == [256, 257, 1216, 1217]
    assert [plan[n]["level_lds_messages"] for n in ("w256", "w257", "w1216", "w1217")] == [8192, 8224, 38912, 0]
    for name in ("w1216", "w1217"):     # the level below the widest one is itself wider than the workgroup: parents and children straddle passes
        spec = G.BY_NAME[name].get()["plain"]
        depth = np.zeros(spec.n, dtype=int)
        for b in range(1, spec.n):
            depth[b] = depth[spec.parent[b]] + 1
        assert G.present(spec.phases)[depth == 2].sum() >= 300
    assert sum(c.B == 1 for c in G.CASES) == 1 and G.BY_NAME["r3_padded"].B == 70


def test_the_table_names_all_eight_instantiations():
    named = set().union(*(G.instantiations(c) for c in G.CASES))
    assert named == {"gs3_k_resident<3,3>", "gs3_k_resident<3,0>", "gs3_k_resident<9,4>", "gs3_k_resident<9,0>",
                     "gs3_k_resident<19,4>", "gs3_k_resident<19,0>", "gs3_k_solve<true,1>", "gs3_k_solve<false,1>"}
    # by default selection alone (no GS3_DENSE_MUTUAL): everything except <3, 0>, which no feeder reaches -- 3 x threads >= conductors > M
    by_default = {"gs3_k_resident<%d,%d>" % c.form[:2] for c in G.CASES if c.form[0]}
    assert by_default == {"gs3_k_resident<3,3>", "gs3_k_resident<9,4>", "gs3_k_resident<9,0>", "gs3_k_resident<19,4>", "gs3_k_resident<19,0>"}
    assert any(not c.form[0] for c in G.CASES) and any(c.levels and not c.lds for c in G.CASES) and any(c.levels and c.lds for c in G.CASES)


@pytest.mark.parametrize("case", G.CASES, ids=_ids)
def test_every_row_is_relabelled_asymmetric_and_has_every_kind_of_node(case):
    d = case.get()
    spec, plain, perm = d["spec"], d["plain"], d["perm"]
    n = spec.n
    assert spec.source != 0 and spec.parent[spec.source] == -1 and len(set(spec.v_source)) == 3 and 1.0 != spec.v_source[0]
    others = np.arange(n) != spec.source
    assert (spec.parent[others] > np.arange(n)[others]).sum() >= 10          # children numbered below their parents
    for i in (0, 1, n // 2, n - 1):      # the relabelling carries everything along
        j = perm[i]
        assert spec.phases[j] == plain.phases[i] and np.array_equal(spec.z[j], plain.z[i]) and np.array_equal(d["P"][:, j], d["P_plain"][:, i])
        assert spec.parent[j] == (-1 if i == 0 else perm[plain.parent[i]])
    pres = G.present(spec.phases)
    assert np.all(d["P"][:, ~pres] == 0) and np.all(d["P"][:, spec.source] == 0) and np.all(d["P"][:, pres & others[:, None]] < 0)
    for m in (3, 5, 6):                  # two-phase nodes of each kind, a single-phase child under some
        two = np.nonzero(spec.phases == m)[0]
        assert len(two) and any(spec.phases[c] in (1, 2, 4) and spec.parent[c] in two for c in range(n))
    z = spec.z[others]
    flat = z.reshape(len(z), 9)
    assert all(len(set(row)) == 9 for row in flat[:: max(1, len(flat) // 50)])   # nine distinct entries
    assert np.min(np.abs(z - z.transpose(0, 2, 1))[:, [0, 0, 1], [1, 2, 2]]) > 1e-6        # Z[i][j] != Z[j][i] on every line
    for b in np.nonzero(others)[0][:: max(1, n // 100)]:                         # every present-phase block well conditioned
        idx = np.nonzero(pres[b])[0]
        assert np.linalg.cond(spec.z[b][np.ix_(idx, idx)]) < 10.0


def _oracle(spec, P, Q, tol=TOL, z=None):
    return O3.fbs3_solve(spec.parent, spec.phases, spec.z if z is None else z, spec.source, spec.v_source, P, Q, tolerance=tol,
                         max_iterations=100)


@pytest.mark.parametrize("case", G.CASES, ids=_ids)
def test_every_row_can_see_what_it_is_there_for(case):
    """The oracle-side conditions, on the feeder and the batch the GPU runs.  Every instance: the oracle converges and its
    iteration count is the same at tolerances 1e-9 (1 -+ 1e-3), so the equality the GPU test asserts is no coin toss.  The first
    instance: at least five sweeps, the lowest voltage inside (0.90, 0.995), and the index mix-ups the GPU side could make
    (row <-> column, phase b <-> c of every Z) move some voltage by 1000 x the 1e-10 bar."""
    d = case.get()
    spec = d["spec"]
    first = None
    for b in range(case.B):
        lo, hi = _oracle(spec, d["P"][b], d["Q"][b], TOL * (1 - 1e-3)), _oracle(spec, d["P"][b], d["Q"][b], TOL * (1 + 1e-3))
        assert lo["converged"] and hi["converged"]
        # the count is monotone in the tolerance: equal at both ends means equal at 1e-9, with the final mismatch clear of it
        assert lo["iterations"] == hi["iterations"], b
        first = first or lo
    assert first["iterations"] >= 5
    mag = np.abs(first["voltages"][G.present(spec.phases)])
    assert 0.90 < mag.min() < 0.995
    swap = [0, 2, 1]
    for zz in (spec.z.transpose(0, 2, 1), spec.z[:, swap][:, :, swap]):
        other = _oracle(spec, d["P"][0], d["Q"][0], z=np.ascontiguousarray(zz))
        assert np.max(np.abs(other["voltages"] - first["voltages"])) >= 1e-7
