"""GPU: every kernel form of the three-phase solver (tests/gs3_cases.py: one feeder per instantiation and selection boundary,
asymmetric impedances, permuted labels, unequal source voltages) against the NumPy oracle at the project's bars, the forms against
each other, repeated solves on one handle, and gs3_create's refusals.  The figures of (A) and (B) are printed before they are
asserted (pytest -s shows them)."""
import numpy as np
import pytest

from grid_fed_rl_gym_amd.components import PowerFlowError
from oracle import oracle3_np as O3
from tests import gs3_cases as G
from tests.test_unbalanced import _solver

pytestmark = pytest.mark.gpu

TOL, MAX_IT = 1e-9, 200
_SOLVED, _REF = {}, {}        # per process: (row, kernel) -> (solution, describe()); (row, instance) -> oracle solution


def _solve(case, kernel, monkeypatch):
    """The row's batch on `kernel`: "default" (the selection as it stands), "resident-dense" (GS3_DENSE_MUTUAL=1) or "levels"
    (GS3_NO_RESIDENT=1).  Solved once per process."""
    key = (case.name, kernel)
    if key not in _SOLVED:
        d = case.get()
        s = _solver(monkeypatch, "resident" if kernel == "default" else kernel, tolerance=TOL, max_iterations=MAX_IT)
        sol = s.solve_batch(d["spec"], d["P"], d["Q"])
        _SOLVED[key] = (sol, s.describe())
        s.close()
    return _SOLVED[key]


def _reference(case, b):
    key = (case.name, b)
    if key not in _REF:
        d = case.get()
        spec = d["spec"]
        _REF[key] = O3.fbs3_solve(spec.parent, spec.phases, spec.z, spec.source, spec.v_source, d["P"][b], d["Q"][b], tolerance=TOL,
                                  max_iterations=MAX_IT)
    return _REF[key]


def _c_oracle(case, first):
    """Instances first.. of a large row on the C oracle.  oracle_c.solve3_batch takes a general Z and source VOLTAGE but wants the
    source at node 0 and parent[i] < i, so it gets the feeder as it was before the relabelling and its answer is carried through
    the permutation.  None where the C oracle is not built: the residual then stands for those instances."""
    from oracle import oracle_c as OC
    d = case.get()
    if not OC.available() or first >= case.B:
        return None
    out = OC.solve3_batch(d["plain"], d["P_plain"][first:], d["Q_plain"][first:], tolerance=TOL, max_iterations=MAX_IT, threads=2)
    V = np.zeros_like(out["voltages"])
    V[:, d["perm"]] = out["voltages"]
    return dict(voltages=V, iterations=out["iterations"], losses=out["losses"], converged=out["converged"])


@pytest.mark.parametrize("case,kernel", [(c, k) for c in G.CASES for k in c.kernels], ids=lambda v: v if isinstance(v, str) else v.name)
def test_gpu_every_form_against_the_oracle(case, kernel, monkeypatch):
    """(A) describe() is what plan_form says; every instance converged; rows of up to 3000 nodes: every instance against the NumPy
    oracle (voltages and losses 1e-10, mismatch 1e-12, equal iteration counts, absent phases exactly 0); larger rows: instance 0
    against the NumPy oracle, the others against the C oracle; all instances: residual and loss balance below 1e-8."""
    d = case.get()
    spec, P, Q = d["spec"], d["P"], d["Q"]
    sol, desc = _solve(case, kernel, monkeypatch)
    plan = G.plan_form(spec, no_resident=(kernel == "levels"))
    print(f"\nGS3FORMS A {case.name}/{kernel}: " + ", ".join(f"{k}={desc[k]}" for k in G.DESCRIBE_FIELDS))
    assert {k: desc[k] for k in G.DESCRIBE_FIELDS} == {k: plan[k] for k in G.DESCRIBE_FIELDS}
    if kernel == "default":
        K, MK, threads = case.form
        assert (desc["positions_per_thread"], desc["mutual_per_thread"], desc["threads"]) == (K, MK, threads)
    else:
        assert desc["kernel"] == "fbs3" and (desc["lds_messages"] != 0) == case.lds
    assert sol.converged.all()
    pres = G.present(spec.phases)
    assert np.all(sol.voltages[:, ~pres] == 0)
    with_oracle = range(case.B) if spec.n <= 3000 else [0]
    fig = dict(dv=0.0, dl=0.0, dmm=0.0, dit=0, res=0.0, bal=0.0, cdv=0.0)
    refs = [_reference(case, b) for b in with_oracle]
    for b, ref in zip(with_oracle, refs):
        fig["dv"] = max(fig["dv"], float(np.max(np.abs(sol.voltages[b] - ref["voltages"]))))
        fig["dl"] = max(fig["dl"], abs(float(sol.losses[b]) - ref["losses"]))
        fig["dmm"] = max(fig["dmm"], abs(float(sol.max_mismatch[b]) - ref["max_mismatch"]))
        fig["dit"] = max(fig["dit"], abs(int(sol.iterations[b]) - ref["iterations"]))
    for b in range(case.B):
        res, ploss = O3.residual(spec.parent, spec.phases, spec.z, spec.source, sol.voltages[b], P[b], Q[b])
        fig["res"] = max(fig["res"], res); fig["bal"] = max(fig["bal"], abs(ploss - float(sol.losses[b])))
    c = _c_oracle(case, 1) if spec.n > 3000 else None
    if c is not None:
        fig["cdv"] = float(np.max(np.abs(sol.voltages[1:] - c["voltages"])))
    print(f"GS3FORMS A {case.name}/{kernel}: oracle instances {len(refs)} of {case.B}, iterations {sol.iterations.min()}..{sol.iterations.max()}, "
          f"worst |dV| {fig['dv']:.2e}, |dlosses| {fig['dl']:.2e}, |dmismatch| {fig['dmm']:.2e}, iteration differences {fig['dit']}, "
          f"residual {fig['res']:.2e}, |sum P - losses| {fig['bal']:.2e}, C oracle |dV| {fig['cdv']:.2e} ({'used' if c is not None else 'not used'})")
    assert all(r["converged"] for r in refs)
    assert fig["dit"] == 0
    assert fig["dv"] < 1e-10 and fig["dl"] < 1e-10 and fig["dmm"] < 1e-12
    assert fig["res"] < 1e-8 and fig["bal"] < 1e-8
    if c is not None:
        assert c["converged"].all() and (c["iterations"] == sol.iterations[1:]).all()
        assert fig["cdv"] < 1e-10 and np.max(np.abs(c["losses"] - sol.losses[1:])) < 1e-10


@pytest.mark.parametrize("case", [c for c in G.CASES if c.form[0]], ids=lambda c: c.name)
def test_gpu_the_forms_agree(case, monkeypatch):
    """(B) the resident kernel as selected, the resident kernel with per-position mutual terms and the level kernel: the same
    iteration counts and flags, voltages, losses and mismatch to 1e-12."""
    ref, dref = _solve(case, "levels", monkeypatch)
    assert dref["kernel"] == "fbs3" and ref.converged.all()
    for kernel in ("default", "resident-dense"):
        a, da = _solve(case, kernel, monkeypatch)
        assert da["kernel"] == "fbs3_resident" and da["positions_per_thread"] == case.form[0]
        assert da["mutual_per_thread"] == (case.form[1] if kernel == "default" else 0)
        dv, dl = float(np.max(np.abs(a.voltages - ref.voltages))), float(np.max(np.abs(a.losses - ref.losses)))
        dmm = float(np.max(np.abs(a.max_mismatch - ref.max_mismatch)))
        print(f"\nGS3FORMS B {case.name}: {kernel} <{da['positions_per_thread']},{da['mutual_per_thread']}> x {da['threads']} vs levels "
              f"(lds_messages {dref['lds_messages']}): |dV| {dv:.2e}, |dlosses| {dl:.2e}, |dmismatch| {dmm:.2e}, "
              f"iterations equal {bool((a.iterations == ref.iterations).all())}")
        assert (a.iterations == ref.iterations).all() and (a.converged == ref.converged).all()
        assert dv < 1e-12 and dl < 1e-12 and dmm < 1e-12


def _same(a, b, rows=slice(None)):
    return all(np.array_equal(getattr(a, f)[rows], getattr(b, f)[rows], equal_nan=True)
               for f in ("converged", "iterations", "voltages", "losses", "max_mismatch"))


@pytest.mark.parametrize("kernel", ["resident", "levels"])
@pytest.mark.parametrize("name", ["w257", "r9_list_sparse"])
def test_gpu_one_handle_many_solves(name, kernel, monkeypatch):
    """(C) what bench.py does -- one handle, solve after solve: a solve returns what a fresh handle returns whatever the handle
    solved before (an early exit, a non-finite instance, an upload without Q).  Bit for bit: both kernels reduce in a fixed order."""
    case = G.BY_NAME[name]
    d = case.get()
    spec, P, Q = d["spec"], d["P"], d["Q"]
    s = _solver(monkeypatch, kernel, tolerance=TOL, max_iterations=MAX_IT)
    one = s.solve_batch(spec, P, Q)
    handle = s._h.value
    assert one.converged.all() and one.iterations.min() >= 5
    idle = s.solve_batch(spec, np.zeros_like(P), np.zeros_like(Q))                 # the early exit: the flat start is the answer
    assert idle.converged.all() and (idle.iterations == 1).all() and (idle.max_mismatch == 0).all()
    Pn = P.copy()
    node = int([b for b in np.nonzero(spec.phases == 7)[0] if b != spec.source][-1])
    Pn[1, node, 1] = np.nan
    bad = s.solve_batch(spec, Pn, Q)
    assert list(bad.converged) == [b != 1 for b in range(case.B)] and not np.isfinite(bad.max_mismatch[1])
    assert _same(bad, one, [0, 2])
    noq = s.solve_batch(spec, P, None)
    again = s.solve_batch(spec, P, Q)
    assert s._h.value == handle                                                    # one handle all along
    assert _same(again, one)
    fresh = _solver(monkeypatch, kernel, tolerance=TOL, max_iterations=MAX_IT)
    zero_q = fresh.solve_batch(spec, P, np.zeros_like(Q))
    assert fresh.describe() == s.describe()
    fresh.close()
    assert zero_q.converged.all() and _same(noq, zero_q) and not _same(noq, one)
    # the measurement path: upload once, solve on the device repeatedly, download
    s.timing_read()
    s.upload(spec, P, Q)
    for _ in range(3):
        s.solve_device()
    got = s.download()
    assert s._h.value == handle and _same(got, one)
    ms, launches = s.timing_read()
    assert launches == 3 and np.isfinite(ms) and ms > 0
    s.close()


def _refusal_cases():
    base = G.BY_NAME["r3_padded"].get()["spec"]
    n = base.n
    kids = np.bincount(base.parent[base.parent >= 0], minlength=n)
    leaves = [b for b in range(n) if kids[b] == 0]

    def variant(**kw):
        f = dict(parent=base.parent.copy(), phases=base.phases.copy(), z=base.z.copy(), source=base.source)
        f.update(kw)
        return G.FeederCase("refused", f["parent"], f["phases"], f["z"], f["source"], base.v_source)

    out = []
    c = next(b for b in leaves if base.phases[base.parent[b]] in (1, 2, 4))
    ph = base.phases.copy(); ph[c] = 7
    out.append(("child phase outside its parent's", variant(phases=ph), rf"node {c} "))
    leaf = leaves[len(leaves) // 2]
    ph = base.phases.copy(); ph[leaf] = 0
    out.append(("phase mask 0", variant(phases=ph), rf"node {leaf} "))
    out.append(("source without all three phases",
                G.FeederCase("refused", np.array([2, 2, -1, 0], dtype=np.int32), np.array([1, 1, 3, 1], dtype=np.uint8),
                             base.z[:4].copy(), 2, base.v_source), "source must carry all three phases"))
    pa = base.parent.copy(); pa[base.source] = leaf
    out.append(("source with a parent", variant(parent=pa), "source must have parent -1"))
    a, b = next((a, b) for i, a in enumerate(leaves) for b in leaves[i + 1:] if base.phases[a] == base.phases[b])
    pa = base.parent.copy(); pa[a], pa[b] = b, a
    out.append(("two-node cycle off the tree", variant(parent=pa), rf"not a tree rooted at the source \({n - 2} of {n} nodes reachable\)"))
    two = int(np.nonzero(np.isin(base.phases, (3, 5, 6)))[0][0])
    z = base.z.copy(); z[two] = (0.5 + 0.25j) * np.ones((3, 3))
    out.append(("singular two-phase block", variant(z=z), rf"node {two} has a singular impedance block"))
    out.append(("a single node", G.FeederCase("refused", np.array([-1], dtype=np.int32), np.array([7], dtype=np.uint8),
                                              np.zeros((1, 3, 3), dtype=complex), 0, base.v_source), r"at least one more node \(n = 1\)"))
    return out


def test_gpu_create_refuses_what_is_not_a_feeder(monkeypatch):
    """(D) gs3_create's refusals: each raises PowerFlowError naming the node or the reason, and the solver object solves a proper
    feeder afterwards as if nothing had happened."""
    case = G.BY_NAME["r3_padded"]
    d = case.get()
    spec, P, Q = d["spec"], d["P"][:2], d["Q"][:2]
    s = _solver(monkeypatch, "resident", tolerance=TOL, max_iterations=MAX_IT)
    good = s.solve_batch(spec, P, Q)
    assert good.converged.all()
    for what, bad, message in _refusal_cases():
        with pytest.raises(PowerFlowError, match=message):
            s.solve_batch(bad, np.zeros((2, bad.n, 3)))
        after = s.solve_batch(spec, P, Q)
        assert _same(after, good), what
    s.close()
