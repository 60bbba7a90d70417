"""Case table of the three-phase solver's kernel forms (plain Python: neither the library nor a device is touched).

gs3_create picks one of eight kernel instantiations from the feeder alone: gs3_k_resident<K, MK> with K = 3 / 9 / 19 positions
per thread and the mutual terms either as a list dealt over the threads (MK = 3 for K = 3, else 4) or per position (MK = 0),
and the level kernel gs3_k_solve with its level messages in LDS (<true, 1>) or in HBM (<false, 1>).  ``plan_form`` restates
the selection rules; ``CASES`` holds, per form and per selection boundary, the smallest feeder that lands there by default
selection (GS3_NO_RESIDENT=1 only for the level-kernel runs).  tests/test_gs3_cases_static.py checks the table on the CPU,
tests/test_gpu_unbalanced_forms.py runs it.

Every feeder of the table is built to tell index mix-ups apart: a full asymmetric 3x3 impedance per line (``general_z``: nine
distinct entries, Z[i][j] != Z[j][i]), randomly permuted node labels (``relabel``: the source anywhere, children numbered below
their parents), an unequal, non-unit source voltage, and two-phase nodes of all three kinds with single-phase children.
"""
from dataclasses import dataclass, field
from typing import Callable, Optional

import numpy as np

V_SOURCE = (1.02, 0.99, 1.00)
LOAD_SCALES = (0.6, 1.0, 1.3)


@dataclass
class FeederCase:
    """What UnbalancedPowerFlow and the oracles read of a feeder (the fields of UnbalancedFeederSpec)."""
    name: str
    parent: np.ndarray
    phases: np.ndarray
    z: np.ndarray
    source: int = 0
    v_source: tuple = V_SOURCE

    @property
    def n(self) -> int:
        return int(len(self.parent))


def _bits(m: int) -> int:
    return (m & 1) + ((m >> 1) & 1) + ((m >> 2) & 1)


def present(phases) -> np.ndarray:
    return ((np.asarray(phases)[:, None] >> np.arange(3)[None, :]) & 1).astype(bool)


# ---------------------------------------------------------------------------------------------------------------- generators
def general_z(rng, n, scale=1.0):
    """[n, 3, 3] line impedances, nine distinct entries each: diagonal zs U(0.8, 1.2), off-diagonals of magnitude
    0.15 .. 0.45 |zs| at the angle of zs +- 0.4 rad, drawn independently for [i][j] and [j][i].  The off-diagonal row sums
    stay below 0.9 |zs| at nearly the diagonal's angle, so every principal sub-block is far from singular (the static test
    bounds the condition numbers).  Entry 0 (the source has no upstream line) is zero."""
    z = np.zeros((n, 3, 3), dtype=complex)
    for b in range(1, n):
        zs = complex(rng.uniform(0.004, 0.01), rng.uniform(0.008, 0.02)) * scale
        for i in range(3):
            for j in range(3):
                if i == j:
                    z[b, i, j] = zs * rng.uniform(0.8, 1.2)
                else:
                    z[b, i, j] = abs(zs) * rng.uniform(0.15, 0.45) * np.exp(1j * (np.angle(zs) + rng.uniform(-0.4, 0.4)))
    return z


def relabel(spec, P, Q, rng):
    """The same feeder under a random permutation of the node labels: node i becomes perm[i].  Returns (spec, P, Q, perm);
    P, Q are [B, n, 3]."""
    n = spec.n
    perm = rng.permutation(n)
    parent = np.full(n, -1, dtype=np.int32)
    phases = np.zeros(n, dtype=np.uint8)
    z = np.zeros_like(spec.z)
    for i in range(n):
        parent[perm[i]] = -1 if spec.parent[i] < 0 else perm[spec.parent[i]]
    phases[perm] = spec.phases
    z[perm] = spec.z
    Pn, Qn = np.zeros_like(P), np.zeros_like(Q)
    Pn[:, perm] = P
    Qn[:, perm] = Q
    return FeederCase(spec.name, parent, phases, z, int(perm[spec.source]), spec.v_source), Pn, Qn, perm


class _Tree:
    """A feeder under construction: node 0 is the source, parent[b] < b."""

    def __init__(self):
        self.parent, self.phases, self.tri = [-1], [7], [0]
        self.ns, self.M = 3, 0          # conductors; non-source conductors that share their node with another phase

    def add(self, p, m):
        assert 0 < m <= 7 and m & ~self.phases[p] == 0
        self.parent.append(p); self.phases.append(m)
        self.ns += _bits(m); self.M += _bits(m) if _bits(m) > 1 else 0
        if m == 7:
            self.tri.append(len(self.parent) - 1)
        return len(self.parent) - 1

    def kinds(self, under):
        """Two-phase nodes of the three kinds below the three-phase node `under`, single-phase children below them
        (11 conductors, 6 of them in the mutual count)."""
        for m in (3, 5, 6):
            t = self.add(under, m)
            for ph in range(3):
                if (m >> ph) & 1 and (m != 5 or ph == 2):
                    self.add(t, 1 << ph)

    def fill(self, rng, ns, M, window=40):
        """Grow to exactly `M` mutual conductors (two- and three-phase nodes below recent three-phase nodes), then to exactly
        `ns` conductors (single-phase nodes below recent nodes: laterals and chains of them)."""
        assert M - self.M != 1 and M >= self.M
        while self.M < M:
            r = M - self.M
            k = 2 if r in (2, 4) else 3 if r == 3 else (2 if rng.random() < 0.4 else 3)
            p = self.tri[int(rng.integers(max(0, len(self.tri) - window), len(self.tri)))]
            self.add(p, 7 if k == 3 else (3, 5, 6)[int(rng.integers(0, 3))])
        assert self.ns <= ns, (self.ns, ns)
        while self.ns < ns:
            p = int(rng.integers(max(0, len(self.parent) - window), len(self.parent)))
            on = [ph for ph in range(3) if (self.phases[p] >> ph) & 1]
            self.add(p, 1 << on[int(rng.integers(0, len(on)))])

    def level(self, rng, parents, width, tri_share=0.15, two_share=0.2):
        """One more level of exactly `width` conductors below `parents`; returns its nodes."""
        out, left = [], width
        tri = [p for p in parents if self.phases[p] == 7]
        while left > 0:
            u = rng.random()
            if left >= 8 and tri and u < tri_share:
                out.append(self.add(tri[int(rng.integers(0, len(tri)))], 7)); left -= 3
            elif left >= 8 and tri and u < tri_share + two_share:
                out.append(self.add(tri[int(rng.integers(0, len(tri)))], (3, 5, 6)[int(rng.integers(0, 3))])); left -= 2
            else:
                p = parents[int(rng.integers(0, len(parents)))]
                on = [ph for ph in range(3) if (self.phases[p] >> ph) & 1]
                out.append(self.add(p, 1 << on[int(rng.integers(0, len(on)))])); left -= 1
        return out


def _finish(name, t, rng, B, drop, seed):
    """Impedances, loads sized for a voltage drop of about `drop` at scale 1 (a linear estimate: r P + x Q of the subtree
    along the path, per phase), the batch at LOAD_SCALES with a +-10 % spread per entry, and the relabelling."""
    n = len(t.parent)
    parent, phases = np.array(t.parent, dtype=np.int32), np.array(t.phases, dtype=np.uint8)
    z = general_z(rng, n)
    pres = present(phases)
    Pn = np.where(pres, -rng.uniform(0.2, 1.0, (n, 3)), 0.0); Pn[0] = 0
    Qn = Pn * rng.uniform(0.2, 0.5, (n, 3))
    sp, sq = -Pn.copy(), -Qn.copy()
    for b in range(n - 1, 0, -1):
        sp[parent[b]] += np.where(pres[b], sp[b], 0.0); sq[parent[b]] += np.where(pres[b], sq[b], 0.0)
    zd = np.einsum("bii->bi", z)
    est = np.zeros((n, 3))
    for b in range(1, n):
        est[b] = est[parent[b]] + np.where(pres[b], zd[b].real * sp[b] + zd[b].imag * sq[b], 0.0)
    k = drop / est.max()
    lam = np.array([LOAD_SCALES[i % 3] * (1.0 + 0.005 * (i // 3)) for i in range(B)]) if B > 1 else np.array([1.0])
    Pb = lam[:, None, None] * k * Pn[None] * rng.uniform(0.9, 1.1, (B, n, 3))
    Qb = lam[:, None, None] * k * Qn[None] * rng.uniform(0.9, 1.1, (B, n, 3))
    plain = FeederCase(name, parent, phases, z)
    spec, Pr, Qr, perm = relabel(plain, Pb, Qb, np.random.default_rng(seed + 7919))
    return dict(spec=spec, P=Pr, Q=Qr, perm=perm, plain=plain, P_plain=Pb, Q_plain=Qb)


def random_tree(name, seed, ns, M, B=3, drop=0.05, window=40):
    """Random deep tree with exactly `ns` conductors of which exactly `M` share their node with another phase."""
    rng = np.random.default_rng(seed)
    t = _Tree()
    t.kinds(t.add(0, 7))
    t.fill(rng, ns, M, window)
    return _finish(name, t, rng, B, drop, seed)


def star(name, seed, w, w2, tail=8, B=3, drop=0.05):
    """The source has children worth exactly `w` conductors, a second level of exactly `w2` conductors hangs off them, and
    `tail` single-phase nodes off that."""
    rng = np.random.default_rng(seed)
    t = _Tree()
    for m in (3, 5, 6, 7, 7):
        t.add(0, m)
    l1 = list(range(1, 6)) + t.level(rng, [0], w - 12)
    l2 = [t.add(1, 1), t.add(1, 2), t.add(2, 4), t.add(3, 2), t.add(3, 4)]
    l2 += t.level(rng, l1, w2 - 5)
    t.level(rng, l2, tail, 0.0, 0.0)
    return _finish(name, t, rng, B, drop, seed)


def hub(name, seed, fan=300, B=3, drop=0.05):
    """A level-2 node with `fan` children of mixed phase sets (the fan-out is not at the source), grandchildren below some."""
    rng = np.random.default_rng(seed)
    t = _Tree()
    a = t.add(0, 7); t.add(0, 1)
    h = t.add(a, 7); t.add(a, 6)
    kids = []
    for i in range(fan):
        kids.append(t.add(h, (7, 1, 2, 4, 3, 5, 6, 1, 2, 4)[i % 10]))
    for c in kids[::3]:
        on = [ph for ph in range(3) if (t.phases[c] >> ph) & 1]
        t.add(c, 1 << on[int(rng.integers(0, len(on)))])
    for c in kids[:40:10]:
        t.add(c, 7)
    return _finish(name, t, rng, B, drop, seed)


def chain(name, seed, length=300, B=3, drop=0.05):
    """`length` three-phase nodes in a line (the source is the first), a few one- and two-phase stubs on the way."""
    rng = np.random.default_rng(seed)
    t = _Tree()
    line = [0]
    for _ in range(length - 1):
        line.append(t.add(line[-1], 7))
    for i, p in enumerate(line[10::40]):
        m = (3, 5, 6, 1, 2, 4)[i % 6]
        s = t.add(p, m)
        on = [ph for ph in range(3) if (m >> ph) & 1]
        t.add(s, 1 << on[-1])
        if i % 2 == 0:
            t.add(s, 1 << on[0])
    return _finish(name, t, rng, B, drop, seed)


# -------------------------------------------------------------------------------------------------------------- form planner
RESIDENT_MAX_CONDUCTORS = 16383
RESIDENT_LDS_BYTES = 160 * 1024          # LDS one workgroup may take on gfx950
LEVEL_THREADS = 256
LEVEL_LDS_LIMIT = 38 * 1024


def plan_form(spec, no_resident=False, dense=False):
    """What describe() reports for `spec`, from the selection rules of gs3_create (no_resident: GS3_NO_RESIDENT=1, dense:
    GS3_DENSE_MUTUAL=1), plus `level_lds_messages`: the LDS message bytes of the level kernel whichever kernel is taken."""
    n = spec.n
    kids = [[] for _ in range(n)]
    for i in range(n):
        if i != spec.source:
            kids[int(spec.parent[i])].append(i)
    level, widths = [int(spec.source)], []
    while level:
        widths.append(sum(_bits(int(spec.phases[b])) for b in level))
        level = [c for b in level for c in kids[b]]
    ns, width = sum(widths), max(widths)
    lds_messages = 32 * width if 32 * width <= LEVEL_LDS_LIMIT else 0
    K = next((k for k in (3, 9, 19) if -(-ns // k) <= 512), 0)
    threads = max(64, -(-(-(-ns // K)) // 64) * 64) if K else 0
    if K and ((((K * threads + 4) & ~3) + 72) * 16 > RESIDENT_LDS_BYTES or ns > RESIDENT_MAX_CONDUCTORS):
        K = 0
    M = sum(_bits(int(spec.phases[b])) for b in range(n) if b != spec.source and _bits(int(spec.phases[b])) > 1)
    out = dict(conductors=ns, levels=len(widths), max_level_width=width, level_lds_messages=lds_messages)
    if K and not no_resident:
        per = 3 if K == 3 else 4
        out.update(kernel="fbs3_resident", lds_messages=0, threads=threads, positions_per_thread=K, mutual_entries=M,
                   mutual_per_thread=per if (M <= per * threads and not dense) else 0)
    else:
        out.update(kernel="fbs3", lds_messages=lds_messages, threads=LEVEL_THREADS, positions_per_thread=0, mutual_entries=0,
                   mutual_per_thread=0)
    return out


DESCRIBE_FIELDS = ("kernel", "conductors", "levels", "max_level_width", "lds_messages", "threads", "positions_per_thread",
                   "mutual_entries", "mutual_per_thread")


# ---------------------------------------------------------------------------------------------------------------- case table
@dataclass
class Case:
    """One row: `build()` makes the feeder and its batch; `form` = (K, MK, threads) the default selection must give ((0, 0, 256):
    the level kernel); `ns`, `M`, `width` = exact targets (None: not pinned); `levels`: also run with GS3_NO_RESIDENT=1, where
    `lds` says whether the level messages fit LDS."""
    name: str
    build: Callable[[], dict]
    form: tuple
    ns: Optional[int] = None
    M: Optional[int] = None
    width: Optional[int] = None
    levels: bool = False
    lds: bool = True
    B: int = 3
    _made: dict = field(default_factory=dict, repr=False)

    def get(self):
        """The built case (cached: the feeders and their loads are made once per process and never modified)."""
        if "full" not in self._made:
            self._made["full"] = self.build()
        return self._made["full"]

    @property
    def kernels(self):
        """The GPU cases of the row against the oracle: the default selection, and the forced level kernel where asked."""
        return ["default"] + (["levels"] if self.levels and self.form[0] else [])


def _row(name, fn, form, ns=None, M=None, width=None, levels=False, lds=True, B=3, **kw):
    if fn is random_tree:
        kw = dict(kw, ns=ns, M=M)
    return Case(name, (lambda: fn(name, B=B, **kw)), form, ns, M, width, levels, lds, B)


CASES = [
    # (drop: the larger random trees need a heavier loading for the oracle's first instance to take five sweeps)
    # resident <3, 3>: a last thread row that is mostly padding (193 of 384 positions), and none at all (1536 = 3 x 512)
    _row("r3_padded", random_tree, (3, 3, 128), ns=193, M=60, B=70, seed=101, drop=0.06),
    _row("r3_full", random_tree, (3, 3, 512), ns=1536, M=500, seed=102),
    # resident <9, 4> just past the K = 3 limit: the list exactly full (768 = 4 x 192), and a mostly single-phase feeder
    _row("r9_list_full", random_tree, (9, 4, 192), ns=1537, M=768, seed=103),
    _row("r9_list_sparse", random_tree, (9, 4, 192), ns=1537, M=40, seed=104),
    # one entry more than the list holds: resident <9, 0> by default selection
    _row("r9_dense", random_tree, (9, 0, 192), ns=1600, M=769, seed=105),
    _row("r9_no_padding", random_tree, (9, 4, 512), ns=4608, M=1500, B=1, seed=106),
    _row("r19_list_full", random_tree, (19, 4, 256), ns=4609, M=1024, seed=107, drop=0.08),
    _row("r19_dense", random_tree, (19, 0, 256), ns=4609, M=1025, seed=108, drop=0.08),
    _row("r19_no_padding", random_tree, (19, 4, 512), ns=9728, M=2000, seed=109, drop=0.085),
    # one conductor more than any resident form takes: the level kernel by default, no environment variable
    _row("levels_by_default", random_tree, (0, 0, 256), ns=9729, M=9000, seed=110, drop=0.085),
    # level kernel (forced) at the widths where its loops change: one pass | a second pass of one slot; LDS messages | HBM messages
    _row("w256", star, (3, 3, 192), width=256, levels=True, seed=111, w=256, w2=150),
    _row("w257", star, (3, 3, 192), width=257, levels=True, seed=112, w=257, w2=150),
    _row("w1216", star, (3, 3, 512), width=1216, levels=True, seed=113, w=1216, w2=300),
    _row("w1217", star, (3, 3, 512), width=1217, levels=True, lds=False, seed=114, w=1217, w2=300),
    _row("hub", hub, (3, 3, 192), levels=True, seed=115),
    _row("chain", chain, (3, 3, 320), levels=True, seed=116),
]
BY_NAME = {c.name: c for c in CASES}


def instantiations(case):
    """The kernel instantiations the GPU tests launch for a row: default selection, GS3_DENSE_MUTUAL=1 and GS3_NO_RESIDENT=1
    where the row has a resident form (the forms-agree test), else the level kernel alone."""
    K, MK, _ = case.form
    lvl = "gs3_k_solve<%s,1>" % ("true" if case.lds else "false")
    if not K:
        return {lvl}
    return {"gs3_k_resident<%d,%d>" % (K, MK), "gs3_k_resident<%d,0>" % K, lvl}
