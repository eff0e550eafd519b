"""Fixtures and yardstick of the checkFeas-bound tests (tests/test_feas_edge_ref.py,
tests/test_gpu_feas_edge.py).

terminate() first runs compare (PQP_CPU.c:334-343): row i is infeasible iff

    GpU[i] > Kp[i] + max((float)(1e-6 * Kp[i]), (float)1e-6)

``thr`` restates the right-hand side in numpy float32 / float64, operation for
operation; it is monotone non-decreasing over the floats, so for a row value g

    k_edge(g)  the smallest float k with thr(k) >= g (bisection over the float
               ordering): the row is feasible, and "on the bound" when
               thr(k_edge) == g exactly;
    k_over(g)  nextbelow(k_edge(g)): thr < g, infeasible by the smallest amount
               a float Kp can express.

Two kinds of fixture hold a g that does not move when Kp_i moves:

  A  (``TypeA``) Kp is an input beside Fd -- pqp_problem_*, pqp_batch_solve_from,
     pqp_shared_solve with a per-state d_Kp, the drop-ins: the bundled example
     stacked k times (oracle.block_diag_problem), warm from its own Y*, where
     the reference loop stops at h = 1; any row is put on the bound or one step
     over by editing Kp_i alone.
  B  (``TypeB``) Fd is derived from Kp inside the launch -- the plant steps and
     the rollouts: probe rows (entries in {-1, 0, 1}, Kp = 1e4) are added to the
     plant's Gp, and the solve starts from Y = 0 on them.  A zero stays zero
     under the multiplicative update, so the probe rows' Fd enters no iterate
     and no cost, and their Kp is free.

Every expectation is warm_ref.ref_solve_full / stop_ref.ref_plant_loop over the
oracle at max_updates = 3, computed once per variant and never written.  Nothing
here touches the GPU or loads the library (of pqp_amd only the numpy helper
horizon_plant is called).
"""
from __future__ import annotations

import numpy as np

import stop_ref
from conftest import EXAMPLE_DIR
from oracle import block_diag_problem
from plant_horizon_ref import plant_problem
from plant_widths_ref import seeded_dynamics
from warm_ref import CAPPED, DONE, ref_solve_full

ON, OVER = "on", "over"
VARIANTS = (ON, OVER)
CAP = 3          # max_updates of every case
LOOSE = 1e4      # Kp of a probe / padding row before a case edits it
TILED_FROM = 16  # stacks of more copies take the bundled example's Y* tiled (no cold solve of the stack)
SPECIAL = {"nan": float("nan"), "+inf": float("inf"), "-inf": float("-inf")}  # Kp values read by checkFeas only
TOL64 = np.float64(1e-6)
TOL32 = np.float32(1e-6)
KEY_INF = 0x7F800000


# ---- the rule ------------------------------------------------------------------------------------
def max_ref(a, b):
    """PQP_CPU.c:32-36: (a > b) ? a : b -- a NaN first operand gives b, a NaN second operand is returned."""
    return a if a > b else b


def thr(k) -> np.float32:
    """Kp + max((float)(1e-6 * Kp), (float)1e-6): the double product rounded to float, a float add."""
    k = np.float32(k)
    with np.errstate(all="ignore"):
        return np.float32(k + max_ref(np.float32(TOL64 * np.float64(k)), TOL32))


def infeasible_row(g, k) -> bool:
    """compare's verdict on one row (PQP_CPU.c:338)."""
    return bool(np.float32(g) > thr(k))


# the three wrong restatements the fixtures must tell from the rule (tests/test_feas_edge_ref.py)
def mutant_ge(g, k) -> bool:
    return bool(np.float32(g) >= thr(k))


def mutant_not_le(g, k) -> bool:
    return not bool(np.float32(g) <= thr(k))


def mutant_fmaxf(g, k) -> bool:
    """fmaxf for the reference's max: a NaN operand is dropped, whichever side it is on."""
    k = np.float32(k)
    with np.errstate(all="ignore"):
        return bool(np.float32(g) > np.float32(k + np.fmax(np.float32(TOL64 * np.float64(k)), TOL32)))


MUTANTS = {">=": mutant_ge, "!(g <= thr)": mutant_not_le, "fmaxf": mutant_fmaxf}


def _key(f) -> int:
    """The float ordering as integers: -inf .. -0 = +0 .. +inf -> -KEY_INF .. 0 .. KEY_INF."""
    b = int(np.float32(f).view(np.uint32))
    return -(b & 0x7FFFFFFF) if b >> 31 else b


def _unkey(i: int) -> np.float32:
    return np.uint32(i if i >= 0 else (0x80000000 | -i)).view(np.float32)


def k_edge(g) -> np.float32:
    """The smallest float k with thr(k) >= g (g finite)."""
    g = np.float32(g)
    assert np.isfinite(g)
    lo, hi = -KEY_INF, KEY_INF  # thr(-inf) = -inf < g <= thr(+inf)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if thr(_unkey(mid)) >= g:
            hi = mid
        else:
            lo = mid
    return _unkey(hi)


def k_over(g) -> np.float32:
    """nextbelow(k_edge(g))."""
    return _unkey(_key(k_edge(g)) - 1)


def on_bound(g) -> bool:
    return bool(thr(k_edge(g)) == np.float32(g))


def g_rows(orc, Gp, U, N, M) -> np.ndarray:
    """Gp U in the reference's order (matrixMultiply: from +0, index order, rounded products)."""
    return orc.matmul(Gp, 0, U, 0, N, M, 1)


def kp_tables(g) -> tuple:
    """(K_edge, K_over) of every row value (each distinct value bisected once)."""
    memo: dict = {}
    for v in g:
        b = int(np.float32(v).view(np.uint32))
        if b not in memo:
            memo[b] = (k_edge(v), k_over(v))
    pairs = [memo[int(np.float32(v).view(np.uint32))] for v in g]
    return np.array([p[0] for p in pairs], np.float32), np.array([p[1] for p in pairs], np.float32)


def frozen(a):
    a = np.ascontiguousarray(a)
    a.setflags(write=False)
    return a


def same_float(a, b) -> bool:
    a, b = np.float32(a), np.float32(b)
    return bool((np.isnan(a) and np.isnan(b)) or a.view(np.uint32) == b.view(np.uint32))


# ---- the non-finite table ------------------------------------------------------------------------
NONFINITE_G = (1.0, float("nan"), float("inf"), float("-inf"))
NONFINITE_KP = (1.0, 0.0, -0.0, float("nan"), float("inf"), float("-inf"))


def nonfinite_expected(g, k) -> int:
    """The reference's answer (1 feasible) in words, without evaluating the rule: NaN on either side is feasible; Kp = +inf is
    feasible; Kp = -inf is infeasible unless g is -inf or NaN; g = +inf is infeasible unless Kp is NaN or +inf."""
    g, k = np.float32(g), np.float32(k)
    if np.isnan(g) or np.isnan(k):
        return 1
    if k == np.inf:
        return 1
    if k == -np.inf:
        return 1 if g == -np.inf else 0
    if g == np.inf:
        return 0
    if g == -np.inf:
        return 1
    return 0 if infeasible_row(g, k) else 1


def one_row_case(N, M, row, g, k):
    """A checkFeas input whose row `row` alone decides: U = (g, 0, ...), Gp[row] = e_0, every other row of Gp
    zero and Kp = LOOSE there.  Row `row`'s sum is g * 1 + 0 + ... = g to the bit (NaN and the infinities too:
    the other products are 0 * 0)."""
    U = np.zeros(M, np.float32)
    U[0] = g
    Gp = np.zeros((N, M), np.float32)
    Gp[row, 0] = 1.0
    Kp = np.full(N, LOOSE, np.float32)
    Kp[row] = k
    return U, Gp.reshape(-1), Kp


# ---- probe rows ----------------------------------------------------------------------------------
def probe_row(j: int, M: int) -> np.ndarray:
    """Probe row j: +1 at column j % M, -1 at column (3 j + 1) % M (where that is another column)."""
    r = np.zeros(M, np.float32)
    r[(3 * j + 1) % M] = -1.0
    r[j % M] = 1.0
    return r


def with_probe_rows(Gp, Kp, N0, M, positions):
    """Gp [N, M] and Kp [N], N = N0 + len(positions): the given rows in their order, probe rows (Kp = LOOSE)
    at `positions` of the result."""
    positions = sorted(positions)
    N = N0 + len(positions)
    assert all(0 <= p < N for p in positions) and len(set(positions)) == len(positions)
    G, K = np.zeros((N, M), np.float32), np.zeros(N, np.float32)
    src = iter(range(N0))
    Gp, Kp = np.asarray(Gp, np.float32).reshape(N0, M), np.asarray(Kp, np.float32).reshape(N0)
    for i in range(N):
        if i in positions:
            G[i], K[i] = probe_row(positions.index(i), M), LOOSE
        else:
            s = next(src)
            G[i], K[i] = Gp[s], Kp[s]
    return G.reshape(-1), K


def start_with_zeros(N, positions) -> np.ndarray:
    Y0 = np.full(N, 1000.0, np.float32)
    Y0[list(positions)] = 0.0
    return Y0


# ---- type A --------------------------------------------------------------------------------------
class TypeA:
    """The bundled example stacked k times (plus `pad` loose probe rows at the end, started from Y = 0): the
    problem P, its Y*, U*, g = Gp U*, and per row the Kp that puts it on the bound and one step over."""

    def __init__(self, orc, k: int, pad: int = 0):
        self.orc, self.k, self.pad = orc, k, pad
        base = block_diag_problem(orc.bundled_problem(EXAMPLE_DIR), k)
        N0, M = base["N"], base["M"]
        if k > TILED_FROM:
            # every block's iterate is the bundled example's own, bit for bit (block_diag_problem): Y* is its Y*
            # tiled, with no cold solve of the stack; that the reference loop stops there is want(i, ON)'s h = 1
            assert not pad
            N, P, one = N0, base, type_a(orc, 1)
            self.cold_h, Y = None, np.tile(one.Ystar, k)
            flag, U, _, _ = orc.terminate(Y, *[P[k_] for k_ in ("Qd", "Fd", "Md", "Qp", "Qp_inv", "Fp", "Mp", "Gp", "Kp")],
                                          N, M)
            assert flag == 1
            Y0 = None
        elif pad:
            N = N0 + pad
            pos = list(range(N0, N))
            Gp, Kp = with_probe_rows(base["Gp"], base["Kp"], N0, M, pos)
            Qd, Fd, Md = orc.convert_to_dual(base["Qp_inv"], Gp, Kp, base["Fp"], base["Mp"], N, M)
            P = dict(base, Gp=Gp, Kp=Kp, Qd=Qd, Fd=Fd, Md=Md, N=N)
            Y0 = start_with_zeros(N, pos)
        else:
            N, P, Y0 = N0, base, np.full(N0, 1000.0, np.float32)
        self.N, self.M = N, M
        if Y0 is not None:
            self.cold_h, _, Y, U, _, _ = ref_solve_full(orc, P, Y0, 0, max_updates=2000)
        self.P = {k_: (frozen(np.asarray(v, np.float32).reshape(-1)) if k_ not in ("N", "M") else v) for k_, v in P.items()}
        self.Ystar, self.Ustar = frozen(Y), frozen(U)
        self.g = frozen(g_rows(orc, P["Gp"], U, N, M))
        Ke, Ko = kp_tables(self.g)
        self.K = {ON: frozen(Ke), OVER: frozen(Ko)}
        self._wants: dict = {}

    def value(self, row: int, label) -> np.float32:
        """Kp of row `row` under a label: ON / OVER from the tables, or one of SPECIAL's values."""
        return np.float32(SPECIAL[label]) if label in SPECIAL else self.K[label][row]

    def kp(self, row: int, label) -> np.ndarray:
        """The problem's Kp with row `row` at the label's value."""
        Kp = self.P["Kp"].copy()
        Kp[row] = self.value(row, label)
        return Kp

    def problem(self, row: int, label) -> dict:
        return dict(self.P, Kp=self.kp(row, label))

    def want(self, row: int, label):
        """ref_solve_full's (h, status, Y, U, Jp, Jd) of the case, warm from Y*, max_updates = CAP."""
        key = (row, label)
        if key not in self._wants:
            w = ref_solve_full(self.orc, self.problem(row, label), self.Ystar, 0, max_updates=CAP)
            self._wants[key] = (w[0], w[1], frozen(w[2]), frozen(w[3]), w[4], w[5])
        return self._wants[key]

    def cases(self, rows=None) -> list:
        """(row, label) interleaved: on, over, on, over ... over the rows (default: every row)."""
        rows = range(self.N) if rows is None else rows
        return [(i, v) for i in rows for v in VARIANTS]

    def special_cases(self, rows) -> list:
        """(row, label) with Kp NaN, +inf (feasible) and -inf (infeasible) on each of the rows."""
        return [(i, v) for i in rows for v in SPECIAL]


# (copies, padding rows) -> the rows a test probes (None: every row): every TypeA the GPU tests use.  28 x 7, 56 x 14
# and 196 x 49 are the fewest copies that reach the one-wave, the LDS-resident and the global-memory kernels; 84,
# 112 and 140 rows the other builds of k_solve_mid2; 197 x 49 is off the multiples of 4; 224 x 56 is the smallest
# stack k_solve_pipe takes; 336 x 84 has more rows than k_solve_single has lanes; 1288 x 322 and 2548 x 637 are the
# smallest stacks pqp_shared_solve runs with 4 and with 2 states per workgroup.
A_USED = {
    (1, 0): None, (2, 0): None, (3, 0): None, (4, 0): None, (5, 0): None, (7, 0): None, (7, 1): None, (8, 0): None,
    (12, 0): None,
    (46, 0): (0, 63, 64, 1023, 1024, 1287),
    (91, 0): (0, 63, 64, 1023, 1024, 2547),
}
_type_a: dict = {}


def type_a(orc, k: int, pad: int = 0) -> TypeA:
    if (k, pad) not in _type_a:
        _type_a[k, pad] = TypeA(orc, k, pad)
    return _type_a[k, pad]


# ---- type B --------------------------------------------------------------------------------------
class TypeB:
    """A plant (Plant.PLANT's arrays, its state x and disturbance D) with probe rows at `positions`: the plant
    A, the problem at x, Y* (exact zeros on the probes), g, and the per-state Kp table -- state 2 j is probe j
    on the bound, state 2 j + 1 one step over, the last two states keep the plant's Kp."""

    def __init__(self, orc, A0: dict, N0: int, M: int, nd: int, ns: int, x, D, positions):
        self.orc = orc
        self.positions = sorted(positions)
        self.N, self.M, self.nd, self.ns = N0 + len(positions), M, nd, ns
        N = self.N
        Gp, Kp = with_probe_rows(A0["Gp"], A0["Kp"], N0, M, self.positions)
        self.A = {k: frozen(np.asarray(v, np.float32).reshape(-1)) for k, v in dict(A0, Gp=Gp, Kp=Kp).items()}
        self.x, self.D = frozen(np.asarray(x, np.float32).reshape(ns)), frozen(np.asarray(D, np.float32).reshape(nd))
        self.P = self.problem_at(self.x, None)
        self.cold_h, _, Y, U, _, _ = ref_solve_full(orc, self.P, start_with_zeros(N, self.positions), 0, max_updates=2000)
        self.Ystar, self.Ustar = frozen(Y), frozen(U)
        self.g = frozen(g_rows(orc, Gp, U, N, M))
        Ke, Ko = kp_tables(self.g)
        rows = []
        for p in self.positions:
            for tab in (Ke, Ko):
                r = Kp.copy()
                r[p] = tab[p]
                rows.append(r)
        rows += [Kp.copy(), Kp.copy()]
        self.Kp = frozen(np.stack(rows))
        self.B = len(rows)
        self.labels = [(p, v) for p in self.positions for v in VARIANTS] + [(None, "plain"), (None, "plain")]
        self.dyn = seeded_dynamics(ns, M, nd, N + M, bu=0.1)
        self._wants: dict = {}
        self._loops: dict = {}

    def problem_at(self, x, b) -> dict:
        """The dual problem at state x under state b's Kp (None: the plant's)."""
        return plant_problem(self.orc, self.A, self.N, self.M, self.nd, self.ns, x, self.D,
                             None if b is None else self.Kp[b])

    def want(self, b: int):
        """(P_b, ref_solve_full of it warm from Y*, max_updates = CAP)."""
        if b not in self._wants:
            P = self.problem_at(self.x, b)
            w = ref_solve_full(self.orc, P, self.Ystar, 0, max_updates=CAP)
            self._wants[b] = (P, (w[0], w[1], frozen(w[2]), frozen(w[3]), w[4], w[5]))
        return self._wants[b]

    def loop(self, b: int, K: int = 2) -> dict:
        """stop_ref.ref_plant_loop of state b: K steps from x, step 0 warm from Y*, no floor, max_updates = CAP."""
        if (b, K) not in self._loops:
            r = stop_ref.ref_plant_loop(self.orc, lambda x: self.problem_at(x, b), self.dyn, self.D, self.x, K,
                                        Y0=self.Ystar, max_updates=CAP)
            self._loops[b, K] = {k: frozen(v) for k, v in r.items()}
        return self._loops[b, K]

    def states(self):
        """x [B, ns] and D [B, nd]: the same state for every row of the Kp table."""
        return np.tile(self.x, (self.B, 1)), np.tile(self.D, (self.B, 1))


def bundled_plant(orc, H: int = 1) -> tuple:
    """(A, N, M, nd, ns, x, D) of the bundled plant stacked H times (H = 1: the example's own arrays)."""
    if H == 1:
        E = orc.load_example(EXAMPLE_DIR)
    else:
        import pqp_amd  # (a numpy-only helper)

        E = pqp_amd.horizon_plant(EXAMPLE_DIR, H)
    keys = ("Qp_inv", "Gp", "Kp", "Fp1", "Fp2", "Fp3", "Mp1", "Mp2", "Mp3", "Mp4", "Mp5", "Mp6")
    return {k: E[k] for k in keys}, E["N"], E["M"], E["nd"], E["ns"], E["x"], E["D"]


# name -> (stages H of the bundled plant, probe positions).
# kind1: 32 x 7, one wave, lane i decides row i.
# mid-A .. mid-D: the one-workgroup step (pqp_plant_mid_step.inc), one fixture per build.  Its C row wave cw takes
# rows cw * 64 + lane (crows = 64 and nCR = ceil(N / 64) at each of these N), so the shares are [0, 64), [64, 128),
# [128, N): the probes are the first and last row of each share, N - 1, and the 16- and 32-lane boundaries of a
# wave where a share leaves room.  mid-A is the smallest: the plant stacked twice + 8 probe rows.
# shared: 8 stages + 8 probes, 232 x 56, the first and last row of each run of 64 rows.
TYPE_B = {
    "kind1": (1, (0, 13, 30, 31)),
    "mid-A": (2, (0, 15, 16, 31, 32, 47, 48, 63)),
    "mid-B": (3, (0, 31, 32, 63, 64, 65, 90, 91)),
    "mid-C": (4, (0, 31, 32, 63, 64, 95, 96, 119)),
    "mid-D": (5, (0, 63, 64, 127, 128, 129, 146, 147)),
    "shared": (8, (0, 63, 64, 127, 128, 191, 192, 231)),
}
MID = ("mid-A", "mid-B", "mid-C", "mid-D")
MID_BUILD = {"mid-A": "A", "mid-B": "B", "mid-C": "C", "mid-D": "D"}  # plant_mid_ref.BUILD_WORDS' keys
_type_b: dict = {}


def type_b(orc, name: str) -> TypeB:
    if name not in _type_b:
        H, positions = TYPE_B[name]
        A, N0, M, nd, ns, x, D = bundled_plant(orc, H)
        _type_b[name] = TypeB(orc, A, N0, M, nd, ns, x, D, positions)
    return _type_b[name]

