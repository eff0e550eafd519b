"""The checkFeas-bound fixtures (tests/feas_edge_ref.py) on the CPU: the yardstick
is right and the cases discriminate, before tests/test_gpu_feas_edge.py compares
a kernel with them.

For every row of every fixture the oracle's "on" result is (h, status) = (1, 1)
and its "over" result differs; most rows are exactly on the bound; the oracle's
feasible() and terminate() equal the compiled reference's on every one of those
cases and on the non-finite table; and the wrong restatements of the rule a
kernel could hold are contradicted by the fixtures.

The third restatement the tests were asked to tell apart, fmaxf for the
reference's max, cannot be told apart by any input: max's first operand,
(float)(1e-6 * Kp), is NaN only when Kp is, and then Kp + max(...) is NaN under
either max; the second operand, (float)1e-6, is never NaN.  test_fmaxf_is_the_same_function
asserts that instead, over the fixtures, the non-finite table and a sweep of
the float range.
"""
from __future__ import annotations

import numpy as np
import pytest

import feas_edge_ref as F
from conftest import assert_bitwise
from feas_edge_ref import CAPPED, DONE, ON, OVER
from oracle import REF_SO, Reference

needs_ref = pytest.mark.skipif(not REF_SO.exists(), reason="oracle/_ref not built (no reference sources)")

A_FIXTURES = list(F.A_USED)  # (copies of the bundled example, padding rows): every TypeA the GPU tests use
B_FIXTURES = list(F.TYPE_B)


def a_id(f):
    return f"{28 * f[0] + f[1]}x{7 * f[0]}"


def test_threshold_is_monotone_and_edges_are_edges():
    """thr over a sweep of the float ordering, and k_edge / k_over of a spread of g: thr(k_edge) >= g > thr(k_over),
    so k_edge is the smallest feasible Kp and k_over the largest infeasible one."""
    rng = np.random.default_rng(0)
    keys = np.sort(rng.integers(-F.KEY_INF, F.KEY_INF, 20000))
    t = np.array([F.thr(F._unkey(int(k))) for k in keys], np.float32)
    assert np.all(t[1:] >= t[:-1])
    gs = [0.0, -0.0, 1e-7, -1e-7, 1e-6, 1e-3, 1.0, -1.0, 22.46, -21.29, 1e4, -1e4, 3e38, -3e38]
    gs += list(rng.uniform(-64, 64, 200).astype(np.float32))
    for g in gs:
        ke, ko = F.k_edge(g), F.k_over(g)
        assert F.thr(ke) >= np.float32(g) > F.thr(ko), (g, ke, ko)
        assert F._key(ke) - F._key(ko) == 1
        assert not F.infeasible_row(g, ke) and F.infeasible_row(g, ko)


@pytest.mark.parametrize("fix", A_FIXTURES, ids=a_id)
def test_type_a_on_stops_and_over_differs(orc, fix):
    a = F.type_a(orc, *fix)
    assert a.cold_h == (313 if fix[0] <= F.TILED_FROM else None)  # the stack stops where the bundled example stops
    assert not a.Ystar[28 * fix[0]:].any()  # a padding row's zero stayed zero
    rows = range(a.N) if F.A_USED[fix] is None else F.A_USED[fix]
    n_on = 0
    for i in rows:
        on, over = a.want(i, ON), a.want(i, OVER)
        assert (on[0], on[1]) == (1, DONE), (fix, i, on[:2])
        assert (over[0], over[1]) != (1, DONE), (fix, i, over[:2])
        assert np.isfinite(on[4]) and np.isfinite(on[5])
        assert_bitwise(on[2], a.Ystar, "a stop at h = 1 returns the start")
        n_on += F.on_bound(a.g[i])
    assert 4 * n_on >= 3 * len(rows), (fix, n_on, len(rows))
    assert n_on == len(rows)  # (the bundled stacks: every row)
    kinds = {(abs(a.want(i, OVER)[0]), a.want(i, OVER)[1]) for i in rows}
    assert kinds <= {(F.CAP + 1, CAPPED), (2, DONE)}, kinds  # capped, or feasible again at the next iterate
    assert (F.CAP + 1, CAPPED) in kinds


@pytest.mark.parametrize("fix", A_FIXTURES[:3], ids=a_id)
def test_type_a_special_bounds(orc, fix):
    """Kp = NaN or +inf on a row: feasible, the solve stops at h = 1; -inf: infeasible."""
    a = F.type_a(orc, *fix)
    for i in (0, a.N // 2, a.N - 1):
        for label in ("nan", "+inf"):
            w = a.want(i, label)
            assert (w[0], w[1]) == (1, DONE), (fix, i, label, w[:2])
        w = a.want(i, "-inf")
        assert (w[0], w[1]) != (1, DONE), (fix, i, w[:2])


@pytest.mark.parametrize("name", B_FIXTURES)
def test_type_b_on_stops_and_over_differs(orc, name):
    b = F.type_b(orc, name)
    assert b.cold_h == 313
    assert not b.Ystar[b.positions].any(), "a zero stays zero under the multiplicative update"
    assert sum(F.on_bound(b.g[p]) for p in b.positions) * 4 >= 3 * len(b.positions)
    assert b.B == 2 * len(b.positions) + 2
    for s in range(b.B):
        P, w = b.want(s)
        assert_bitwise(P["Qd"], b.P["Qd"], f"{name} state {s}: Qd after the edit of Kp")
        assert_bitwise(P["Qp"], b.P["Qp"], f"{name} state {s}: Qp")
        pos, label = b.labels[s]
        if label == OVER:
            assert (w[0], w[1]) != (1, DONE), (name, pos, w[:2])
        else:
            assert (w[0], w[1]) == (1, DONE) and np.isfinite(w[4]) and np.isfinite(w[5]), (name, pos, label, w[:2])
            assert_bitwise(w[2], b.Ystar, "a stop at h = 1 returns the start")
        if pos is not None:  # the probe row's Fd is the only thing that moved
            moved = np.nonzero(P["Fd"].view(np.uint32) != b.P["Fd"].view(np.uint32))[0]
            assert set(moved.tolist()) <= {pos}, (name, pos, moved)
            assert_bitwise(P["Md"], b.P["Md"], "Md")


@pytest.mark.parametrize("name", ["kind1", "mid-A"])
def test_type_b_rollout_yardstick(orc, name):
    """K = 2 closed-loop steps per state: step 0 is want()'s, and the states are finite where the step stopped
    with costs."""
    b = F.type_b(orc, name)
    for s in range(b.B):
        r, (_, w) = b.loop(s), b.want(s)
        assert int(r["h"][0]) == abs(w[0]) and int(r["status"][0]) == w[1]
        assert np.array_equal(np.isnan(r["Ys"][0]), np.isnan(w[2]))
        if b.labels[s][1] != OVER:
            assert np.isfinite(r["X"]).all()


@needs_ref
@pytest.mark.parametrize("fix", A_FIXTURES, ids=a_id)
def test_type_a_oracle_is_the_reference(orc, fix):
    ref = Reference()
    a = F.type_a(orc, *fix)
    for i, label in a.cases(F.A_USED[fix]) + a.special_cases((0, a.N - 1)):
        P = a.problem(i, label)
        want_feasible = label in (ON, "nan", "+inf")
        assert orc.feasible(a.Ustar, P["Gp"], P["Kp"], a.N, a.M) == ref.feasible(a.Ustar, P) == int(want_feasible), (fix, i, label)
        flag, U, _, _ = orc.terminate(a.Ystar, *[P[k] for k in ("Qd", "Fd", "Md", "Qp", "Qp_inv", "Fp", "Mp", "Gp", "Kp")],
                                      a.N, a.M)
        rflag, rU = ref.terminate(a.Ystar, P)
        assert flag == rflag == int(want_feasible), (fix, i, label, flag, rflag)
        assert_bitwise(U, rU, "U")


@needs_ref
@pytest.mark.parametrize("name", B_FIXTURES)
def test_type_b_oracle_is_the_reference(orc, name):
    ref = Reference()
    b = F.type_b(orc, name)
    for s in range(b.B):
        P, _ = b.want(s)
        want_feasible = b.labels[s][1] != OVER
        assert orc.feasible(b.Ustar, P["Gp"], P["Kp"], b.N, b.M) == ref.feasible(b.Ustar, P) == int(want_feasible), (name, s)
        flag, U, _, _ = orc.terminate(b.Ystar, *[P[k] for k in ("Qd", "Fd", "Md", "Qp", "Qp_inv", "Fp", "Mp", "Gp", "Kp")],
                                      b.N, b.M)
        rflag, rU = ref.terminate(b.Ystar, P)
        assert flag == rflag == int(want_feasible), (name, s, flag, rflag)
        assert_bitwise(U, rU, "U")


def nonfinite_table():
    return [(g, k) for g in F.NONFINITE_G for k in F.NONFINITE_KP]


def test_nonfinite_table_oracle(orc):
    """One decisive row: the oracle, the restated rule and the table in words agree on all 24 pairs."""
    for g, k in nonfinite_table():
        U, Gp, Kp = F.one_row_case(5, 3, 4, g, k)
        got = orc.feasible(U, Gp, Kp, 5, 3)
        assert got == F.nonfinite_expected(g, k) == int(not F.infeasible_row(g, k)), (g, k, got)


@needs_ref
def test_nonfinite_table_reference(orc):
    ref = Reference()
    for g, k in nonfinite_table():
        U, Gp, Kp = F.one_row_case(5, 3, 4, g, k)
        assert ref.feasible(U, dict(Gp=Gp, Kp=Kp, N=5, M=3)) == orc.feasible(U, Gp, Kp, 5, 3), (g, k)


def fixture_rows(orc):
    """(g, Kp) of every decisive row of every case the GPU tests run: the on / over rows of the fixtures and the
    non-finite table."""
    rows = []
    for fix in A_FIXTURES:
        a = F.type_a(orc, *fix)
        rows += [(a.g[i], a.value(i, v)) for i, v in a.cases(F.A_USED[fix])]
    for name in B_FIXTURES:
        b = F.type_b(orc, name)
        rows += [(b.g[p], b.Kp[s][p]) for s, (p, _) in enumerate(b.labels) if p is not None]
    return rows + nonfinite_table()


@pytest.mark.parametrize("mutant", [">=", "!(g <= thr)"])
def test_wrong_restatements_are_contradicted(orc, mutant):
    """A kernel holding `>=` for `>` is wrong on every row that is exactly on the bound; one holding
    `!(g <= thr)` on every NaN row."""
    wrong = [(g, k) for g, k in fixture_rows(orc) if F.MUTANTS[mutant](g, k) != F.infeasible_row(g, k)]
    assert wrong, mutant
    if mutant == ">=":
        assert all(F.thr(k) == np.float32(g) for g, k in wrong)
    else:
        assert all(np.isnan(g) or np.isnan(k) for g, k in wrong)


def test_fmaxf_is_the_same_function(orc):
    """(See the module's docstring.)  Should this ever fail, the failing (g, Kp) is a case the GPU tests lack."""
    rng = np.random.default_rng(1)
    sweep = [(np.float32(1.0), F._unkey(int(k))) for k in rng.integers(-F.KEY_INF - 100, F.KEY_INF + 100, 20000)
             if abs(int(k)) <= 0x7FFFFFFF]
    nans = [(g, np.uint32(b).view(np.float32)) for g in F.NONFINITE_G for b in (0x7FC00000, 0xFFC00000, 0x7F800001)]
    for g, k in fixture_rows(orc) + sweep + nans:
        assert F.mutant_fmaxf(g, k) == F.infeasible_row(g, k), (g, k)
