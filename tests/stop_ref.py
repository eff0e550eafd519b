"""The gap-tolerance stopping rule's yardstick (include/pqp.h section 2k).

``stop_decide`` restates the C text of the rule (pqp_device.h: gap_stop, then
tol_stop) in numpy float32 / float64, operation for operation.  The solve loop
is warm_ref.ref_solve_full's with the oracle's flag replaced by the rule's
decision over the oracle's terminate() -- (flag, U, Jp, Jd): the reference's
own decision first, then the tolerances on the costs of an iterate that passed
checkFeas (an infeasible iterate has NaN costs and matches no tolerance).  The
closed loop is rollout_ref.ref_closed_loop's over that loop, for any plant.

Nothing here touches the GPU or the library.
"""
from __future__ import annotations

import numpy as np

from rollout_ref import floored, ref_advance

CONTINUE, DONE, CAPPED, TOL = 0, 1, 2, 3  # the library's per-state status words (0: the rule's "go on")
K_TOL = np.float64(1e-6)                  # eaj = erj (PQP_CPU.c:21-22)


def gap_stop(Jp, Jd) -> bool:
    """terminate()'s gap tests (PQP_CPU.c:683-685) in the reference's order."""
    Jp, Jd = np.float32(Jp), np.float32(Jd)
    with np.errstate(all="ignore"):
        if Jp > -Jd:
            return False
        gap = np.float64(np.float32(Jp + Jd))
        if gap > K_TOL:
            return False
        return not (gap / np.abs(np.float64(Jd)) > K_TOL)


def tol_stop(Jp, Jd, abs_tol, rel_tol) -> int:
    """The caller's tolerances: TOL or CONTINUE.  The tolerances are C floats."""
    Jp, Jd = np.float32(Jp), np.float32(Jd)
    abs_tol, rel_tol = np.float32(abs_tol), np.float32(rel_tol)
    if not (abs_tol > 0) and not (rel_tol > 0):
        return CONTINUE
    with np.errstate(all="ignore"):
        gap = np.float64(np.float32(Jp + Jd))  # the float32 sum, as :683
        if gap <= np.float64(abs_tol):
            return TOL
        if gap <= np.float64(rel_tol) * np.abs(np.float64(Jd)):  # one double product, no division
            return TOL
    return CONTINUE


def stop_decide(Jp, Jd, abs_tol=0.0, rel_tol=0.0) -> int:
    """pqp_stop_decide: 0 continue, 1 the reference's tests pass, 3 within the tolerances."""
    if gap_stop(Jp, Jd):
        return DONE
    return tol_stop(Jp, Jd, abs_tol, rel_tol)


def ref_solve_full(orc, P, Y0, max_updates=0, abs_tol=0.0, rel_tol=0.0):
    """-> (h, status, Y, U, Jp, Jd): warm_ref.ref_solve_full in converge mode
    (capped solves return -h) with status TOL where a tolerance stopped it."""
    N, M = int(P["N"]), int(P["M"])
    Qd, Fd = P["Qd"], P["Fd"]
    theta = orc.theta(Qd, N)
    Y = np.ascontiguousarray(np.asarray(Y0, np.float32).reshape(N)).copy()
    U = np.zeros(M, np.float32)
    Jp = Jd = float("nan")
    h = 1
    while True:
        flag, U, jp, jd = orc.terminate(Y, Qd, Fd, P["Md"], P["Qp"], P["Qp_inv"], P["Fp"], P["Mp"], P["Gp"], P["Kp"],
                                        N, M)
        if not (np.isnan(jp) and np.isnan(jd)):
            Jp, Jd = jp, jd
        decision = DONE if flag else tol_stop(jp, jd, abs_tol, rel_tol)
        if decision:
            return h, decision, Y, U, Jp, Jd
        if 0 < max_updates <= h - 1:
            return -h, CAPPED, Y, U, Jp, Jd
        Y = orc.update(Y, Qd, theta, Fd, N)
        h += 1


def ref_plant_loop(orc, problem_at, dyn, D, x0, K, Y0=None, floor=0.0, max_updates=0, abs_tol=0.0, rel_tol=0.0) -> dict:
    """K steps of one state of a plant: problem_at(x) is the dual problem at
    state x, dyn = (A, Bu, Bd) row-major, D the disturbance of every step.  Y0
    None: step 0 is cold; else warm from Y0.  Returns X [K+1, ns], U [K, M],
    h, status, Jp, Jd [K], Y [N] (the last step's) and Ys [K, N] (every step's)."""
    A, Bu, Bd = (np.ascontiguousarray(np.asarray(m, np.float32)).reshape(-1) for m in dyn)
    x = np.ascontiguousarray(np.asarray(x0, np.float32)).reshape(-1)
    out = dict(X=[x], U=[], h=[], status=[], Jp=[], Jd=[], Ys=[])
    Y = None if Y0 is None else np.asarray(Y0, np.float32)
    for _ in range(K):
        P = problem_at(x)
        y0 = np.full(int(P["N"]), 1000.0, np.float32) if Y is None else floored(Y, floor)
        h, status, Y, U, Jp, Jd = ref_solve_full(orc, P, y0, max_updates, abs_tol, rel_tol)
        x = ref_advance(orc, A, Bu, Bd, x, U, D)
        out["X"].append(x)
        for k, v in (("U", U), ("h", abs(h)), ("status", status), ("Jp", Jp), ("Jd", Jd), ("Ys", Y)):
            out[k].append(v)
    res = {k: np.asarray(v, np.float32) for k, v in out.items() if k in ("X", "U", "Jp", "Jd", "Ys")}
    res.update(h=np.asarray(out["h"], np.int64), status=np.asarray(out["status"], np.int32), Y=Y)
    return res


def ref_closed_loop(orc, directory, A, Bu, Bd, x0, K, Kp=None, Y0=None, floor=0.0, max_updates=0, abs_tol=0.0,
                    rel_tol=0.0) -> dict:
    """rollout_ref.ref_closed_loop (the bundled plant, its own D at every step) under the rule."""
    E = orc.load_example(directory)
    N, M = E["N"], E["M"]

    def problem_at(x):
        P = orc.example_at_state(directory, x)
        if Kp is not None:
            P["Kp"] = np.ascontiguousarray(np.asarray(Kp, np.float32))
            _, P["Fd"], P["Md"] = orc.convert_to_dual(E["Qp_inv"], E["Gp"], P["Kp"], P["Fp"], P["Mp"], N, M)
        return P

    return ref_plant_loop(orc, problem_at, (A, Bu, Bd), E["D"], x0, K, Y0, floor, max_updates, abs_tol, rel_tol)
