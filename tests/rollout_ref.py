"""The closed loop's yardstick (include/pqp.h section 2j).

The state update is the reference's own primitives: three matrixMultiply
(PQP_CPU.c:84) through the oracle's ``matmul`` -- every sum from +0.0f in index
order, every product rounded before its add -- and two matrixAdd (:157),
``a + 1.0f * b``, as float32 adds: x+ = (A x + 1 Bu U) + 1 Bd D.

The closed loop of the bundled plant is the oracle's problem rebuilt at every
state (``example_at_state``, ``convert_to_dual`` where the bounds are the
caller's) and warm_ref's solve loop started from the previous step's Y, floored
before every warm start when the floor is positive.
"""
from __future__ import annotations

import numpy as np

from warm_ref import ref_solve_full

ONE = np.float32(1.0)


def ref_advance(orc, A, Bu, Bd, x, U, D) -> np.ndarray:
    """x+ [ns] of one state: A [ns*ns], Bu [ns*M], Bd [ns*nd] row-major."""
    x, U, D = (np.ascontiguousarray(np.asarray(v, np.float32)).reshape(-1) for v in (x, U, D))
    ns, M, nd = x.size, U.size, D.size
    t = orc.matmul(A, 0, x, 0, ns, ns, 1)
    v = orc.matmul(Bu, 0, U, 0, ns, M, 1)
    w = orc.matmul(Bd, 0, D, 0, ns, nd, 1)
    xn = (t + ONE * v).astype(np.float32)   # matrixAdd(t, t, v, 1)
    return (xn + ONE * w).astype(np.float32)  # matrixAdd(t, t, w, 1)


def ref_advance_batch(orc, A, Bu, Bd, x, U, D) -> np.ndarray:
    return np.stack([ref_advance(orc, A, Bu, Bd, x[b], U[b], D[b]) for b in range(len(x))])


def floored(Y, floor) -> np.ndarray:
    """y_floor > Y_i ? y_floor : Y_i (a NaN stays); Y as given for floor <= 0."""
    Y = np.asarray(Y, np.float32)
    if not floor > 0:
        return Y.copy()
    return np.where(np.float32(floor) > Y, np.float32(floor), Y).astype(np.float32)


def ref_closed_loop(orc, directory, A, Bu, Bd, x0, K, Kp=None, Y0=None, floor=0.0, max_updates=0) -> dict:
    """K steps of one state of the bundled plant (its own D at every step).
    Y0 None: step 0 is cold; else it starts warm from Y0.  Returns X [K+1, ns],
    U [K, M], h, status, Jp, Jd [K] and Y [N] (the last step's)."""
    E = orc.load_example(directory)
    N, M = E["N"], E["M"]
    x = np.ascontiguousarray(np.asarray(x0, np.float32)).reshape(-1)
    out = dict(X=[x], U=[], h=[], status=[], Jp=[], Jd=[])
    Y = None if Y0 is None else np.asarray(Y0, np.float32)
    for k in range(K):
        P = orc.example_at_state(directory, x)
        if Kp is not None:
            P["Kp"] = np.ascontiguousarray(np.asarray(Kp, np.float32))
            _, P["Fd"], P["Md"] = orc.convert_to_dual(E["Qp_inv"], E["Gp"], P["Kp"], P["Fp"], P["Mp"], N, M)
        y0 = np.full(N, 1000.0, np.float32) if Y is None else floored(Y, floor)
        h, status, Y, U, Jp, Jd = ref_solve_full(orc, P, y0, 0, max_updates=max_updates)
        x = ref_advance(orc, A, Bu, Bd, x, U, E["D"])
        out["X"].append(x)
        out["U"].append(U)
        out["h"].append(abs(h))
        out["status"].append(status)
        out["Jp"].append(Jp)
        out["Jd"].append(Jd)
    res = {k: np.asarray(v, np.float32) for k, v in out.items() if k in ("X", "U", "Jp", "Jd")}
    res.update(h=np.asarray(out["h"], np.int64), status=np.asarray(out["status"], np.int32), Y=Y)
    return res
