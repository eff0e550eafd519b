"""The warm-start yardstick: solveQuadraticDual (PQP_CPU.c:694-750) with line
:710 (initMat(Y, 1000)) replaced by Y = Y0 and nothing else changed, written
over the oracle's terminate() and update().  h starts at 1; converge mode
calls terminate(Y0) before the first update; fixed mode runs num_iter - 1
updates from Y0.  Y0 is taken as given (no clamping, no validation).
"""
from __future__ import annotations

import numpy as np

DONE, CAPPED = 1, 2  # the library's per-problem status words


def ref_solve_full(orc, P, Y0, mode=0, num_iter=1000, max_updates=0):
    """-> (h, status, Y, U, Jp, Jd).  Capped converge solves return -h, as
    Oracle.solve does; Jp / Jd are those of the last terminate() that got past
    the feasibility test (NaN if none), U is the last terminate()'s (zeros in
    fixed mode, which calls none).  max_updates <= 0: no cap."""
    N, M = int(P["N"]), int(P["M"])
    Qd, Fd = P["Qd"], P["Fd"]
    theta = orc.theta(Qd, N)
    Y = np.ascontiguousarray(np.asarray(Y0, np.float32).reshape(N)).copy()
    U = np.zeros(M, np.float32)
    Jp = Jd = float("nan")
    h = 1
    if mode == 1:
        while h < num_iter:
            Y = orc.update(Y, Qd, theta, Fd, N)
            h += 1
        return h, DONE, Y, U, Jp, Jd
    while True:
        flag, U, jp, jd = orc.terminate(Y, Qd, Fd, P["Md"], P["Qp"], P["Qp_inv"], P["Fp"], P["Mp"], P["Gp"], P["Kp"],
                                        N, M)
        if not (np.isnan(jp) and np.isnan(jd)):
            Jp, Jd = jp, jd
        if flag:
            return h, DONE, Y, U, Jp, Jd
        if 0 < max_updates <= h - 1:
            return -h, CAPPED, Y, U, Jp, Jd
        Y = orc.update(Y, Qd, theta, Fd, N)
        h += 1


def ref_solve_from(orc, P, Y0, mode=0, num_iter=1000, max_updates=0):
    """-> (h, status, Y, U): the reference loop started from Y0."""
    return ref_solve_full(orc, P, Y0, mode, num_iter, max_updates)[:4]
