// pqp_shared_step.hip -- the shared plant's control step (include/pqp.h 2i):
// x, D -> Fp, Mp, Fd, Md -> the converge solve, for B states of ONE plant in
// one launch.  k_step_shared is k_solve_shared (pqp_shared_solve.hip) with a
// prologue in front of it: one workgroup owns S consecutive states, forms
// their linear terms with the bits of pqp_batch_compute_fp / _mp and
// pqp_shared_relinearize, and then runs shared_converge_loop -- the very
// function k_solve_shared runs -- to the end: the host bounds max_updates by
// one launch's budget, so there are no resume words, no pending counter and no
// init launch.
//
// Prologue arithmetic (the contract; pqp_plant_mid.hip's prologue has the same
// bits): every sum from +0.0f in index order, each product rounded before it
// is added.
//   Fp   = (Fp1 D) + 1.0f (Fp2 x);  Fp = Fp + -1.0f Fp3                 (computeFp, PQP_CPU.c:373)
//   Mp   = sum over the five ordered dots (x'Mp1).x, (D'Mp2).x, Mp4'x, (D'Mp3).D, Mp5'D of dot / 2,
//          from +0.0f, then + Mp6 / 2                                      (computeMp, :395-425)
//   Fd   = (Gp Qp_inv) Fp + 1.0f Kp                                        (:456-459)
//   Md   = sum_j (Fp'Qp_inv)_j Fp_j + -1.0f Mp                             (:475-478)
// Every matrix-vector product is a shared_product: the S operands of a k are a
// row of an [k][S] LDS image, two neighbouring states the halves of one
// v_pk_mul_f32 / v_pk_add_f32, and the matrix is read once for the S states
// from a padded k-major copy made at create.
//
// LDS: the prologue's words (x, D, x'Mp1, D'Mp2, D'Mp3, Fp, Fp'Qp_inv, each
// [.][S]) lie over the solve's per-state vectors, which are filled only after
// Md is formed.  step_shared_state_floats (pqp_shared_solve.h) is the one
// answer to how many floats a state takes, for the host and for this carve-up.
//
// Fp and Fd are outputs AND working storage: the solve loop reads them from
// the caller's d_Fp / d_Fd (LDS is full of iterates at S = 8).  They are
// written here by vector stores (global_store_dword), and read in the loop by
// other waves of the same workgroup through SharedSolveCore's plain `const
// float*` members -- vector loads (global_load_dword) at lane-dependent
// addresses, never `const __restrict__` kernel arguments, which the compiler
// may take for kernel-constant and fetch through the scalar cache.  Between
// the stores and the first load lie workgroup barriers (__syncthreads: a
// workgroup-scope release / acquire around s_barrier, vmcnt(0) before it), and
// a workgroup's waves share one CU's vector L1, so the loads see the stores.
// No other workgroup reads them in this launch.
//
// Included by pqp_kernels.hip after pqp_shared_solve.hip, whose helpers it calls.
#include "pqp_device.h"
#include "pqp_shared_solve.h"

#pragma clang fp contract(off)

namespace pqp {

namespace {

// x[k][s] (k < ld) <- src[(b0 + s) * n + k] for the block's nst states; +0.0f for a missing state and the padding
template <int S>
__device__ __forceinline__ void stage_states(float* x, const float* src, int n, int ld, int b0, int nst) {
    for (int e = threadIdx.x; e < ld * S; e += blockDim.x) {
        const int k = e / S, s = e - k * S;
        x[e] = (s < nst && k < n) ? src[(size_t)(b0 + s) * n + k] : 0.0f;
    }
}

}  // namespace

// k_step_shared and k_step_shared_tol: one text (pqp_shared_step_kernel.inc), compiled with and without the
// caller's gap tolerances (pqp.h 2k)
#define PQP_STEP_SHARED_KERNEL k_step_shared
#define PQP_STEP_SHARED_TOL false
#include "pqp_shared_step_kernel.inc"
#undef PQP_STEP_SHARED_KERNEL
#undef PQP_STEP_SHARED_TOL
#define PQP_STEP_SHARED_KERNEL k_step_shared_tol
#define PQP_STEP_SHARED_TOL true
#include "pqp_shared_step_kernel.inc"
#undef PQP_STEP_SHARED_KERNEL
#undef PQP_STEP_SHARED_TOL

int step_shared_states(int N, int M, int nd, int ns) {
    if (nd <= 0 || ns <= 0 || nd > (1 << 20) || ns > (1 << 20)) return 0;
    const int S = solve_shared_states(N, M);
    if (S == 0) return 0;
    return step_shared_lds_bytes(N, M, nd, ns, S) + kSolveSharedStaticLds <= kSolveSharedLdsBudget ? S : 0;
}

hipError_t launch_step_shared(const SharedStepArgs& a, int S, hipStream_t s) {
    const SharedSolveCore& v = a.solve;
    if (S != step_shared_states(v.N, v.M, a.nd, a.ns) || S == 0) return hipErrorInvalidValue;
    const size_t lds = step_shared_lds_bytes(v.N, v.M, a.nd, a.ns, S);
    if (shared_tol(a.abs_tol, a.rel_tol))  // a positive tolerance: the _tol build
        return launch_shared_s(k_step_shared_tol<8>, k_step_shared_tol<4>, k_step_shared_tol<2>, S, v.B, v.N, v.M, lds,
                               s, a);
    return launch_shared_s(k_step_shared<8>, k_step_shared<4>, k_step_shared<2>, S, v.B, v.N, v.M, lds, s, a);
}

}  // namespace pqp
