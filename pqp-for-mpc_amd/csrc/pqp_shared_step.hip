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
// other waves of the same workgroup through SharedSolveArgs' plain `const
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

// grid = ceil(B / S) workgroups of blockDim.x (a multiple of 64) threads;
// dynamic LDS = S * step_shared_state_floats(N, M, nd, ns) floats.
template <int S>
__global__ void __launch_bounds__(kSolveSharedThreads) k_step_shared(SharedStepArgs T) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    __shared__ long long s_h[S];
    __shared__ int s_fin[S], s_bad[S], s_new[S];
    __shared__ float s_Jp[S], s_Jd[S], s_jp[S], s_jd[S];
    __shared__ float s_Mp[S], s_Md[S], s_dot[5 * S];
    const SharedSolveArgs& A = T.solve;
    const int tid = threadIdx.x, NT = blockDim.x;
    const int N = A.N, M = A.M, ldq = A.ldq, ldm = A.ldm;
    const int nd = T.nd, nx = T.ns, ldd = shared_round4(nd), ldx = shared_round4(nx);
    const int b0 = blockIdx.x * S;
    const int nst = (A.B - b0) < S ? (A.B - b0) : S;  // states of this block
    // ---- the prologue's words, over the solve's vectors ----
    float* xs = lds;                        // [ldx][S]  x
    float* ds = xs + (size_t)S * ldx;       // [ldd][S]  D
    float* r0 = ds + (size_t)S * ldd;       // [ldx][S]  x'Mp1
    float* r1 = r0 + (size_t)S * ldx;       // [ldx][S]  D'Mp2
    float* r3 = r1 + (size_t)S * ldx;       // [ldd][S]  D'Mp3
    float* fpx = r3 + (size_t)S * ldd;      // [ldm][S]  Fp
    float* tmp = fpx + (size_t)S * ldm;     // [ldm][S]  Fp2 x, then Fp'Qp_inv, then its terms
    stage_states<S>(xs, T.x, nx, ldx, b0, nst);
    stage_states<S>(ds, T.D, nd, ldd, b0, nst);
    __syncthreads();
    // computeFp :373.  Both products give row j to the same lane (the split depends on M and the
    // workgroup only), so Fp2 x needs no barrier before it is added.
    shared_product<S>(T.Fp2T, ldm, M, nx, xs, [&](int j, int s, float v) { tmp[(size_t)j * S + s] = v; });
    shared_product<S>(T.Fp1T, ldm, M, nd, ds, [&](int j, int s, float v) {
        float fp = v + 1.0f * tmp[(size_t)j * S + s];  // matrixAdd(Fp, Fp, tmp, 1)
        fp = fp + -1.0f * T.Fp3[j];                    // matrixAdd(Fp, Fp, Fp3, -1)
        fpx[(size_t)j * S + s] = fp;
        if (s < nst) T.Fp[(size_t)(b0 + s) * M + j] = fp;
    });
    // computeMp's row vectors :397-423
    shared_product<S>(T.Mp1P, ldx, nx, nx, xs, [&](int j, int s, float v) { r0[(size_t)j * S + s] = v; });
    shared_product<S>(T.Mp2P, ldx, nx, nd, ds, [&](int j, int s, float v) { r1[(size_t)j * S + s] = v; });
    shared_product<S>(T.Mp3P, ldd, nd, nd, ds, [&](int j, int s, float v) { r3[(size_t)j * S + s] = v; });
    __syncthreads();
    // Fd = (Gp Qp_inv) Fp + Kp :456-459 and Fp'Qp_inv :475 (k_relin_shared's body, Fp from LDS)
    shared_product<S>(T.GQT, ldq, N, M, fpx, [&](int i, int s, float v) {
        if (s < nst) {
            const float kp = A.KpB ? A.KpB[(size_t)(b0 + s) * N + i] : A.Kp[i];
            T.Fd[(size_t)(b0 + s) * N + i] = v + 1.0f * kp;  // matrixAdd(Fd, Fd, Kp) :459
        }
    });
    shared_product<S>(T.QinvR, ldm, M, M, fpx, [&](int j, int s, float v) { tmp[(size_t)j * S + s] = v; });
    // the five ordered dots that end Mp, one lane per dot and state (the last lanes: the first have the most rows)
    if (tid >= NT - 5 * S) {
        const int e = tid - (NT - 5 * S), t = e / S, s = e - t * S;
        const float* db = t < 3 ? xs : ds;  // (x'Mp1).x, (D'Mp2).x, Mp4'x, (D'Mp3).D, Mp5'D
        const int dlen = t < 3 ? nx : nd;
        float dot = 0.0f;
        if (t == 2 || t == 4) {  // the plant's vector, from global memory
            const float* dm = t == 2 ? T.Mp4 : T.Mp5;
            for (int k = 0; k < dlen; ++k) dot += dm[k] * db[(size_t)k * S + s];
        } else {  // a row vector of this state, from LDS
            const float* da = t == 0 ? r0 : (t == 1 ? r1 : r3);
            for (int k = 0; k < dlen; ++k) dot += da[(size_t)k * S + s] * db[(size_t)k * S + s];
        }
        s_dot[t * S + s] = dot;
    }
    __syncthreads();
    for (int e = tid; e < M * S; e += NT) tmp[e] = tmp[e] * fpx[e];  // :475-476
    __syncthreads();
    if (tid < S) {
        float dot = 0.0f;
        for (int j = 0; j < M; ++j) dot += tmp[(size_t)j * S + tid];
        float mp = 0.0f;
        for (int t = 0; t < 5; ++t) mp += s_dot[t * S + tid] / 2;  // k_mp_finish's order
        mp += T.Mp6[0] / 2;
        const float md = dot + -1.0f * mp;  // :478
        s_Mp[tid] = mp;
        s_Md[tid] = md;
        if (tid < nst) {
            if (T.Mp) T.Mp[b0 + tid] = mp;
            if (T.Md) T.Md[b0 + tid] = md;
        }
        // every state starts at h = 1 with no costs yet; a missing state is finished and never written
        s_h[tid] = 1;
        s_fin[tid] = tid < nst ? kStatusContinue : kStatusDone;
        s_Jp[tid] = s_Jd[tid] = __builtin_nanf("");
        s_bad[tid] = s_new[tid] = 0;
    }
    __syncthreads();  // the prologue's words are dead: the iterates, Y = 1000 (:710) or the caller's rows
    float* ya = lds;                   // [ldq][S]
    float* yb = ya + (size_t)S * ldq;  // [ldq][S]
    for (int s = 0; s < S; ++s) {
        const float* y0 = (s < nst && T.warm) ? A.Y + (size_t)(b0 + s) * N : nullptr;
        for (int i = tid; i < ldq; i += NT) {
            ya[(size_t)i * S + s] = (s < nst && i < N) ? (y0 ? y0[i] : 1000.0f) : 0.0f;
            yb[(size_t)i * S + s] = 0.0f;
        }
    }
    __syncthreads();
    const SharedSolveCtl ctl = {s_h, s_fin, s_bad, s_new, s_Jp, s_Jd, s_jp, s_jd};
    float* cur;
    shared_converge_loop<S, false>(A, b0, nst, lds, ctl, s_Md, s_Mp, cur);
}

int step_shared_states(int N, int M, int nd, int ns) {
    if (nd <= 0 || ns <= 0 || nd > (1 << 20) || ns > (1 << 20)) return 0;
    const int S = solve_shared_states(N, M);
    if (S == 0) return 0;
    return step_shared_lds_bytes(N, M, nd, ns, S) + kSolveSharedStaticLds <= kSolveSharedLdsBudget ? S : 0;
}

hipError_t launch_step_shared(const SharedStepArgs& a, int S, hipStream_t s) {
    const SharedSolveArgs& v = a.solve;
    if (S != step_shared_states(v.N, v.M, a.nd, a.ns) || S == 0) return hipErrorInvalidValue;
    const size_t lds = step_shared_lds_bytes(v.N, v.M, a.nd, a.ns, S);
    const dim3 grid((unsigned)((v.B + S - 1) / S)), block(solve_shared_threads(v.N, v.M));
    switch (S) {
        case 8: hipLaunchKernelGGL(k_step_shared<8>, grid, block, lds, s, a); break;
        case 4: hipLaunchKernelGGL(k_step_shared<4>, grid, block, lds, s, a); break;
        default: hipLaunchKernelGGL(k_step_shared<2>, grid, block, lds, s, a); break;
    }
    return hipGetLastError();
}

}  // namespace pqp
