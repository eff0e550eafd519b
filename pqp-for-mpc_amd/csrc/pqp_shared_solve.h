// pqp_shared_solve.h -- internal interface of the shared-plant converge solve
// (pqp_shared_solve.hip: k_solve_shared, k_relin_shared) and of the shared
// plant's control step (pqp_shared_step.hip: k_step_shared) to the host shim.
// Not part of the C ABI.  (Beside pqp_launch.h, not in it: that header's text
// is part of the key of the kernels' recorded counter measurements, which
// these declarations do not touch.)
#pragma once
#include "pqp_launch.h"

namespace pqp {

constexpr size_t kSolveSharedLdsBudget = 160 * 1024;
constexpr size_t kSolveSharedStaticLds = 1024;  // k_solve_shared's per-state control words (at most)

__host__ __device__ inline int shared_round4(int n) { return (n + 3) & ~3; }
// LDS floats one state takes in k_solve_shared: two iterate images, tq and the
// Fd.Y terms ([ldq] each), and Gp'Y + Fp, U and U'Qp ([ldm] each).  The host's
// LDS check and the kernel's carve-up both go through this.
__host__ __device__ inline size_t solve_shared_state_floats(int N, int M) {
    return (size_t)4 * shared_round4(N) + (size_t)3 * shared_round4(M);
}
inline size_t solve_shared_lds_bytes(int N, int M, int S) {
    return (size_t)S * solve_shared_state_floats(N, M) * sizeof(float);
}
// States per workgroup k_solve_shared uses for the shape (8, 4 or 2); 0 where it is not supported.
int solve_shared_states(int N, int M);

// Per-state resume words of a shared solve (one per state, device memory).
struct SharedSolveState {
    long long h;   // reference's h of the current iterate (starts at 1)
    int status;    // SolveStatus
    int pad;
    float Jp, Jd;  // costs of the last terminate() that passed checkFeas (NaN: none yet)
};

// All device pointers.  The plant's matrices, each padded to a multiple of 4
// floats per row and laid out so that one lane's two (or one) output rows of a
// product are neighbours in memory for every k:
//   QdT  [N][ldq] column-major Qd (the update; QdR itself when Qd is bit-symmetric)
//   QdR  [N][ldq] row-major Qd (Y'Qd)          GpP  [N][ldm] row-major Gp (Gp'Y)
//   GpT  [M][ldq] Gp' (checkFeas)              QinvT [M][ldm] Qp_inv' (U)
//   QpP  [M][ldm] row-major Qp (U'Qp)
struct SharedSolveCore {
    const float *QdT, *QdR, *theta, *GpP, *GpT, *QinvT, *QpP, *Kp;
    const float *Fd, *Md, *Fp, *Mp, *KpB;  // per state: [B][N], [B], [B][M], [B], NULL or [B][N]
    float *Y, *U;                          // [B][N] (in: the iterate to continue from), [B][M]
    long long* h;                          // optional outputs, written when a state finishes
    int* status;
    float *Jp, *Jd;
    SharedSolveState* st;
    int* pending;  // +1 per workgroup with a state still running when the launch ends
    int N, M, ldq, ldm, B, sym;
    long long max_updates, chunk;
};
// k_solve_shared's argument: the above, then the gap tolerances (pqp.h 2k; both 0: the reference's rule alone).
// They come last here and in SharedStepArgs, which embeds the core without them, so that every word the kernels
// read before the tolerances existed keeps its place in the kernel arguments.
struct SharedSolveArgs : SharedSolveCore {
    float abs_tol, rel_tol;
};
// A solve or step with a positive tolerance runs the kernels' _tol build (k_solve_shared_tol, k_step_shared_tol);
// every other one the build without the tolerances, whose instructions are those it had before them.
inline bool shared_tol(float abs_tol, float rel_tol) { return abs_tol > 0.0f || rel_tol > 0.0f; }
// st[b] = {h = 1, running, no costs}; Y[b] = Y0[b] (NULL: 1000; Y itself: kept)
hipError_t launch_shared_solve_init(int B, int N, SharedSolveState* st, const float* Y0, float* Y, hipStream_t s);
// one bounded launch: every running state advances by at most a.chunk iterates
hipError_t launch_solve_shared(const SharedSolveArgs& a, int S, hipStream_t s);

// Fd [B][N], Md [B] of B states in ONE launch.  GQT [M][ldq] (Gp Qp_inv)', QinvR [M][ldm] row-major Qp_inv.
struct SharedRelinArgs {
    const float *GQT, *QinvR, *Kp;
    const float *Fp, *Mp, *KpB;
    float *Fd, *Md;
    int N, M, ldq, ldm, B;
};
hipError_t launch_relin_shared(const SharedRelinArgs& a, int S, hipStream_t s);

// ---- the control step (pqp_shared_step.hip: k_step_shared; pqp.h 2i) ----
// LDS floats one state's prologue words take: x, x'Mp1, D'Mp2 ([round4(ns)] each), D, D'Mp3
// ([round4(nd)] each), Fp and Fp'Qp_inv ([ldm] each).  They lie over the solve's vectors, which
// are dead then, so a state takes the larger of the two.  step_shared_states, the launcher's LDS
// size and the kernel's carve-up all go through these.
__host__ __device__ inline size_t step_shared_prologue_floats(int M, int nd, int ns) {
    return (size_t)3 * shared_round4(ns) + (size_t)2 * shared_round4(nd) + (size_t)2 * shared_round4(M);
}
__host__ __device__ inline size_t step_shared_state_floats(int N, int M, int nd, int ns) {
    const size_t a = solve_shared_state_floats(N, M), b = step_shared_prologue_floats(M, nd, ns);
    return a > b ? a : b;
}
inline size_t step_shared_lds_bytes(int N, int M, int nd, int ns, int S) {
    return (size_t)S * step_shared_state_floats(N, M, nd, ns) * sizeof(float);
}
// States per workgroup k_step_shared uses: solve_shared_states(N, M) where the prologue's words
// for that many states fit the launch's LDS too, else 0.
int step_shared_states(int N, int M, int nd, int ns);

// All device pointers.  `solve` as for k_solve_shared, with Fp / Fd the same buffers as below, Md, Mp,
// st and pending unused, chunk = max_updates.  The plant's linear-term matrices, padded and k-major:
//   Fp1T [nd][ldm] Fp1'     Fp2T [ns][ldm] Fp2'     Mp1P [ns][ldx] row-major Mp1
//   Mp2P [nd][ldx] row-major Mp2                     Mp3P [nd][ldd] row-major Mp3
//   GQT, QinvR as SharedRelinArgs;  Fp3 [M], Mp4 [ns], Mp5 [nd], Mp6 [1] as given
// (ldx = round4(ns), ldd = round4(nd)).
struct SharedStepArgs {
    SharedSolveCore solve;
    const float *Fp1T, *Fp2T, *Fp3, *Mp1P, *Mp2P, *Mp3P, *Mp4, *Mp5, *Mp6, *GQT, *QinvR;
    const float *x, *D;  // [B][ns], [B][nd]
    float *Fp, *Fd;      // [B][M], [B][N]: outputs, and what the solve loop reads
    float *Mp, *Md;      // [B] each, optional
    int nd, ns, warm;
    float abs_tol, rel_tol;  // the gap tolerances (pqp.h 2k), last: see SharedSolveArgs
};
// one launch: every state runs to its end (max_updates <= one launch's budget)
hipError_t launch_step_shared(const SharedStepArgs& a, int S, hipStream_t s);

// dst [orows][ld] <- src (row-major orows x ocols, or, transposed, ocols x orows), columns ocols..ld-1 zeroed
hipError_t launch_shared_layout(const float* src, int orows, int ocols, int transposed, float* dst, int ld,
                                hipStream_t s);

}  // namespace pqp
