// pqp_shared_solve.h -- internal interface of the shared-plant converge solve
// (pqp_shared_solve.hip: k_solve_shared, k_relin_shared) to the host shim.
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
struct SharedSolveArgs {
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

// dst [orows][ld] <- src (row-major orows x ocols, or, transposed, ocols x orows), columns ocols..ld-1 zeroed
hipError_t launch_shared_layout(const float* src, int orows, int ocols, int transposed, float* dst, int ld,
                                hipStream_t s);

}  // namespace pqp
