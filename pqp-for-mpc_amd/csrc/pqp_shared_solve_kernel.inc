// pqp_shared_solve_kernel.inc -- the text of k_solve_shared (pqp_shared_solve.hip), which includes it twice:
//   PQP_SOLVE_SHARED_KERNEL k_solve_shared,     PQP_SOLVE_SHARED_TOL false: the reference's stopping rule alone
//   PQP_SOLVE_SHARED_KERNEL k_solve_shared_tol, PQP_SOLVE_SHARED_TOL true:  then the caller's gap tolerances (pqp.h 2k)
// Two kernels of one text, as pqp_plant_step.inc: with the flag compiled out, k_solve_shared's three builds
// keep the instructions they had before the tolerances existed (DESIGN.md 4k).
//
// grid = ceil(B / S) workgroups of blockDim.x (a multiple of 64) threads;
// dynamic LDS = S * solve_shared_state_floats(N, M) floats.
template <int S>
__global__ void __launch_bounds__(kSolveSharedThreads) PQP_SOLVE_SHARED_KERNEL(SharedSolveArgs A) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    __shared__ long long s_h[S];
    __shared__ int s_fin[S], s_bad[S], s_new[S];
    __shared__ float s_Jp[S], s_Jd[S], s_jp[S], s_jd[S];
    const int tid = threadIdx.x, NT = blockDim.x;
    const int N = A.N, ldq = A.ldq;
    const int b0 = blockIdx.x * S;
    const int ns = (A.B - b0) < S ? (A.B - b0) : S;  // states of this block
    if (tid < S) {
        SharedSolveState z;
        z.h = 0, z.status = kStatusDone, z.Jp = z.Jd = 0.0f;  // a missing state: finished, never written
        if (tid < ns) z = A.st[b0 + tid];
        s_h[tid] = z.h, s_fin[tid] = z.status, s_Jp[tid] = z.Jp, s_Jd[tid] = z.Jd;
        s_bad[tid] = s_new[tid] = 0;
    }
    int left = __syncthreads_count(tid < S && s_fin[tid] == kStatusContinue);
    if (left == 0) return;  // every state finished in an earlier launch
    float* ya = lds;                   // [ldq][S]
    float* yb = ya + (size_t)S * ldq;  // [ldq][S]
    for (int s = 0; s < S; ++s) {
        const float* y0 = (s < ns && s_fin[s] == kStatusContinue) ? A.Y + (size_t)(b0 + s) * N : nullptr;
        for (int i = tid; i < ldq; i += NT) {
            ya[(size_t)i * S + s] = (y0 && i < N) ? y0[i] : 0.0f;
            yb[(size_t)i * S + s] = 0.0f;
        }
    }
    __syncthreads();
    const SharedSolveCtl ctl = {s_h, s_fin, s_bad, s_new, s_Jp, s_Jd, s_jp, s_jd};
    float* cur;
    left = shared_converge_loop<S, true, PQP_SOLVE_SHARED_TOL>(A, b0, ns, lds, ctl, A.Md + b0, A.Mp + b0, cur, A.abs_tol,
                                                               A.rel_tol);
    if (left == 0) return;
    // the states still running: their iterate and resume words for the next launch
    for (int s = 0; s < ns; ++s) {
        if (s_fin[s] != kStatusContinue) continue;
        for (int i = tid; i < N; i += NT) A.Y[(size_t)(b0 + s) * N + i] = cur[(size_t)i * S + s];
    }
    if (tid < ns && s_fin[tid] == kStatusContinue) {
        SharedSolveState z;
        z.h = s_h[tid], z.status = kStatusContinue, z.pad = 0, z.Jp = s_Jp[tid], z.Jd = s_Jd[tid];
        A.st[b0 + tid] = z;
    }
    if (tid == 0 && A.pending) atomicAdd(A.pending, 1);
}
