// pqp_shared_step_kernel.inc -- the text of k_step_shared (pqp_shared_step.hip), which includes it twice:
//   PQP_STEP_SHARED_KERNEL k_step_shared,     PQP_STEP_SHARED_TOL false: the reference's stopping rule alone
//   PQP_STEP_SHARED_KERNEL k_step_shared_tol, PQP_STEP_SHARED_TOL true:  then the caller's gap tolerances (pqp.h 2k)
// Two kernels of one text, as pqp_plant_step.inc: with the flag compiled out, k_step_shared's three builds
// keep the instructions they had before the tolerances existed (DESIGN.md 4k).
//
// grid = ceil(B / S) workgroups of blockDim.x (a multiple of 64) threads;
// dynamic LDS = S * step_shared_state_floats(N, M, nd, ns) floats.
template <int S>
__global__ void __launch_bounds__(kSolveSharedThreads) PQP_STEP_SHARED_KERNEL(SharedStepArgs T) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    __shared__ long long s_h[S];
    __shared__ int s_fin[S], s_bad[S], s_new[S];
    __shared__ float s_Jp[S], s_Jd[S], s_jp[S], s_jd[S];
    __shared__ float s_Mp[S], s_Md[S], s_dot[5 * S];
    const SharedSolveCore& A = T.solve;
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
    shared_converge_loop<S, false, PQP_STEP_SHARED_TOL>(A, b0, nst, lds, ctl, s_Md, s_Mp, cur, T.abs_tol, T.rel_tol);
}
