// pqp_shared_solve.hip -- solveQuadraticDual in converge mode for B states of
// ONE plant (include/pqp.h 2h).  Qp_inv, Gp, Kp -- and so Qd, Qp, Theta and
// Gp Qp_inv -- are shared by the batch; Fd, Md, Fp, Mp (perhaps Kp) and the
// iterate differ per state.  k_batch_shared (pqp_shared.hip) took the update
// of that workload from a matrix-vector to a matrix-matrix product; here
// terminate() follows it, so that the whole loop of PQP_CPU.c:694-750 reads
// every shared matrix once per S states and keeps no per-state matrix at all.
//
// Arithmetic (the contract): k_solve_single's (pqp_kernels.hip), that is the
// reference's, per state.  Every sum starts from +0.0f, runs in index order and
// rounds each product before it is added.
//   update       k_batch_shared's literal form:  den_i = sum_k (max_ref(0, q_ik) + t_ik) y_k,
//                num_i with max_ref(0, -q_ik); t_ik = theta_i at k == i, else +0.0f; then
//                y'_i = (num_i + 1.0f max_ref(0, -Fd_i)) / (den_i + 1.0f max_ref(0, Fd_i)) * y_i
//   terminate()  t_j = (sum_i Gp[i][j] y_i) + 1.0f Fp_j;   U_i = -sum_j Qp_inv[i][j] t_j;
//                infeasible iff some row has sum_j Gp[i][j] U_j > Kp_i + max_ref((float)(1e-6 Kp_i), (float)1e-6);
//                else Jd from tq_j = sum_i y_i Qd[i][j], quad = sum_j tq_j y_j, lin = sum_j Fd_j y_j,
//                J = (float)(0.0 + 0.5 (double)quad); J += lin; J += Md / 2; Jp the same with U, Qp, Fp, Mp;
//                then gap_stop(Jp, Jd) and, where it says continue, the caller's tolerances (tol_stop, pqp.h 2k).
//
// One workgroup owns S consecutive states.  Every per-state vector lives in
// LDS as [index][S]: a product against a shared matrix reads its S operands of
// one k with a wave-uniform broadcast, and two neighbouring states are the two
// halves of one packed multiply and one packed add (v_pk_mul_f32 /
// v_pk_add_f32: never an FMA).  A lane owns two neighbouring output rows (one
// coalesced 8-byte load per k, 16 in flight) -- one row where the product has no
// more rows than the workgroup has lanes, so that more waves stay busy.
//
// The states of a workgroup stop at different iterates.  A state that stops
// (or reaches the cap) has its Y, U, h, status and costs written out at that
// moment; its LDS columns go on being computed and are ignored (packed halves
// are independent: its partner sees nothing of it).  The workgroup leaves when
// all its states have finished or its chunk of iterates is used, and then writes
// the iterate and the resume words of the states still running; the next launch
// continues from them.  A ragged last block computes on +0 iterates for the
// missing states and writes nothing for them.
//
// Y'Qd: with a bit-symmetric Qd the update's pass also forms tq (a third
// sum per row and state over the same loads) -- the update to Y_{h+1} is then
// computed before terminate(Y_h) and dropped for the states that stop at h.  That
// form is taken only when some state of the workgroup was feasible at the previous
// iterate; otherwise, and for a Qd that is not symmetric, tq is a pass of its own
// over the row-major Qd, made only when some state passed checkFeas.
#include "pqp_device.h"
#include "pqp_shared_solve.h"

#pragma clang fp contract(off)

namespace pqp {

namespace {

typedef float ss2 __attribute__((ext_vector_type(2)));
typedef float ss4 __attribute__((ext_vector_type(4)));

constexpr int kSolveSharedThreads = 512;  // 2 rows per lane: 1024 rows per pass
constexpr int kSolveSharedUnroll = 16;    // matrix loads per lane in flight (k_batch_shared's measured choice)

// the S operands of one k (a row of a [k][S] image) as S / 2 pairs of neighbouring states
template <int S>
__device__ __forceinline__ void states_at(const float* __restrict__ x, ss2 (&v)[S / 2]) {
    if constexpr (S == 2) {
        v[0] = *reinterpret_cast<const ss2*>(x);
    } else {
#pragma unroll
        for (int j = 0; j < S / 4; ++j) {
            const ss4 t = *reinterpret_cast<const ss4*>(x + 4 * j);
            v[2 * j] = ss2{t.x, t.y};
            v[2 * j + 1] = ss2{t.z, t.w};
        }
    }
}

// a[r][.] = sum over k = 0..nk-1, in order and from +0.0f, of col[k * lda + r] * x[k][.] for this lane's R rows
template <int S, int R>
__device__ __forceinline__ void pk_dot(ss2 (&a)[R][S / 2], const float* __restrict__ col, int lda, int nk,
                                       const float* __restrict__ x) {
    constexpr int U = kSolveSharedUnroll;
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int p = 0; p < S / 2; ++p) a[r][p] = ss2{0.0f, 0.0f};
    int k = 0;
    const float* src = col;
    for (; k + U <= nk; k += U) {
        float q[U][R];
#pragma unroll
        for (int j = 0; j < U; ++j) {
            if constexpr (R == 2) {
                const float2 t = *reinterpret_cast<const float2*>(src + (size_t)j * lda);
                q[j][0] = t.x;
                q[j][1] = t.y;
            } else {
                q[j][0] = src[(size_t)j * lda];
            }
        }
        src += (size_t)U * lda;
#pragma unroll
        for (int j = 0; j < U; ++j) {
            ss2 xv[S / 2];
            states_at<S>(x + (size_t)(k + j) * S, xv);
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const ss2 qv = {q[j][r], q[j][r]};
#pragma unroll
                for (int p = 0; p < S / 2; ++p) a[r][p] += qv * xv[p];
            }
        }
    }
    for (; k < nk; ++k) {
        ss2 xv[S / 2];
        states_at<S>(x + (size_t)k * S, xv);
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const float qs = src[r];
            const ss2 qv = {qs, qs};
#pragma unroll
            for (int p = 0; p < S / 2; ++p) a[r][p] += qv * xv[p];
        }
        src += lda;
    }
}

// epi(i, s, sum_k A[k * lda + i] * x[k][s]) for every row i < n_out and state s < S; R rows per lane
template <int S, int R, class Epi>
__device__ __forceinline__ void shared_rows(const float* __restrict__ A, int lda, int n_out, int nk,
                                            const float* __restrict__ x, Epi epi) {
    for (int row = R * (int)threadIdx.x; row < n_out; row += R * (int)blockDim.x) {
        ss2 a[R][S / 2];
        pk_dot<S, R>(a, A + row, lda, nk, x);
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int i = row + r;
            if (i >= n_out) continue;
#pragma unroll
            for (int s = 0; s < S; ++s) epi(i, s, a[r][s >> 1][s & 1]);
        }
    }
}
// (every matrix is padded to lda % 4 == 0 and zero-filled there, so the second row of a pair is always readable)
template <int S, class Epi>
__device__ __forceinline__ void shared_product(const float* __restrict__ A, int lda, int n_out, int nk,
                                               const float* __restrict__ x, Epi epi) {
    if (n_out <= (int)blockDim.x) shared_rows<S, 1>(A, lda, n_out, nk, x, epi);
    else shared_rows<S, 2>(A, lda, n_out, nk, x, epi);
}

// den / num (and, FUSE, the Y'Qd sum) of one lane: 2 rows x S states, states paired
template <int S, bool FUSE>
struct UpdAcc {
    ss2 p[2][S / 2];
    ss2 n[2][S / 2];
    ss2 q[2][FUSE ? S / 2 : 1];
};

// one k of the update: this lane's two Qd entries against the S iterates y[0..S)
template <int S, bool FUSE, bool DIAG>
__device__ __forceinline__ void upd_step(UpdAcc<S, FUSE>& a, float2 q, const float* __restrict__ y, int k, int row,
                                         float th0, float th1) {
    const float t0 = (DIAG && k == row) ? th0 : 0.0f;
    const float t1 = (DIAG && k == row + 1) ? th1 : 0.0f;
    const float qp0 = max_ref(0.0f, q.x) + t0, qn0 = max_ref(0.0f, -q.x) + t0;  // :524-537
    const float qp1 = max_ref(0.0f, q.y) + t1, qn1 = max_ref(0.0f, -q.y) + t1;
    const ss2 vp0 = {qp0, qp0}, vn0 = {qn0, qn0}, vp1 = {qp1, qp1}, vn1 = {qn1, qn1};
    const ss2 vq0 = {q.x, q.x}, vq1 = {q.y, q.y};
    ss2 yv[S / 2];
    states_at<S>(y, yv);
#pragma unroll
    for (int p = 0; p < S / 2; ++p) {
        a.p[0][p] += vp0 * yv[p];  // :608-609
        a.n[0][p] += vn0 * yv[p];
        a.p[1][p] += vp1 * yv[p];
        a.n[1][p] += vn1 * yv[p];
        if constexpr (FUSE) {  // Y'Qd :110, k in order (Qd bit-symmetric: this column is also Qd's)
            a.q[0][p] += yv[p] * vq0;
            a.q[1][p] += yv[p] * vq1;
        }
    }
}

template <int S, bool FUSE, bool DIAG>
__device__ __forceinline__ void upd_segment(UpdAcc<S, FUSE>& a, const float* __restrict__ col, int ldq, int ka, int kb,
                                            const float* __restrict__ y, int row, float th0, float th1) {
    constexpr int U = kSolveSharedUnroll;
    int k = ka;
    const float* src = col + (size_t)k * ldq;
    for (; k + U <= kb; k += U) {
        float2 q[U];
#pragma unroll
        for (int j = 0; j < U; ++j) q[j] = *reinterpret_cast<const float2*>(src + (size_t)j * ldq);
        src += (size_t)U * ldq;
#pragma unroll
        for (int j = 0; j < U; ++j) upd_step<S, FUSE, DIAG>(a, q[j], y + (size_t)(k + j) * S, k + j, row, th0, th1);
    }
    for (; k < kb; ++k) {
        upd_step<S, FUSE, DIAG>(a, *reinterpret_cast<const float2*>(src), y + (size_t)k * S, k, row, th0, th1);
        src += ldq;
    }
}

// updateY2 (PQP_CPU.c:603-618) of the workgroup's S states from `cur` into `nxt`; FUSE: tq = Y'Qd of `cur` too
template <int S, bool FUSE>
__device__ __forceinline__ void shared_update(const SharedSolveCore& A, int b0, int ns, const float* __restrict__ cur,
                                              float* __restrict__ nxt, float* __restrict__ tq) {
    const int N = A.N, ldq = A.ldq;
    const int tid = threadIdx.x, NT = blockDim.x, wave = tid >> 6;
    for (int r0 = 0; r0 < N; r0 += 2 * NT) {
        const int row = r0 + 2 * tid;
        if (row >= N) continue;
        // the diagonal of this wave's 128 rows lies in k in [w0, w0 + 128)
        const int w0 = r0 + 128 * wave;
        const int wb = (w0 + 128) < N ? (w0 + 128) : N;
        const float th0 = A.theta[row], th1 = (row + 1 < N) ? A.theta[row + 1] : 0.0f;
        UpdAcc<S, FUSE> a;
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int p = 0; p < S / 2; ++p) {
                a.p[r][p] = a.n[r][p] = ss2{0.0f, 0.0f};
                if constexpr (FUSE) a.q[r][p] = ss2{0.0f, 0.0f};
            }
        const float* col = A.QdT + row;
        upd_segment<S, FUSE, false>(a, col, ldq, 0, w0, cur, row, th0, th1);
        upd_segment<S, FUSE, true>(a, col, ldq, w0, wb, cur, row, th0, th1);
        upd_segment<S, FUSE, false>(a, col, ldq, wb, N, cur, row, th0, th1);
        if constexpr (FUSE) {  // first, so that its sums' registers are free during the divisions
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                if (row + r >= N) continue;
#pragma unroll
                for (int s = 0; s < S; ++s) tq[(size_t)(row + r) * S + s] = a.q[r][s >> 1][s & 1];
            }
        }
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const int i = row + r;
            if (i >= N) continue;
#pragma unroll
            for (int s = 0; s < S; ++s) {
                const float f = (s < ns) ? A.Fd[(size_t)(b0 + s) * N + i] : 0.0f;
                const float num = a.n[r][s >> 1][s & 1] + 1.0f * max_ref(0.0f, -f);  // matrixAdd(num, Fdn, 1) :611
                const float den = a.p[r][s >> 1][s & 1] + 1.0f * max_ref(0.0f, f);   // matrixAdd(den, Fdp, 1) :612
                nxt[(size_t)i * S + s] = num / den * cur[(size_t)i * S + s];         // updY :594
            }
        }
    }
}

// sum of q[k][s] and of l[k][s] over k = 0..n-1 in order (the two chains interleaved), then computeCost's tail :658-665
__device__ __forceinline__ float cost_chain(const float* __restrict__ q, const float* __restrict__ l, int n, int S,
                                            int s, float mc) {
    float quad = 0.0f, lin = 0.0f;
    int k = 0;
    for (; k + 8 <= n; k += 8) {
        float a[8], b[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            a[j] = q[(size_t)(k + j) * S + s];
            b[j] = l[(size_t)(k + j) * S + s];
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            quad += a[j];
            lin += b[j];
        }
    }
    for (; k < n; ++k) {
        quad += q[(size_t)k * S + s];
        lin += l[(size_t)k * S + s];
    }
    float J = 0.0f;
    J = (float)((double)J + 0.5 * (double)quad);
    J += lin;
    J += mc / 2;
    return J;
}

// The per-state control words of a workgroup (static LDS of the kernel that runs the loop):
// h, the status (SolveStatus), this iterate's checkFeas failure, "finished at this iterate",
// the costs of the last terminate() that passed checkFeas, and this iterate's two costs.
struct SharedSolveCtl {
    long long* h;
    int *fin, *bad, *fresh;
    float *Jp, *Jd, *jp, *jd;
};

// The loop of PQP_CPU.c:718-746 -- terminate(), then updateY2 -- for the S states of one workgroup
// (k_solve_shared and k_step_shared: the same text, so the same arithmetic).  In: the control words
// of c, the iterates as the first image of lds ([ldq][S]; the second zero) and a barrier after both;
// md / mp: Md and Mp of state s at [s].  A state that finishes has its Y, U, h, status and costs
// written at that moment (RESUME: its resume words too).  Leaves when no state is running or
// A.chunk updates were made; returns the states still running, `cur` the image of their iterate.
// TOL: the caller's gap tolerances abs_tol, rel_tol (pqp.h 2k) are tried where gap_stop says continue; else
// they are not read.
template <int S, bool RESUME, bool TOL>
__device__ __forceinline__ int shared_converge_loop(const SharedSolveCore& A, int b0, int ns, float* lds,
                                                    const SharedSolveCtl& c, const float* md, const float* mp,
                                                    float*& cur, float abs_tol, float rel_tol) {
    const int tid = threadIdx.x, NT = blockDim.x;
    const int N = A.N, M = A.M, ldq = A.ldq, ldm = A.ldm;
    long long* const s_h = c.h;
    int* const s_fin = c.fin;
    int* const s_bad = c.bad;
    int* const s_new = c.fresh;
    float* const s_Jp = c.Jp;
    float* const s_Jd = c.Jd;
    float* const s_jp = c.jp;
    float* const s_jd = c.jd;
    float* ya = lds;                       // [ldq][S]
    float* yb = ya + (size_t)S * ldq;      // [ldq][S]
    float* tq = yb + (size_t)S * ldq;      // [ldq][S]  Y'Qd row, then its terms (Jd)
    float* fy = tq + (size_t)S * ldq;      // [ldq][S]  Fd.Y terms
    float* tM = fy + (size_t)S * ldq;      // [ldm][S]  Gp'Y + Fp, then the Fp.U terms
    float* Us = tM + (size_t)S * ldm;      // [ldm][S]  U
    float* tu = Us + (size_t)S * ldm;      // [ldm][S]  U'Qp row, then its terms (Jp)
    int left = 0;
    cur = ya;
    float* nxt = yb;
    bool was_feasible = false;
    long long done_here = 0;
    const int cb = NT >= 128 ? 64 : S;  // first lane of the primal cost chains (another wave where there is one)
    for (;;) {
        const bool fuse = A.sym && was_feasible;
        if (fuse) {
            shared_update<S, true>(A, b0, ns, cur, nxt, tq);
            __syncthreads();
        }
        // ---- terminate(Y)  PQP_CPU.c:673-687 ----
        // computeUfromY :352-360
        shared_product<S>(A.GpP, ldm, M, N, cur, [&](int j, int s, float v) {
            tM[(size_t)j * S + s] = v + 1.0f * ((s < ns) ? A.Fp[(size_t)(b0 + s) * M + j] : 0.0f);
        });
        __syncthreads();
        shared_product<S>(A.QinvT, ldm, M, M, tM, [&](int i, int s, float v) { Us[(size_t)i * S + s] = -v; });
        __syncthreads();
        // checkFeas :632-641
        {
            unsigned bad = 0;
            shared_product<S>(A.GpT, ldq, N, M, Us, [&](int i, int s, float v) {
                const float kp = A.KpB ? ((s < ns) ? A.KpB[(size_t)(b0 + s) * N + i] : 0.0f) : A.Kp[i];
                if (v > kp + max_ref((float)(kTol * kp), (float)kTol)) bad |= 1u << s;
            });
            if (bad)
                for (int s = 0; s < S; ++s)
                    if (bad >> s & 1) atomicOr(&s_bad[s], 1);
        }
        __syncthreads();
        // a state that is running and has no row over its bound goes on to the costs
        const bool any_feasible = __syncthreads_or(tid < S && s_fin[tid] == kStatusContinue && !s_bad[tid]) != 0;
        if (any_feasible) {
            // computeCost(Y, Qd, Fd, Md) and computeCost(U, Qp, Fp, Mp) :648-666
            if (!fuse)
                shared_product<S>(A.QdR, ldq, N, N, cur, [&](int j, int s, float v) { tq[(size_t)j * S + s] = v; });
            shared_product<S>(A.QpP, ldm, M, M, Us, [&](int j, int s, float v) { tu[(size_t)j * S + s] = v; });
            __syncthreads();
            // the dot products' terms formed in parallel, then summed in k order by one lane per state and cost
            for (int s = 0; s < ns; ++s) {
                const float* fd = A.Fd + (size_t)(b0 + s) * N;
                const float* fp = A.Fp + (size_t)(b0 + s) * M;
                for (int j = tid; j < N; j += NT) {
                    const size_t e = (size_t)j * S + s;
                    tq[e] = tq[e] * cur[e];
                    fy[e] = fd[j] * cur[e];
                }
                for (int j = tid; j < M; j += NT) {
                    const size_t e = (size_t)j * S + s;
                    tu[e] = tu[e] * Us[e];
                    tM[e] = fp[j] * Us[e];
                }
            }
            __syncthreads();
            if (tid < ns) s_jd[tid] = cost_chain(tq, fy, N, S, tid, md[tid]);
            else if (tid >= cb && tid < cb + ns) s_jp[tid - cb] = cost_chain(tu, tM, M, S, tid - cb, mp[tid - cb]);
            __syncthreads();
        }
        was_feasible = any_feasible;
        // each running state's decision; a state that finishes here is final from now on
        if (tid < S) {
            const int s = tid;
            int fresh = 0;
            if (s_fin[s] == kStatusContinue) {
                bool stop = false;
                int how = kStatusDone;  // TOL: or kStatusTol
                if (!s_bad[s]) {
                    const float Jp = s_jp[s], Jd = s_jd[s];
                    s_Jp[s] = Jp, s_Jd[s] = Jd;
                    stop = gap_stop(Jp, Jd);
                    if constexpr (TOL)
                        if (!stop && tol_stop(Jp, Jd, abs_tol, rel_tol)) stop = true, how = kStatusTol;
                }
                const long long h = s_h[s];
                const int fin = stop ? how
                                     : (A.max_updates > 0 && h - 1 >= A.max_updates) ? kStatusCapped : kStatusContinue;
                if (fin != kStatusContinue) {
                    s_fin[s] = fin;
                    fresh = 1;
                    SharedSolveState z;
                    z.h = h, z.status = fin, z.pad = 0, z.Jp = s_Jp[s], z.Jd = s_Jd[s];
                    if constexpr (RESUME) A.st[b0 + s] = z;
                    if (A.h) A.h[b0 + s] = h;
                    if (A.status) A.status[b0 + s] = fin;
                    if (A.Jp) A.Jp[b0 + s] = z.Jp;
                    if (A.Jd) A.Jd[b0 + s] = z.Jd;
                }
            }
            s_new[s] = fresh;
            s_bad[s] = 0;
        }
        left = __syncthreads_count(tid < S && s_fin[tid] == kStatusContinue);
        for (int s = 0; s < ns; ++s) {
            if (!s_new[s]) continue;
            for (int i = tid; i < N; i += NT) A.Y[(size_t)(b0 + s) * N + i] = cur[(size_t)i * S + s];
            for (int i = tid; i < M; i += NT) A.U[(size_t)(b0 + s) * M + i] = Us[(size_t)i * S + s];
        }
        if (left == 0 || done_here >= A.chunk) break;
        // ---- updateY2  PQP_CPU.c:603-618 ----
        if (!fuse) shared_update<S, false>(A, b0, ns, cur, nxt, nullptr);
        __syncthreads();
        float* t = cur;
        cur = nxt;
        nxt = t;
        if (tid < S && s_fin[tid] == kStatusContinue) ++s_h[tid];
        ++done_here;
    }
    return left;
}

}  // namespace

// k_solve_shared and k_solve_shared_tol: one text (pqp_shared_solve_kernel.inc), compiled with and without the
// caller's gap tolerances (pqp.h 2k)
#define PQP_SOLVE_SHARED_KERNEL k_solve_shared
#define PQP_SOLVE_SHARED_TOL false
#include "pqp_shared_solve_kernel.inc"
#undef PQP_SOLVE_SHARED_KERNEL
#undef PQP_SOLVE_SHARED_TOL
#define PQP_SOLVE_SHARED_KERNEL k_solve_shared_tol
#define PQP_SOLVE_SHARED_TOL true
#include "pqp_shared_solve_kernel.inc"
#undef PQP_SOLVE_SHARED_KERNEL
#undef PQP_SOLVE_SHARED_TOL

// Fd [B][N] and Md [B] of B states (convertToDual's computeFd / computeMd, PQP_CPU.c:456-479; pqp_relin.hip's
// arithmetic) against the shared Gp Qp_inv and Qp_inv: one workgroup per S states, Fp staged as [k][S].
// dynamic LDS = 2 * S * ldm floats.
template <int S>
__global__ void __launch_bounds__(kSolveSharedThreads) k_relin_shared(SharedRelinArgs A) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x, NT = blockDim.x;
    const int N = A.N, M = A.M, ldm = A.ldm;
    const int b0 = blockIdx.x * S;
    const int ns = (A.B - b0) < S ? (A.B - b0) : S;
    float* fpx = lds;                       // [ldm][S]  Fp
    float* tmp = fpx + (size_t)S * ldm;     // [ldm][S]  Fp'Qp_inv, then its terms
    for (int s = 0; s < S; ++s)
        for (int k = tid; k < ldm; k += NT)
            fpx[(size_t)k * S + s] = (s < ns && k < M) ? A.Fp[(size_t)(b0 + s) * M + k] : 0.0f;
    __syncthreads();
    shared_product<S>(A.GQT, A.ldq, N, M, fpx, [&](int i, int s, float v) {
        if (s < ns) {
            const float kp = A.KpB ? A.KpB[(size_t)(b0 + s) * N + i] : A.Kp[i];
            A.Fd[(size_t)(b0 + s) * N + i] = v + 1.0f * kp;  // matrixAdd(Fd, Fd, Kp) :459
        }
    });
    shared_product<S>(A.QinvR, ldm, M, M, fpx, [&](int j, int s, float v) { tmp[(size_t)j * S + s] = v; });
    __syncthreads();
    for (int e = tid; e < M * S; e += NT) tmp[e] = tmp[e] * fpx[e];  // :475-476
    __syncthreads();
    if (tid < ns) {
        float md = 0.0f;
        for (int j = 0; j < M; ++j) md += tmp[(size_t)j * S + tid];
        A.Md[b0 + tid] = md + -1.0f * A.Mp[b0 + tid];  // :478
    }
}

__global__ void __launch_bounds__(256) k_shared_solve_init(int B, int N, SharedSolveState* __restrict__ st,
                                                          const float* Y0, float* Y) {
    const long long n = (long long)B * N, step = (long long)gridDim.x * 256;
    const long long e0 = (long long)blockIdx.x * 256 + threadIdx.x;
    if (Y0 != Y)
        for (long long e = e0; e < n; e += step) Y[e] = Y0 ? Y0[e] : 1000.0f;  // initMat(Y, 1000) :710
    for (long long b = e0; b < B; b += step) {
        SharedSolveState z;
        z.h = 1, z.status = kStatusContinue, z.pad = 0;
        z.Jp = z.Jd = __builtin_nanf("");
        st[b] = z;
    }
}

__global__ void __launch_bounds__(256) k_shared_layout(const float* __restrict__ src, int orows, int ocols,
                                                      int transposed, float* __restrict__ dst, int ld) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long long)orows * ld) return;
    const int r = (int)(e / ld), c = (int)(e - (long long)r * ld);
    dst[e] = c < ocols ? (transposed ? src[(size_t)c * orows + r] : src[(size_t)r * ocols + c]) : 0.0f;
}

// The largest of 8, 4, 2 states whose vectors fit the LDS beside the control words; 0: unsupported.
// (Not 16, which k_batch_shared takes where it fits: the fused update then holds 96 sums per lane beside
// its 32 loaded words, and the compiler spilled some of them to scratch.)
int solve_shared_states(int N, int M) {
    if (N <= 0 || M <= 0 || N > (1 << 20) || M > (1 << 20)) return 0;
    for (int S = 8; S >= 2; S >>= 1)
        if (solve_shared_lds_bytes(N, M, S) + kSolveSharedStaticLds <= kSolveSharedLdsBudget) return S;
    return 0;
}

namespace {
inline int solve_shared_threads(int N, int M) {
    const int pairs = ((N > M ? N : M) + 1) / 2;
    return pairs >= kSolveSharedThreads ? kSolveSharedThreads : (pairs + 63) / 64 * 64;
}
// ONE launch of a shared-plant kernel at S states per workgroup: its instantiation for S = 8, 4 or (any other) 2,
// one workgroup per S of the B states
template <class Args>
hipError_t launch_shared_s(void (*k8)(Args), void (*k4)(Args), void (*k2)(Args), int S, int B, int N, int M,
                           size_t lds, hipStream_t s, const Args& a) {
    hipLaunchKernelGGL(S == 8 ? k8 : S == 4 ? k4 : k2, dim3((unsigned)((B + S - 1) / S)),
                       dim3(solve_shared_threads(N, M)), lds, s, a);
    return hipGetLastError();
}
}  // namespace

hipError_t launch_shared_solve_init(int B, int N, SharedSolveState* st, const float* Y0, float* Y, hipStream_t s) {
    const long long n = (long long)B * N;
    const long long blocks = (n + 255) / 256;
    hipLaunchKernelGGL(k_shared_solve_init, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, s, B, N, st,
                       Y0, Y);
    return hipGetLastError();
}

hipError_t launch_solve_shared(const SharedSolveArgs& a, int S, hipStream_t s) {
    if (S != solve_shared_states(a.N, a.M) || S == 0) return hipErrorInvalidValue;
    const size_t lds = solve_shared_lds_bytes(a.N, a.M, S);
    if (shared_tol(a.abs_tol, a.rel_tol))  // a positive tolerance: the _tol build
        return launch_shared_s(k_solve_shared_tol<8>, k_solve_shared_tol<4>, k_solve_shared_tol<2>, S, a.B, a.N, a.M,
                               lds, s, a);
    return launch_shared_s(k_solve_shared<8>, k_solve_shared<4>, k_solve_shared<2>, S, a.B, a.N, a.M, lds, s, a);
}

hipError_t launch_relin_shared(const SharedRelinArgs& a, int S, hipStream_t s) {
    if (S != solve_shared_states(a.N, a.M) || S == 0) return hipErrorInvalidValue;
    const size_t lds = (size_t)2 * S * a.ldm * sizeof(float);
    return launch_shared_s(k_relin_shared<8>, k_relin_shared<4>, k_relin_shared<2>, S, a.B, a.N, a.M, lds, s, a);
}

hipError_t launch_shared_layout(const float* src, int orows, int ocols, int transposed, float* dst, int ld,
                                hipStream_t s) {
    const long long n = (long long)orows * ld;
    hipLaunchKernelGGL(k_shared_layout, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, src, orows, ocols,
                       transposed, dst, ld);
    return hipGetLastError();
}

}  // namespace pqp
