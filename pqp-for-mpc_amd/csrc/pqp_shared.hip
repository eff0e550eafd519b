// pqp_shared.hip -- the batched update for B states of ONE dual problem.
//
// In the MPC workload every problem of a batch is the same plant at another
// state: Qd and Theta are shared, only Fd and Y differ.  pqp_batch_iterate
// wants a Qd per problem and streams all of them from HBM on every update.
// k_batch_shared takes the one Qd and reads each of its elements once per
// S states instead of once per state: Qd y for S states is a matrix-matrix
// product, bound by VALU issue and not by HBM (Qd stays in L2 / Infinity Cache:
// every workgroup re-reads the same 4 N ldq bytes).
//
// Arithmetic (the contract; pqp.h 2b'): per state s and row i
//   den = sum over k = 0..N-1, in that order and from +0.0f, of (max_ref(0, q_ik) + t_ik) * y_s[k]
//   num = the same with max_ref(0, -q_ik);   t_ik = theta_i when k == i, else +0.0f
// each product rounded before it is added, then update_rows4's epilogue.  This
// is the literal form k_batch_iterate uses inside its diagonal window, to which
// its lean form elsewhere is bit-identical (DESIGN.md "Lean form"); here the
// literal form is the cheap one, because the two split values depend on (i, k)
// only: they are computed once per Qd element and serve all S states.
//
// One workgroup owns S consecutive states and all N rows; one lane owns two
// neighbouring rows (one global_load_dwordx2 per k, coalesced over the wave).
// The S iterates live in LDS as [k][S], so y.[k] is a wave-uniform broadcast
// read and two neighbouring states are the halves of one packed multiply and
// one packed add (v_pk_mul_f32 / v_pk_add_f32: never an FMA).  The iterates
// ping-pong between two LDS images, 2 * S * ldq * 4 bytes in all.  A ragged
// last block computes on +0 iterates for the missing states and writes nothing
// for them.  Rows past one pass of 2 * blockDim rows take further passes, as in
// k_batch_iterate.
#include "pqp_device.h"
#include "pqp_shared.h"

#pragma clang fp contract(off)

namespace pqp {

namespace {

typedef float sh2 __attribute__((ext_vector_type(2)));
typedef float sh4 __attribute__((ext_vector_type(4)));

constexpr size_t kSharedLdsBudget = 160 * 1024;
constexpr int kSharedThreads = 512;  // 2 rows per lane: 1024 rows per pass
// Qd loads per lane in flight.  Measured at N = 1024, B = 4096, 10 updates per launch: 16 deep 3.60 ms
// (3.59-3.62), 8 deep 3.65 (3.64-3.66); loading the next block ahead of the current one's arithmetic
// (8 + 8 or 16 + 16) spills and measured 81 and 186 ms.
constexpr int kSharedUnroll = 16;

// den / num of one lane: 2 rows x S states, states paired
template <int S>
struct AccS {
    sh2 p[2][S / 2];
    sh2 n[2][S / 2];
};

// one k: this lane's two Qd entries against the S iterates y[0..S)
template <int S, bool DIAG>
__device__ __forceinline__ void shared_step(AccS<S>& a, float2 q, const float* __restrict__ y, int k, int row,
                                            float th0, float th1) {
    const float t0 = (DIAG && k == row) ? th0 : 0.0f;
    const float t1 = (DIAG && k == row + 1) ? th1 : 0.0f;
    const float qp0 = max_ref(0.0f, q.x) + t0, qn0 = max_ref(0.0f, -q.x) + t0;  // :524-537
    const float qp1 = max_ref(0.0f, q.y) + t1, qn1 = max_ref(0.0f, -q.y) + t1;
    const sh2 vp0 = {qp0, qp0}, vn0 = {qn0, qn0}, vp1 = {qp1, qp1}, vn1 = {qn1, qn1};
#pragma unroll
    for (int j = 0; j < S / 4; ++j) {
        const sh4 yv = *reinterpret_cast<const sh4*>(y + 4 * j);
        const sh2 ya = {yv.x, yv.y}, yb = {yv.z, yv.w};
        a.p[0][2 * j] += vp0 * ya;      a.n[0][2 * j] += vn0 * ya;      // :608-609
        a.p[0][2 * j + 1] += vp0 * yb;  a.n[0][2 * j + 1] += vn0 * yb;
        a.p[1][2 * j] += vp1 * ya;      a.n[1][2 * j] += vn1 * ya;
        a.p[1][2 * j + 1] += vp1 * yb;  a.n[1][2 * j + 1] += vn1 * yb;
    }
}

// k in [ka, kb): `col` points at QdT + row, y at the [k][S] image
template <int S, int U, bool DIAG>
__device__ __forceinline__ void shared_segment(AccS<S>& a, const float* __restrict__ col, int ldq, int ka, int kb,
                                               const float* __restrict__ y, int row, float th0, float th1) {
    int k = ka;
    const float* src = col + (size_t)k * ldq;
    for (; k + U <= kb; k += U) {
        float2 q[U];
#pragma unroll
        for (int j = 0; j < U; ++j) q[j] = *reinterpret_cast<const float2*>(src + (size_t)j * ldq);
        src += (size_t)U * ldq;
#pragma unroll
        for (int j = 0; j < U; ++j) shared_step<S, DIAG>(a, q[j], y + (size_t)(k + j) * S, k + j, row, th0, th1);
    }
    for (; k < kb; ++k) {
        shared_step<S, DIAG>(a, *reinterpret_cast<const float2*>(src), y + (size_t)k * S, k, row, th0, th1);
        src += ldq;
    }
}

}  // namespace

// grid = ceil(B / S) workgroups of blockDim.x (a multiple of 64) threads;
// dynamic LDS = 2 * S * ldq floats.  Y0 may be NULL (1000) or alias Y: a
// workgroup reads its own states' Y0 before the loop and writes Y after it.
template <int S, int U>
__global__ void __launch_bounds__(kSharedThreads) k_batch_shared(const float* __restrict__ QdT, int ldq, int N,
                                                                 const float* __restrict__ theta,
                                                                 const float* __restrict__ Fd, int ldv,
                                                                 const float* Y0, float* Y, int B, int updates) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* ya = lds;
    float* yb = lds + (size_t)S * ldq;
    const int tid = threadIdx.x, NT = blockDim.x;
    const int b0 = blockIdx.x * S;
    const int ns = (B - b0) < S ? (B - b0) : S;  // states of this block
    for (int s = 0; s < S; ++s) {
        const float* y0 = (Y0 && s < ns) ? Y0 + (size_t)(b0 + s) * ldv : nullptr;
        for (int i = tid; i < N; i += NT) {
            ya[(size_t)i * S + s] = (s < ns) ? (y0 ? y0[i] : 1000.0f) : 0.0f;  // initMat(Y,1000) :710
            yb[(size_t)i * S + s] = 0.0f;
        }
    }
    __syncthreads();
    const int wave = tid >> 6;
    for (int u = 0; u < updates; ++u) {
        const float* cur = (u & 1) ? yb : ya;
        float* nxt = (u & 1) ? ya : yb;
        for (int r0 = 0; r0 < N; r0 += 2 * NT) {
            const int row = r0 + 2 * tid;
            if (row >= N) continue;
            // the diagonal of this wave's 128 rows lies in k in [w0, w0 + 128)
            const int w0 = r0 + 128 * wave;
            const int wb = (w0 + 128) < N ? (w0 + 128) : N;
            const float th0 = theta[row], th1 = (row + 1 < N) ? theta[row + 1] : 0.0f;
            AccS<S> a;
#pragma unroll
            for (int r = 0; r < 2; ++r)
#pragma unroll
                for (int j = 0; j < S / 2; ++j) a.p[r][j] = a.n[r][j] = sh2{0.0f, 0.0f};
            const float* col = QdT + row;
            shared_segment<S, U, false>(a, col, ldq, 0, w0, cur, row, th0, th1);
            shared_segment<S, U, true>(a, col, ldq, w0, wb, cur, row, th0, th1);
            shared_segment<S, U, false>(a, col, ldq, wb, N, cur, row, th0, th1);
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                const int i = row + r;
                if (i >= N) continue;
#pragma unroll
                for (int s = 0; s < S; ++s) {
                    if (s >= ns) continue;
                    const float f = Fd[(size_t)(b0 + s) * ldv + i];
                    const float num = a.n[r][s >> 1][s & 1] + 1.0f * max_ref(0.0f, -f);  // matrixAdd(num, Fdn, 1) :611
                    const float den = a.p[r][s >> 1][s & 1] + 1.0f * max_ref(0.0f, f);   // matrixAdd(den, Fdp, 1) :612
                    nxt[(size_t)i * S + s] = num / den * cur[(size_t)i * S + s];         // updY :594
                }
            }
        }
        __syncthreads();
    }
    const float* fin = (updates & 1) ? yb : ya;
    for (int s = 0; s < ns; ++s)
        for (int i = tid; i < N; i += NT) Y[(size_t)(b0 + s) * ldv + i] = fin[(size_t)i * S + s];
}

// States per workgroup by the LDS the two [k][S] images need; 0: unsupported.
int batch_shared_states(int N, int ldq) {
    if (N <= 0 || ldq < N || (ldq & 3)) return 0;
    const size_t col = (size_t)2 * ldq * sizeof(float);
    if (16 * col <= kSharedLdsBudget) return 16;
    if (8 * col <= kSharedLdsBudget) return 8;
    return 0;
}

hipError_t launch_batch_shared(int B, const float* QdT, int ldq, int N, const float* theta, const float* Fd, int ldv,
                               const float* Y0, float* Y, int updates, hipStream_t s) {
    const int S = batch_shared_states(N, ldq);
    if (S == 0) return hipErrorInvalidValue;
    const size_t lds = (size_t)2 * S * ldq * sizeof(float);
    const int pairs = (N + 1) / 2;
    const int nt = pairs >= kSharedThreads ? kSharedThreads : (pairs + 63) / 64 * 64;
    const dim3 grid((unsigned)((B + S - 1) / S));
    constexpr int kPerLaunch = 256;  // as launch_batch_iterate: no single launch runs unbounded
    int done = 0;
    do {
        const int c = (updates - done) < kPerLaunch ? (updates - done) : kPerLaunch;
        const float* y0 = done ? Y : Y0;
        if (S == 16)
            hipLaunchKernelGGL((k_batch_shared<16, kSharedUnroll>), grid, dim3(nt), lds, s, QdT, ldq, N, theta, Fd, ldv,
                               y0, Y, B, c);
        else
            hipLaunchKernelGGL((k_batch_shared<8, kSharedUnroll>), grid, dim3(nt), lds, s, QdT, ldq, N, theta, Fd, ldv,
                               y0, Y, B, c);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        done += c;
    } while (done < updates);
    return hipSuccess;
}

}  // namespace pqp
