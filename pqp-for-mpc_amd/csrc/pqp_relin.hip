// pqp_relin.hip -- relinearization of resident problems: new Fd and Md from
// new linear terms Fp, Mp, Kp with everything that depends on Gp and Qp_inv
// alone kept (convertToDual's computeFd / computeMd, PQP_CPU.c:456-479, with
// the temporary Gp Qp_inv of :491-492 computed once).
//
//   Fd[i] = (sum_k GQ[i][k] Fp[k]) + Kp[i]        k = 0..M-1 in order from +0.0f
//   Md    = (sum_j (sum_k Fp[k] Qp_inv[k][j]) Fp[j]) - Mp
//
// with every product rounded before its add (no FMA), as matrixMultiply
// (:88-146) and k_matmul_seq do: the results equal pqp_batch_convert_to_dual's
// bit for bit.
//
// GQ = Gp Qp_inv is kept in a layout of its own (k_relin_pack), B*N*M floats
// for the whole batch.  Rows are numbered r = b * N + i across the batch and
// taken in groups of 64, one wave's: group g holds its rows' packets
// {GQ[r][4kb .. 4kb+3]} kb-major, packet (r, kb) at float4 index
// g * 64 * (M/4) + kb * w + (r & 63), w = 64 (the last group: the rows it
// has).  Behind the packets, for M % 4 != 0, the last M % 4 columns as
// scalars, column 4 (M/4) + t of row r at t * B * N + r.  One lane owns one
// row: the 64 lanes of a wave read 64 consecutive 16-byte packets (1 KiB per
// load instruction), a lane's next k comes from the next KiB, and a wave
// streams one contiguous 16 M-byte region from its start to its end (16 loads
// in flight per lane), every wave another one.  With N = 28 a wave holds 2.3
// problems and no lane but the last workgroup's tail idles.
//
// k_relinearize is ONE launch: its first workgroups compute Md (one lane per
// problem for M <= 16, one workgroup per problem above: lane j sums column j
// of Qp_inv in k order, coalesced over j, thread 0 then the M terms in j
// order), the rest Fd.  A problem's Md reads its whole Qp_inv (4 M^2 bytes)
// through one CU, so at M = 512 it, not the walk of GQ, ends the launch
// (16-byte loads and 32 of them in flight per lane measured no
// faster: the CU's share of the memory system bounds it, not latency).
#include <algorithm>

#include "pqp_device.h"
#include "pqp_relin.h"

#pragma clang fp contract(off)

namespace pqp {

namespace {

typedef float rf4 __attribute__((ext_vector_type(4)));

constexpr int kRelinThreads = 256;
constexpr int kRelinMdLaneMaxM = 16;     // Md: one lane per problem up to this M (M^2 dependent steps)
constexpr int kRelinLdsFloats = 12288;   // Fp staged in LDS when it fits this many floats

inline unsigned cdivr(long long a, long long b) { return (unsigned)((a + b - 1) / b); }
__host__ __device__ inline int relin_round4(int n) { return (n + 3) & ~3; }

// Row-major GQ [B][N][M] -> the packed layout above; one thread per
// destination float (coalesced stores; the 16-byte source segments of a wave
// come from 16 rows).
__global__ void __launch_bounds__(256) k_relin_pack(int B, int N, int M, const float* __restrict__ src,
                                                    float* __restrict__ dst) {
    const long long d = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long total = (long long)B * N * M;
    if (d >= total) return;
    const int kbf = M >> 2;
    const long long rows = (long long)B * N, p4 = rows * kbf * 4;
    long long r;
    int k;
    if (d < p4) {
        const long long q = d >> 2, g = q / (64LL * kbf), rem = q - g * 64 * kbf;
        const long long w = rows - 64 * g < 64 ? rows - 64 * g : 64;
        const int kb = (int)(rem / w);
        r = 64 * g + (rem - kb * w);
        k = 4 * kb + (int)(d & 3);
    } else {
        const long long t = (d - p4) / rows;
        r = (d - p4) - t * rows;
        k = 4 * kbf + (int)t;
    }
    dst[d] = src[r * M + k];  // row r = b * N + i of the stacked row-major GQ
}

// Md of problem b by one lane (small M): tmp_j = sum_k Fp[k] Qp_inv[k][j] for
// each j in turn, then the running sum of tmp_j Fp[j] (:475-476), then - Mp
// (:478).
__device__ __forceinline__ float md_one_lane(const float* __restrict__ Qinv, const float* __restrict__ Fp,
                                             float mp, int M) {
    float md = 0.0f;
    for (int j = 0; j < M; ++j) {
        float t = 0.0f;
#pragma unroll 8
        for (int k = 0; k < M; ++k) t += Fp[k] * Qinv[(size_t)k * M + j];
        md += t * Fp[j];
    }
    return md + -1.0f * mp;
}

// LDS: Fp of the block's problems staged in shared memory (rows of round4(M)
// floats, 16-byte reads broadcast to the lanes of one problem); otherwise
// read from global memory.
template <bool LDS>
__global__ void __launch_bounds__(kRelinThreads)
k_relinearize(int B, int N, int M, const float* __restrict__ GQ, const float* __restrict__ Qinv,
              const float* __restrict__ Kp, const float* __restrict__ Fp, const float* __restrict__ Mp,
              float* __restrict__ Fd, float* __restrict__ Md, int md_blocks) {
    extern __shared__ __attribute__((aligned(16))) float fps[];
    __shared__ float tmpc[kRelinThreads];
    const int tid = threadIdx.x;
    const int Mr = relin_round4(M);

    if ((int)blockIdx.x < md_blocks) {  // ---- Md
        if (M <= kRelinMdLaneMaxM) {
            const long long b = (long long)blockIdx.x * kRelinThreads + tid;
            if (b < B) Md[b] = md_one_lane(Qinv + (size_t)b * M * M, Fp + (size_t)b * M, Mp[b], M);
            return;
        }
        const size_t b = blockIdx.x;
        const float* q = Qinv + b * M * M;
        const float* fg = Fp + b * M;
        if (LDS) {
            for (int k = tid; k < M; k += kRelinThreads) fps[k] = fg[k];
            __syncthreads();
        }
        const float* f = LDS ? fps : fg;
        float md = 0.0f;  // thread 0's running sum over j
        for (int j0 = 0; j0 < M; j0 += kRelinThreads) {
            const int j = j0 + tid;
            float t = 0.0f;
            if (j < M) {
#pragma unroll 8
                for (int k = 0; k < M; ++k) t += f[k] * q[(size_t)k * M + j];  // coalesced over j
            }
            tmpc[tid] = t;
            __syncthreads();
            if (tid == 0) {
                const int n = M - j0 < kRelinThreads ? M - j0 : kRelinThreads;
                for (int e = 0; e < n; ++e) md += tmpc[e] * f[j0 + e];
            }
            __syncthreads();
        }
        if (tid == 0) Md[b] = md + -1.0f * Mp[b];
        return;
    }

    // ---- Fd: row r = b * N + i of the batch
    const long long rows = (long long)B * N;
    const long long r0 = (long long)((int)blockIdx.x - md_blocks) * kRelinThreads;
    const int b0 = (int)(r0 / N);
    if (LDS) {
        const long long rl = r0 + kRelinThreads - 1 < rows - 1 ? r0 + kRelinThreads - 1 : rows - 1;
        const int nb = (int)(rl / N) - b0 + 1;
        for (int e = tid; e < nb * Mr; e += kRelinThreads) {
            const int pb = e / Mr, k = e - pb * Mr;
            fps[e] = k < M ? Fp[(size_t)(b0 + pb) * M + k] : 0.0f;
        }
        __syncthreads();
    }
    const long long r = r0 + tid;
    if (r >= rows) return;
    const int b = (int)(r / N);
    const int kbf = M >> 2, R = M & 3;
    const long long g = r >> 6;  // the wave's row group: 64 rows, fewer in the batch's last
    const size_t w = rows - 64 * g < 64 ? rows - 64 * g : 64;
    const rf4* pk = reinterpret_cast<const rf4*>(GQ) + (size_t)g * 64 * kbf + (r & 63);
    const float* f = LDS ? fps + (size_t)(b - b0) * Mr : Fp + (size_t)b * M;
    float s = 0.0f;
#pragma unroll 16
    for (int kb = 0; kb < kbf; ++kb) {
        const rf4 g4 = __builtin_nontemporal_load(pk + (size_t)kb * w);
        float f0, f1, f2, f3;
        if (LDS) {
            const rf4 fv = *reinterpret_cast<const rf4*>(f + 4 * kb);
            f0 = fv.x, f1 = fv.y, f2 = fv.z, f3 = fv.w;
        } else {
            f0 = f[4 * kb], f1 = f[4 * kb + 1], f2 = f[4 * kb + 2], f3 = f[4 * kb + 3];
        }
        s += g4.x * f0;
        s += g4.y * f1;
        s += g4.z * f2;
        s += g4.w * f3;
    }
    if (R) {
        const float* tail = GQ + (size_t)rows * kbf * 4 + r;
        for (int t = 0; t < R; ++t) s += tail[(size_t)t * rows] * f[4 * kbf + t];
    }
    Fd[r] = s + 1.0f * Kp[r];  // matrixAdd(Fd, Fd, Kp) :459
}

// {Fdn, Fdp} of a resident problem's stored layouts from its new Fd: the two
// 32-lane / relay fdpn arrays (k_build_split: fdpn[2e] = Fdn, [2e+1] = Fdp)
// and the lean layout's aux words (k_build_lean: aux[4e] = Fdn, [4e+1] = Fdp;
// its Theta word and NaN flags stay).  Null arrays are skipped.
__global__ void __launch_bounds__(256) k_relin_refresh(const float* __restrict__ Fd, int N, float* __restrict__ fdpn0,
                                                       float* __restrict__ fdpn1, float* __restrict__ aux) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= N) return;
    const float fd = Fd[e];
    const float fdn = max_ref(0.0f, -fd);  // matrixNeg(Fdn, Fd) :704
    const float fdp = max_ref(0.0f, fd);   // matrixPos(Fdp, Fd) :703
    if (fdpn0) {
        fdpn0[2 * e + 0] = fdn;
        fdpn0[2 * e + 1] = fdp;
    }
    if (fdpn1) {
        fdpn1[2 * e + 0] = fdn;
        fdpn1[2 * e + 1] = fdp;
    }
    if (aux) {
        aux[4 * e + 0] = fdn;
        aux[4 * e + 1] = fdp;
    }
}

}  // namespace

hipError_t launch_relin_pack(int B, int N, int M, const float* GQ_rowmajor, float* GQ, hipStream_t s) {
    hipLaunchKernelGGL(k_relin_pack, dim3(cdivr((long long)B * N * M, 256)), dim3(256), 0, s, B, N, M, GQ_rowmajor, GQ);
    return hipGetLastError();
}

hipError_t launch_relinearize(int B, int N, int M, const float* GQ, const float* Qinv, const float* Kp,
                              const float* Fp, const float* Mp, float* Fd, float* Md, hipStream_t s) {
    const int md_blocks = M <= kRelinMdLaneMaxM ? (int)cdivr(B, kRelinThreads) : B;
    const unsigned fd_blocks = cdivr((long long)B * N, kRelinThreads);
    // Fp rows a workgroup can need: every problem its 256 rows touch (Fd), one (Md)
    const long long nb = std::min<long long>(B, (kRelinThreads - 1) / N + 2);
    const long long need = nb * relin_round4(M);
    const dim3 grid(md_blocks + fd_blocks), block(kRelinThreads);
    if (need <= kRelinLdsFloats)
        hipLaunchKernelGGL(k_relinearize<true>, grid, block, sizeof(float) * (size_t)need, s, B, N, M, GQ, Qinv, Kp, Fp,
                           Mp, Fd, Md, md_blocks);
    else
        hipLaunchKernelGGL(k_relinearize<false>, grid, block, 0, s, B, N, M, GQ, Qinv, Kp, Fp, Mp, Fd, Md, md_blocks);
    return hipGetLastError();
}

// SolveState{h = 1, resume = 1} for every problem: the start of a warm batched
// solve (k_init_state's, with the iterate taken from SolveArgs::Y as a chunked
// relaunch takes it)
__global__ void k_init_state_warm(int B, SolveState* __restrict__ st) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= B) return;
    SolveState z{};
    z.h = 1;
    z.resume = 1;
    st[b] = z;
}
hipError_t launch_state_init_warm(int B, SolveState* st, hipStream_t s) {
    hipLaunchKernelGGL(k_init_state_warm, dim3(cdivr(B, 256)), dim3(256), 0, s, B, st);
    return hipGetLastError();
}

hipError_t launch_relin_refresh(const float* Fd, int N, float* fdpn0, float* fdpn1, float* aux, hipStream_t s) {
    if (!fdpn0 && !fdpn1 && !aux) return hipSuccess;
    hipLaunchKernelGGL(k_relin_refresh, dim3(cdivr(N, 256)), dim3(256), 0, s, Fd, N, fdpn0, fdpn1, aux);
    return hipGetLastError();
}

}  // namespace pqp
