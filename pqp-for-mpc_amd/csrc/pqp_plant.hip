// pqp_plant.hip -- one control step of B states of ONE plant in one launch.
//
// In the MPC workload every problem of a batch is the same plant at another
// state: Qp_inv, Gp, Kp (and so Qp, Qd, Theta, Gp Qp_inv) are shared, only x
// and D differ, and through them Fp, Mp, Fd, Md.  k_plant_step keeps the plant
// once (PlantData) and, per state b, computes
//   Fp = (Fp1 D + Fp2 x) - Fp3                                   computeFp  :373
//   Mp = sum of the halved terms x'Mp1 x, D'Mp2 x, Mp4'x, D'Mp3 D, Mp5'D, Mp6   :395
//   Fd = (Gp Qp_inv) Fp + Kp,  Md = (Fp'Qp_inv) Fp - Mp          convertToDual :456-479
// and then runs solveQuadraticDual's converge loop (:694-750) from Y = 1000 or
// from the caller's Y -- the arithmetic of pqp_batch_compute_fp / _mp,
// pqp_batch_relinearize and k_solve_wave, bit for bit: every sum runs k in
// order from +0.0f, every product is rounded before its add (no FMA), every
// matrixAdd is a + sign * b.
//
// One wave (one 64-thread workgroup) per state at a time, with k_solve_wave's
// lane assignment and iteration (pqp_kernels.hip); what differs:
//   * the grid is the device's resident wave slots, not B: workgroup w takes
//     states w, w + G, w + 2G, ...  The solve loop's matrix registers (mat, gq,
//     qinv) are loaded once per wave from the shared plant, Theta comes
//     precomputed, and the prologue's operands (Fp1..Mp5, Gp Qp_inv, Qp_inv)
//     are staged in LDS once per workgroup.
//   * a per-state prologue computes Fp, Mp, Fd, Md: the row sums one lane per
//     row (row strides odd: 32 lanes read 32 banks), the column sums one lane
//     per column (consecutive words), and the six ordered dot products that
//     end Mp and Md on six lanes side by side, from LDS.  The lanes that carry
//     Fd . Y and Fp . U in the solve loop's passes, and Fdp / Fdn / Fp / Kp,
//     are refreshed from it.
//   * h, status, the costs and every other output go straight to the caller's
//     arrays: no SolveState, no pending counter, no relaunch.  The host bounds
//     max_updates by the batched solvers' per-launch budget.
// Every loop bound is wave-uniform, so the workgroup's barriers (one wave:
// they only order the LDS traffic) are reached by all 64 lanes.
//
// The closed loop (pqp.h 2j) is here too: k_plant_advance, the state update
// x+ = (A x + Bu U) + Bd D of B states in the reference's matrixMultiply /
// matrixAdd arithmetic, and k_plant_step's ROLL form, in which the wave takes
// its state through K steps -- step, outputs, floor, x+, prologue -- with the
// dynamics staged in LDS behind the plant.
#include <type_traits>

#include "pqp_device.h"
#include "pqp_plant.h"

#pragma clang fp contract(off)

namespace pqp {

int g_plant_grid = 0;
// The plain iteration is the default: on 16384 bundled-plant states it holds 3
// waves per SIMD against the pipelined form's 2 and measured faster both warm
// (0.060 against 0.064 ms per step: the speculative pass is wasted when the
// first terminate() stops) and cold (2.34 against 2.42); DESIGN.md 4e.
int g_plant_pipe = 0;

namespace {

typedef float pf2 __attribute__((ext_vector_type(2)));
typedef float pf4 __attribute__((ext_vector_type(4)));

constexpr size_t kPlantLdsBudget = 150 * 1024;

// LDS of one workgroup, in floats.  First the per-state vectors (each 16-byte
// aligned, zero-padded to its full width), then the staged plant operands.
struct PlantLds {
    // per state
    int xs, ds, r0, r1, r3;        // 64 each: x, D, x'Mp1, D'Mp2, D'Mp3
    int fps, tqs, fds;             // 32 each: Fp, Fp'Qp_inv, Fd
    int ya, yb, rowb, tb, ub, rpb; // 32 each: the solve loop's (k_solve_wave)
    int junk;                      // 64: the pipelined form's store sink
    // per workgroup
    int l1, l2, lg;                // row strides of Fp1, Fp2, GQ (odd)
    int Fp1, Fp2, Fp3, Mp1, Mp2, Mp3, Mp4, Mp5, GQ, Qi;
    int total;
};
__host__ __device__ inline PlantLds plant_lds(int N, int M, int nd, int ns) {
    PlantLds L;
    int o = 0;
    L.xs = o;   o += 64;
    L.ds = o;   o += 64;
    L.r0 = o;   o += 64;
    L.r1 = o;   o += 64;
    L.r3 = o;   o += 64;
    L.fps = o;  o += 32;
    L.tqs = o;  o += 32;
    L.fds = o;  o += 32;
    L.ya = o;   o += 32;
    L.yb = o;   o += 32;
    L.rowb = o; o += 32;
    L.tb = o;   o += 32;
    L.ub = o;   o += 32;
    L.rpb = o;  o += 32;
    L.junk = o; o += 64;
    L.l1 = nd | 1;
    L.l2 = ns | 1;
    L.lg = M | 1;
    L.Fp1 = o;  o += M * L.l1;
    L.Fp2 = o;  o += M * L.l2;
    L.Fp3 = o;  o += M;
    L.Mp1 = o;  o += ns * ns;
    L.Mp2 = o;  o += nd * ns;
    L.Mp3 = o;  o += nd * nd;
    L.Mp4 = o;  o += ns;
    L.Mp5 = o;  o += nd;
    L.GQ = o;   o += N * L.lg;
    L.Qi = o;   o += M * M;
    L.total = o;
    return L;
}

// The waves per SIMD k_solve_wave's plain form reaches at the same widths: the
// register budget each instantiation is held to (the state loop's extra live
// values would otherwise cost a wave per SIMD at 6 of the 15 widths, the
// bundled plant's among them).
__host__ __device__ constexpr int plant_min_waves(int NMAX, int MMAX, bool PIPE) {
    if (PIPE) return 1;
    if (MMAX == 8) return NMAX <= 8 ? 5 : (NMAX <= 16 ? 4 : (NMAX <= 28 ? 3 : 2));
    if (MMAX == 16) return NMAX <= 8 ? 4 : (NMAX <= 16 ? 3 : 2);
    return NMAX <= 24 ? 2 : 1;
}

// k_plant_step and k_plant_step_tol: one text (pqp_plant_step.inc), compiled with and without the
// caller's gap tolerances (pqp.h 2k)
#define PQP_PLANT_STEP_KERNEL k_plant_step
#define PQP_PLANT_STEP_TOL false
#include "pqp_plant_step.inc"
#undef PQP_PLANT_STEP_KERNEL
#undef PQP_PLANT_STEP_TOL
#define PQP_PLANT_STEP_KERNEL k_plant_step_tol
#define PQP_PLANT_STEP_TOL true
#include "pqp_plant_step.inc"
#undef PQP_PLANT_STEP_KERNEL
#undef PQP_PLANT_STEP_TOL

// ---- x+ = (A x + 1 Bu U) + 1 Bd D for B states (pqp_dynamics_advance, the
// rollout chain): one lane per row of x+, one wave per state at a time, four
// waves per workgroup; AT, BdT and (M <= 64) BuT staged in LDS once per
// workgroup, k-major, so a wave's words of one k are consecutive.  A wider Bu
// (the shared plant's M) is read from memory, k-major too.  Sums as the
// reference's matrixMultiply (:84): k in order from +0.0f, every product
// rounded before its add; then matrixAdd (:157) twice.  The group loop's bound
// is workgroup-uniform, so every wave reaches the barriers. ----
constexpr int kAdvWaves = 4;

__host__ __device__ inline int advance_lds_floats(int ns, int M, int nd) {
    return ns * ns + (M <= 64 ? M * ns : 0) + nd * ns + kAdvWaves * 192;
}

__global__ void __launch_bounds__(64 * kAdvWaves) k_plant_advance(DynData d, PlantAdvance a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int ns = d.ns, M = d.M, nd = d.nd;
    const bool bu_lds = M <= 64;
    float* const ATs = lds;
    float* const BuTs = ATs + ns * ns;
    float* const BdTs = BuTs + (bu_lds ? M * ns : 0);
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    float* const xv = BdTs + nd * ns + wave * 192;  // this wave's x, D, U: 64 words each
    float* const dv = xv + 64;
    float* const uv = xv + 128;
    for (int e = tid; e < ns * ns; e += 64 * kAdvWaves) ATs[e] = d.AT[e];
    if (bu_lds)
        for (int e = tid; e < M * ns; e += 64 * kAdvWaves) BuTs[e] = d.BuT[e];
    for (int e = tid; e < nd * ns; e += 64 * kAdvWaves) BdTs[e] = d.BdT[e];
    __syncthreads();
    const int pr = lane < ns ? lane : 0;
    const long long groups = ((long long)a.B + kAdvWaves - 1) / kAdvWaves;
    for (long long g = blockIdx.x; g < groups; g += gridDim.x) {
        const long long b = g * kAdvWaves + wave;
        const bool live = b < a.B;  // wave-uniform
        if (live) {
            if (lane < ns) xv[lane] = a.x[(size_t)b * ns + lane];
            if (lane < nd) dv[lane] = a.D[(size_t)b * nd + lane];
            if (bu_lds && lane < M) uv[lane] = a.U[(size_t)b * M + lane];
        }
        __syncthreads();
        if (live) {
            float t = 0.0f, v = 0.0f, w = 0.0f;
#pragma unroll 4
            for (int j = 0; j < ns; ++j) t += ATs[j * ns + pr] * xv[j];
            if (bu_lds) {
#pragma unroll 4
                for (int j = 0; j < M; ++j) v += BuTs[j * ns + pr] * uv[j];
            } else {
                const float* const Ub = a.U + (size_t)b * M;
#pragma unroll 4
                for (int j = 0; j < M; ++j) v += d.BuT[(size_t)j * ns + pr] * Ub[j];
            }
#pragma unroll 4
            for (int j = 0; j < nd; ++j) w += BdTs[j * ns + pr] * dv[j];
            float xn = t + 1.0f * v;
            xn = xn + 1.0f * w;
            if (lane < ns) a.xnext[(size_t)b * ns + lane] = xn;
            if (a.Y)
                for (int i = lane; i < a.N; i += 64) {
                    const float y = a.Y[(size_t)b * a.N + i];
                    a.Y[(size_t)b * a.N + i] = a.y_floor > y ? a.y_floor : y;
                }
        }
        __syncthreads();  // the next group's x, D, U come after this one's reads
    }
}

// Y_i = y_floor > Y_i ? y_floor : Y_i over n words: the floor before a rollout chain's first, warm, step
__global__ void __launch_bounds__(256) k_plant_floor(float* Y, size_t n, float y_floor) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const float y = Y[i];
        Y[i] = y_floor > y ? y_floor : y;
    }
}

// ---- the dispatch: (N, M) to one of the 15 widths, picked once; then the kernel of a form and a rule ----
// The unrolled sums run to the next instantiated width >= N (>= M), as launch_tiny_grid's.
struct PlantWidths {
    int nmax, mmax;
};
inline PlantWidths plant_pick_widths(int N, int M) {
    return {N <= 8 ? 8 : N <= 16 ? 16 : N <= 24 ? 24 : N <= 28 ? 28 : 32, M <= 8 ? 8 : M <= 16 ? 16 : 32};
}

// PIPE: the pipelined step; ROLL: the fused rollout; neither: the plain step
template <bool PIPE, bool ROLL>
using PlantKernel = void (*)(PlantData, std::conditional_t<ROLL, PlantRollStep, PlantStep>);

// tol: k_plant_step_tol, where the step has a positive tolerance (plant_step_tol)
template <bool PIPE, bool ROLL, int NMAX, int MMAX>
PlantKernel<PIPE, ROLL> plant_kernel_at(bool tol) {
    return tol ? k_plant_step_tol<NMAX, MMAX, PIPE, ROLL> : k_plant_step<NMAX, MMAX, PIPE, ROLL>;
}
template <bool PIPE, bool ROLL, int NMAX>
PlantKernel<PIPE, ROLL> plant_kernel_m(int mmax, bool tol) {
    switch (mmax) {
        case 8: return plant_kernel_at<PIPE, ROLL, NMAX, 8>(tol);
        case 16: return plant_kernel_at<PIPE, ROLL, NMAX, 16>(tol);
        default: return plant_kernel_at<PIPE, ROLL, NMAX, 32>(tol);
    }
}
template <bool PIPE, bool ROLL>
PlantKernel<PIPE, ROLL> plant_kernel(int N, int M, bool tol = false) {
    const PlantWidths w = plant_pick_widths(N, M);
    switch (w.nmax) {
        case 8: return plant_kernel_m<PIPE, ROLL, 8>(w.mmax, tol);
        case 16: return plant_kernel_m<PIPE, ROLL, 16>(w.mmax, tol);
        case 24: return plant_kernel_m<PIPE, ROLL, 24>(w.mmax, tol);
        case 28: return plant_kernel_m<PIPE, ROLL, 28>(w.mmax, tol);
        default: return plant_kernel_m<PIPE, ROLL, 32>(w.mmax, tol);
    }
}
PlantKernel<false, false> plant_step_kernel(int N, int M, bool pipe, bool tol = false) {
    return pipe ? plant_kernel<true, false>(N, M, tol) : plant_kernel<false, false>(N, M, tol);
}

size_t plant_roll_lds_bytes(int N, int M, int nd, int ns) {
    return plant_lds_bytes(N, M, nd, ns) + plant_dyn_lds_bytes(M, nd, ns);
}

// ---- what every launch of the plant family shares (pqp_plant_mid.hip's too: it is included after this file) ----
// Workgroups of `kernel` (`threads` each, `lds` bytes of dynamic LDS) resident on the current device at once: its
// CUs times the kernel's occupancy; 0 with the error left in hipGetLastError.  What every *_resident_wgs asks, of
// its shape's instantiation.
int resident_wgs(const void* kernel, int threads, size_t lds) {
    int dev = 0, cus = 0, per_cu = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, threads, lds) != hipSuccess) return 0;
    return cus * per_cu;
}
// The grid of a launch over B states (or groups of states): min(B, slots), then at most plant_grid, at least 1.
int plant_launch_grid(long long B, int slots) {
    int grid = (int)(B < slots ? B : slots);
    if (g_plant_grid > 0 && grid > g_plant_grid) grid = g_plant_grid;
    return grid < 1 ? 1 : grid;
}

}  // namespace

int plant_widths(int N, int M) {
    const PlantWidths w = plant_pick_widths(N, M);
    return w.nmax | w.mmax << 8;
}

int g_plant_roll_chain = 0;

size_t plant_dyn_lds_bytes(int M, int nd, int ns) { return sizeof(float) * ((size_t)ns * ns + (size_t)M * ns + (size_t)nd * ns); }

bool plant_roll_shape_ok(int N, int M, int nd, int ns) {
    return plant_shape_ok(N, M, nd, ns) && plant_roll_lds_bytes(N, M, nd, ns) <= kPlantLdsBudget;
}

int plant_roll_resident_wgs(int N, int M, int nd, int ns) {
    return resident_wgs((const void*)plant_kernel<false, true>(N, M), 64, plant_roll_lds_bytes(N, M, nd, ns));
}

hipError_t launch_plant_roll(const PlantData& P, const PlantStep& S, const PlantRoll& R, int slots, hipStream_t s) {
    PlantRollStep SR{};
    static_cast<PlantStep&>(SR) = S;
    SR.R = R;
    hipLaunchKernelGGL((plant_kernel<false, true>(P.N, P.M, plant_step_tol(S))), dim3(plant_launch_grid(S.B, slots)),
                       dim3(64), plant_roll_lds_bytes(P.N, P.M, P.nd, P.ns), s, P, SR);
    return hipGetLastError();
}

hipError_t launch_plant_advance(const DynData& d, const PlantAdvance& a, hipStream_t s) {
    const long long groups = ((long long)a.B + kAdvWaves - 1) / kAdvWaves;
    hipLaunchKernelGGL(k_plant_advance, dim3(plant_launch_grid(groups, 2048)), dim3(64 * kAdvWaves),
                       sizeof(float) * (size_t)advance_lds_floats(d.ns, d.M, d.nd), s, d, a);
    return hipGetLastError();
}

hipError_t launch_plant_floor(float* Y, size_t n, float y_floor, hipStream_t s) {
    const size_t blocks = (n + 255) / 256;
    hipLaunchKernelGGL(k_plant_floor, dim3((unsigned)(blocks < 1024 ? blocks : 1024)), dim3(256), 0, s, Y, n, y_floor);
    return hipGetLastError();
}

size_t plant_lds_bytes(int N, int M, int nd, int ns) { return sizeof(float) * (size_t)plant_lds(N, M, nd, ns).total; }

bool plant_shape_ok(int N, int M, int nd, int ns) {
    if (N < 1 || M < 1 || nd < 1 || ns < 1) return false;
    if (N > 32 || M > 32 || N + M >= 64 || nd > 64 || ns > 64) return false;
    return plant_lds_bytes(N, M, nd, ns) <= kPlantLdsBudget;
}

int plant_resident_wgs(int N, int M, int nd, int ns, bool pipe) {
    return resident_wgs((const void*)plant_step_kernel(N, M, pipe), 64, plant_lds_bytes(N, M, nd, ns));
}

hipError_t launch_plant_step(const PlantData& P, const PlantStep& S, int slots, bool pipe, hipStream_t s) {
    hipLaunchKernelGGL(plant_step_kernel(P.N, P.M, pipe, plant_step_tol(S)), dim3(plant_launch_grid(S.B, slots)),
                       dim3(64), plant_lds_bytes(P.N, P.M, P.nd, P.ns), s, P, S);
    return hipGetLastError();
}

}  // namespace pqp
