// pqp_plant_mid.hip -- the resident plant's control step at horizon sizes:
// B states of ONE plant in one launch, one workgroup per state at a time
// (pqp.h 2g; k_plant_step, pqp_plant.hip, is the one-wave form for N, M <= 32).
//
// k_plant_step_mid is k_solve_mid2 (pqp_kernels.hip: the roles UW / T / C / cost
// on disjoint waves of one workgroup, terminate() pipelined beside the update)
// with a state loop around it:
//   * the grid is the device's resident workgroups, not B: workgroup w takes
//     states w, w + G, w + 2G, ...
//   * staged ONCE per workgroup, in mid2_layout's arrangement: Qd (stride ldn),
//     Gp', Qp_inv, Qp', the `ones` row, the band table, and in registers the
//     update rows' diagonal literals dP / dN from the plant's precomputed Theta.
//     What k_solve_mid2 derives from Qd alone each launch -- no NaN (FAST),
//     finite (product first), bit-symmetric (Y'Qd by rows) -- comes from create
//     (PlantMidFlags).
//   * per state, a prologue with the bits of pqp_batch_compute_fp / _mp and
//     pqp_batch_relinearize (pqp_plant.hip's, its rows spread over the waves;
//     Fp1..Mp5 and Gp Qp_inv read through L2, Qp_inv from its staged copy), then
//     the refresh of every per-state word of the layout: Fdp / Fdn, Kp, Fp, Fd
//     as row mk of Gp', the Y ring, the tq and U rings, tM, tu, fu, fdy, sums
//     and all 16 flag words.
//   * h, status, the costs and every other output go straight to the caller's
//     arrays: no SolveState, no relaunch (the host bounds max_updates by the
//     batched solvers' per-launch budget).
// The phase loop is restated here, not shared with k_solve_mid2, whose text
// and registers stay as they are (as k_plant_step restated k_solve_wave).
//
// Control flow: the state loop's bounds depend on blockIdx / gridDim / B only;
// the phase loop leaves on a decision that every thread either takes itself
// from the same LDS words between the phase's two barriers, or (DEC1) reads
// from flag[14] after the second barrier.  Every barrier is reached by every
// wave.  Barriers only: no spin wait, nothing between workgroups.
//
// LDS: mid2_layout(N, M, true), whose per-state words come first and whose
// matrices last.  The prologue's own words (x, D, the column sums, Fp'Qp_inv:
// kPmScratch floats, dead once Md is formed) lie over the layout's first words,
// the Y and tq rings, which are filled only after them; where those 5 nk floats
// are fewer, plant_mid_front(N) floats in front of the layout make up the rest.
// So at N >= 80 a workgroup takes exactly k_solve_mid2's LDS, and as many
// workgroups share a CU (two at n_dual 112).
//
// Included by pqp_kernels.hip (after k_solve_mid2's helpers, which it calls, and after pqp_plant.hip, whose
// resident_wgs and plant_launch_grid its launches share).
#include "pqp_plant.h"

#pragma clang fp contract(off)

namespace pqp {

namespace {

constexpr int kPmX = 0, kPmD = 64, kPmR0 = 128, kPmR1 = 192, kPmR3 = 256, kPmTq = 320, kPmDots = 384;
constexpr int kPmScratch = 392;  // floats
// floats in front of the layout (a multiple of 8: the layout stays 16-byte aligned)
__host__ __device__ inline int plant_mid_front(int N) {
    const int rings = 5 * round8(N);  // Y (3 nk) and tq (2 nk), the layout's first words
    return rings >= kPmScratch ? 0 : kPmScratch - rings;
}
constexpr size_t kPlantMidLdsBudget = 150 * 1024;

// The kernel's one argument, and a pointer to where it lies (the kernel
// argument segment) that the compiler cannot see through: what a state's
// prologue and its results read of P and S -- some thirty pointers -- is read
// through a fresh such pointer each time, so none of it is held in registers
// (or spilled and reloaded) through the phase loop between them, as
// k_plant_step's prologue re-derives its offsets from opaque copies.
struct PlantMidArgs {
    PlantData P;
    PlantStep S;
    PlantMidFlags F;
};
typedef const __attribute__((address_space(4))) PlantMidArgs* PlantMidArgsPtr;
__device__ __forceinline__ PlantMidArgsPtr plant_mid_args() {
    PlantMidArgsPtr a = (PlantMidArgsPtr)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(a));
    return a;
}

// The fused rollout's argument (pqp.h 2l): the step's three, each at the offset it has in PlantMidArgs (so
// plant_mid_args() reads them in either kernel), then the rollout's, read through a pointer as opaque.  S's
// arrays then carry a leading K axis (U, h, status, Jp, Jd), its D is [d_steps][B][nd] and its x is unused.
struct PlantMidRollArgs {
    PlantData P;
    PlantStep S;
    PlantMidFlags F;
    PlantRoll R;
};
static_assert(offsetof(PlantMidRollArgs, P) == offsetof(PlantMidArgs, P) &&
                  offsetof(PlantMidRollArgs, S) == offsetof(PlantMidArgs, S) &&
                  offsetof(PlantMidRollArgs, F) == offsetof(PlantMidArgs, F),
              "the step's words keep their offsets");
typedef const __attribute__((address_space(4))) PlantMidRollArgs* PlantMidRollArgsPtr;
__device__ __forceinline__ PlantMidRollArgsPtr plant_mid_roll_args() {
    PlantMidRollArgsPtr a = (PlantMidRollArgsPtr)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(a));
    return a;
}

// The rollout's state update, one matrixMultiply (PQP_CPU.c:84) on one wave: sum over j < n of Mt[j * ld + r] * v_j
// for this lane's row r, in index order from +0.0f, every product rounded before its add.  Mt is k-major in memory
// (the lanes' words of one j consecutive) and v_j is lane j's `vl` (n <= 64).  Eight rows are loaded ahead of their
// adds, so a step pays an eighth of the sum's memory latencies; a row past n - 1 is loaded as row n - 1 and not added.
// Every lane of the wave calls it.
__device__ __forceinline__ float plant_mid_dot_lanes(const float* Mt, int ld, int r, int n, float vl) {
    float s = 0.0f;
    for (int j = 0; j < n; j += 8) {
        float a[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) a[u] = Mt[(j + u < n ? j + u : n - 1) * ld + r];
#pragma unroll
        for (int u = 0; u < 8; ++u)
            if (j + u < n) s += a[u] * __shfl(vl, j + u);
    }
    return s;
}

// k_plant_step_mid and k_plant_step_mid_tol: one text (pqp_plant_mid_step.inc), compiled with and without
// the caller's gap tolerances (pqp.h 2k); k_plant_roll_mid and k_plant_roll_mid_tol: the same
// text with the step loop of the fused rollout (pqp.h 2l)
#define PQP_PLANT_MID_ROLL false
#define PQP_PLANT_MID_KERNEL k_plant_step_mid
#define PQP_PLANT_MID_TOL false
#include "pqp_plant_mid_step.inc"
#undef PQP_PLANT_MID_KERNEL
#undef PQP_PLANT_MID_TOL
#define PQP_PLANT_MID_KERNEL k_plant_step_mid_tol
#define PQP_PLANT_MID_TOL true
#include "pqp_plant_mid_step.inc"
#undef PQP_PLANT_MID_KERNEL
#undef PQP_PLANT_MID_TOL
#undef PQP_PLANT_MID_ROLL
#define PQP_PLANT_MID_ROLL true
#define PQP_PLANT_MID_KERNEL k_plant_roll_mid
#define PQP_PLANT_MID_TOL false
#include "pqp_plant_mid_step.inc"
#undef PQP_PLANT_MID_KERNEL
#undef PQP_PLANT_MID_TOL
#define PQP_PLANT_MID_KERNEL k_plant_roll_mid_tol
#define PQP_PLANT_MID_TOL true
#include "pqp_plant_mid_step.inc"
#undef PQP_PLANT_MID_KERNEL
#undef PQP_PLANT_MID_TOL
#undef PQP_PLANT_MID_ROLL

typedef void (*PlantMidKernel)(PlantMidArgs);
typedef void (*PlantMidRollKernel)(PlantMidRollArgs);

// launch_mid_grid's choice of k_solve_mid2's build at its default knobs
inline bool plant_mid_pair(int N) { return N >= 96 && N <= 128; }
inline int plant_mid_threads(int N) { return 64 * mid2_waves(N, true, plant_mid_pair(N), 64); }

// ---- the dispatch: N to one of the four builds, picked once; then the kernel of a form and a rule ----
// lean: the rings of <384, false, 6>; pair: lane sides (<1024, true>), which start at N = 96, seven waves: never
// lean, so launch_mid_grid's <384, true, 6> has no counterpart; band: the band table (every build but N <= 64's)
struct PlantMidBuild {
    int threads;
    bool pair, lean, band;
};
inline PlantMidBuild plant_mid_pick(int N) {
    const int threads = plant_mid_threads(N);
    const bool lean = threads <= 384;
    return {threads, !lean && plant_mid_pair(N), lean, !lean || N > 64};
}

// tol: the _tol kernel, where the step has a positive tolerance (plant_step_tol)
template <int MAXT, bool PAIR, int MINW = 1, bool BAND = true>
PlantMidKernel plant_mid_kernel_at(bool tol, std::false_type) {
    return tol ? k_plant_step_mid_tol<MAXT, PAIR, MINW, BAND> : k_plant_step_mid<MAXT, PAIR, MINW, BAND>;
}
template <int MAXT, bool PAIR, int MINW = 1, bool BAND = true>
PlantMidRollKernel plant_mid_kernel_at(bool tol, std::true_type) {
    return tol ? k_plant_roll_mid_tol<MAXT, PAIR, MINW, BAND> : k_plant_roll_mid<MAXT, PAIR, MINW, BAND>;
}
// ROLL: the fused rollout's kernel, build for build the step's
template <bool ROLL>
std::conditional_t<ROLL, PlantMidRollKernel, PlantMidKernel> plant_mid_kernel(int N, bool tol = false) {
    const PlantMidBuild b = plant_mid_pick(N);
    const std::bool_constant<ROLL> form;
    if (b.lean && b.band) return plant_mid_kernel_at<384, false, 6>(tol, form);
    if (b.lean) return plant_mid_kernel_at<384, false, 6, false>(tol, form);
    return b.pair ? plant_mid_kernel_at<1024, true>(tol, form) : plant_mid_kernel_at<1024, false>(tol, form);
}

}  // namespace

int plant_mid_build(int N) {
    const PlantMidBuild b = plant_mid_pick(N);
    return b.threads | b.pair << 16 | b.lean << 17 | b.band << 18;
}

size_t plant_mid_lds_bytes(int N, int M) {
    return sizeof(float) * ((size_t)plant_mid_front(N) + (size_t)mid2_layout(N, M, true).total);
}

bool plant_mid_shape_ok(int N, int M, int nd, int ns) {
    if (N < 1 || M < 1 || nd < 1 || ns < 1) return false;
    if (nd > 64 || ns > 64 || M >= 64) return false;
    if (N <= 32 && M <= 32) return false;  // the one-wave step's (or the tiny solvers')
    if (N > 192) return false;             // the band table's three 64-row groups
    if (solve_mid_lds_bytes(N, M, true) > kPlantMidLdsBudget) return false;  // batched path 3
    if (!mid2_fits(N, M, true, plant_mid_pair(N), 64)) return false;
    return plant_mid_lds_bytes(N, M) <= kPlantMidLdsBudget;
}

int plant_mid_resident_wgs(int N, int M) {
    return resident_wgs((const void*)plant_mid_kernel<false>(N), plant_mid_threads(N), plant_mid_lds_bytes(N, M));
}

int plant_mid_roll_resident_wgs(int N, int M) {
    return resident_wgs((const void*)plant_mid_kernel<true>(N), plant_mid_threads(N), plant_mid_lds_bytes(N, M));
}

hipError_t launch_plant_roll_mid(const PlantData& P, const PlantStep& S, const PlantMidFlags& F, const PlantRoll& R,
                                 int slots, hipStream_t s) {
    const PlantMidRollArgs A{P, S, F, R};
    hipLaunchKernelGGL(plant_mid_kernel<true>(P.N, plant_step_tol(S)), dim3(plant_launch_grid(S.B, slots)),
                       dim3(plant_mid_threads(P.N)), plant_mid_lds_bytes(P.N, P.M), s, A);
    return hipGetLastError();
}

hipError_t launch_plant_step_mid(const PlantData& P, const PlantStep& S, const PlantMidFlags& F, int slots,
                                 hipStream_t s) {
    const PlantMidArgs A{P, S, F};
    hipLaunchKernelGGL(plant_mid_kernel<false>(P.N, plant_step_tol(S)), dim3(plant_launch_grid(S.B, slots)),
                       dim3(plant_mid_threads(P.N)), plant_mid_lds_bytes(P.N, P.M), s, A);
    return hipGetLastError();
}

}  // namespace pqp
