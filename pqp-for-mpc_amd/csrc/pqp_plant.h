// pqp_plant.h -- internal interface of the resident-plant control step
// (pqp_plant.hip) to the host shim.  Not part of the C ABI.  (Beside
// pqp_launch.h, not in it, like pqp_relin.h: that header's text keys the
// kernels' recorded counter measurements.)
#pragma once
#include "pqp_launch.h"

namespace pqp {

// What k_plant_step reads of one plant: every pointer a device buffer of the
// plant's own, in the reference's row-major layouts.  GQ = Gp Qp_inv [N][M]
// (convertToDual's temporary, :491-492), theta [N] (computeTheta's diagonal).
struct PlantData {
    int N, M, nd, ns;
    const float *Qd, *Gp, *Qp, *Qinv, *Kp, *theta, *GQ;
    const float *Fp1, *Fp2, *Fp3, *Mp1, *Mp2, *Mp3, *Mp4, *Mp5, *Mp6;
};

// One control step's per-state arrays (pqp_plant_step's arguments).
struct PlantStep {
    int B, warm;
    long long max_updates;
    const float *x, *D, *Kp;  // Kp: null (the plant's) or [B][N]
    float *Y, *U;
    long long* h;
    int* status;
    float *Fp, *Mp, *Fd, *Md, *Jp, *Jd;
    float abs_tol, rel_tol;  // the gap tolerances (pqp.h 2k); both 0: the reference's rule alone
};
// A step with a positive tolerance runs the kernels' _tol build (k_plant_step_tol, k_plant_step_mid_tol); every
// other step the build without the tolerances, whose instructions are those it had before them.
inline bool plant_step_tol(const PlantStep& S) { return S.abs_tol > 0.0f || S.rel_tol > 0.0f; }

// Test and tuning knobs of the step (pqp_tune keys "plant_grid", "plant_pipe").
// plant_grid: at most this many workgroups (0: every resident wave slot);
// plant_pipe: 1 the software-pipelined iteration, 0 the plain one (default).
extern int g_plant_grid;
extern int g_plant_pipe;

// The shapes k_plant_step runs: k_solve_wave's (N, M <= 32, N + M < 64), with
// ns, nd <= 64 and the staged operands within one workgroup's LDS.
bool plant_shape_ok(int N, int M, int nd, int ns);
// bytes of LDS one workgroup (one wave) of the step takes
size_t plant_lds_bytes(int N, int M, int nd, int ns);
// NMAX | MMAX << 8 of the k_plant_step instantiation that the launches below pick for (N, M) -- the step in
// both forms and the fused rollout, under either stopping rule: the one choice their dispatch switches over.
// Host only (tests: which cases reach which of the 15 widths).
int plant_widths(int N, int M);
// Workgroups of the form `pipe` resident on the current device at once (its
// CUs times the occupancy of the shape's instantiation); 0 with the error left
// in hipGetLastError.  Queried once per plant, never in a step.
int plant_resident_wgs(int N, int M, int nd, int ns, bool pipe);
// ONE launch: states b = w, w + grid, ... on workgroup w; no allocation, no
// synchronisation.  slots: plant_resident_wgs' count for the form launched.
hipError_t launch_plant_step(const PlantData& P, const PlantStep& S, int slots, bool pipe, hipStream_t s);

// ---- the closed loop (pqp_plant.hip, pqp.h 2j) ----
// The state update x+ = (A x + Bu U) + Bd D as the kernels read it: every
// matrix transposed (k-major), so that the lanes' words of one k are
// consecutive -- AT [ns][ns], BuT [M][ns], BdT [nd][ns], device buffers.
struct DynData {
    int ns, M, nd;
    const float *AT, *BuT, *BdT;
};
// One k_plant_advance launch: xnext [B][ns] from x [B][ns], U [B][M], D [B][nd].
// Y non-null: the launch also floors Y [B][N] (y_floor > Y_i ? y_floor : Y_i),
// the rollout chain's step between two control steps.
struct PlantAdvance {
    int B, N;
    float y_floor;
    const float *x, *U, *D;
    float *xnext, *Y;
};
// What a fused rollout adds to PlantStep, whose arrays then carry a leading K
// axis (U, h, status, Jp, Jd), whose D is [d_steps][B][nd] and whose x is unused.
struct PlantRoll {
    int K, d_steps;  // d_steps: 1 (one D for every step) or K
    float y_floor;   // > 0: applied before every warm start
    float* X;        // [K + 1][B][ns]; row 0 read, rows 1..K written
    DynData dyn;
};
// the fused rollout's second kernel argument: the step's, then the rollout's
struct PlantRollStep : PlantStep {
    PlantRoll R;
};

// Tuning key "plant_roll_chain": 1 runs a kind-1 rollout as the chain of
// step and advance launches too (0, the default: the fused launch).
extern int g_plant_roll_chain;

// M a k_plant_advance launch takes (above 64, Bu is read from memory, not LDS)
constexpr int kDynMaxM = 1024;
// bytes of LDS the dynamics take beside the plant in the fused rollout
size_t plant_dyn_lds_bytes(int M, int nd, int ns);
// The fused rollout runs plant_shape_ok's shapes whose dynamics fit the launch's LDS beside the plant.
bool plant_roll_shape_ok(int N, int M, int nd, int ns);
// Workgroups of the fused rollout resident on the current device at once; 0 with the error in hipGetLastError.
int plant_roll_resident_wgs(int N, int M, int nd, int ns);
// ONE launch each; no allocation, no synchronisation.
hipError_t launch_plant_roll(const PlantData& P, const PlantStep& S, const PlantRoll& R, int slots, hipStream_t s);
hipError_t launch_plant_advance(const DynData& d, const PlantAdvance& a, hipStream_t s);
hipError_t launch_plant_floor(float* Y, size_t n, float y_floor, hipStream_t s);

// ---- the one-workgroup step at horizon sizes (pqp_plant_mid.hip, pqp.h 2g) ----
// What k_solve_mid2 derives from Qd alone when it stages a problem, found once
// at create: sym -- Qd bit-symmetric (Y'Qd's column j read as row j); fast -- no
// NaN in Qd (the v_max / v_med3 splits); qfinite -- fast and no inf (the
// product-first update).  dense: the tuning knob mid2_dense (sum every k).
struct PlantMidFlags {
    int sym, fast, qfinite, dense;
};
// The shapes k_plant_step_mid runs: those the batched path 3 solves on the
// converge-mode k_solve_mid2 at default knobs (M < 64, at most 16 waves, the
// staged matrices within one workgroup's LDS), N or M above 32, nd, ns <= 64.
bool plant_mid_shape_ok(int N, int M, int nd, int ns);
// bytes of LDS one workgroup of the step takes (mid2_layout and the prologue's words)
size_t plant_mid_lds_bytes(int N, int M);
// threads | pair << 16 | lean << 17 | band << 18 of the k_plant_step_mid build that the launch below picks for N,
// under either stopping rule: the workgroup's threads, lane sides (<1024, true>), the lean rings (<384, false, 6>),
// the band table (every build but N <= 64's): the one choice the dispatch of the step and of the fused rollout
// switches over.  Host only (tests: which cases reach which of the four builds).
int plant_mid_build(int N);
// Workgroups resident on the current device at once; 0 with the error left in
// hipGetLastError.  Queried once per plant, never in a step.
int plant_mid_resident_wgs(int N, int M);
// ONE launch: states b = w, w + grid, ... on workgroup w; no allocation, no synchronisation.
hipError_t launch_plant_step_mid(const PlantData& P, const PlantStep& S, const PlantMidFlags& F, int slots,
                                 hipStream_t s);

// ---- the one-workgroup plants' fused rollout (pqp_plant_mid.hip, pqp.h 2l): k_plant_step_mid's ROLL form ----
// Every shape of plant_mid_shape_ok has it: the launch takes the step's LDS (the dynamics are read through L2).
// Workgroups resident on the current device at once; 0 with the error left in hipGetLastError.
int plant_mid_roll_resident_wgs(int N, int M);
// ONE launch of K steps: state b's trajectory on workgroup b mod grid; no allocation, no synchronisation.
// S and R as launch_plant_roll's; slots: plant_mid_roll_resident_wgs' count.
hipError_t launch_plant_roll_mid(const PlantData& P, const PlantStep& S, const PlantMidFlags& F, const PlantRoll& R,
                                 int slots, hipStream_t s);

}  // namespace pqp
