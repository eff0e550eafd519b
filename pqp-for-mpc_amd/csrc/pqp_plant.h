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
};

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
// Workgroups of the form `pipe` resident on the current device at once (its
// CUs times the occupancy of the shape's instantiation); 0 with the error left
// in hipGetLastError.  Queried once per plant, never in a step.
int plant_resident_wgs(int N, int M, int nd, int ns, bool pipe);
// ONE launch: states b = w, w + grid, ... on workgroup w; no allocation, no
// synchronisation.  slots: plant_resident_wgs' count for the form launched.
hipError_t launch_plant_step(const PlantData& P, const PlantStep& S, int slots, bool pipe, hipStream_t s);

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
// Workgroups resident on the current device at once; 0 with the error left in
// hipGetLastError.  Queried once per plant, never in a step.
int plant_mid_resident_wgs(int N, int M);
// ONE launch: states b = w, w + grid, ... on workgroup w; no allocation, no synchronisation.
hipError_t launch_plant_step_mid(const PlantData& P, const PlantStep& S, const PlantMidFlags& F, int slots,
                                 hipStream_t s);

}  // namespace pqp
