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

// ROLL (the fused rollout, pqp.h 2j; S is then a PlantRollStep): a step loop
// inside the state loop.  The wave carries state b through S.R.K steps: after
// each it writes the step's outputs, floors Y, forms x+ = (A x + Bu U) + Bd D
// from the dynamics staged in LDS behind the plant and from the x, U and D it
// still holds, stores the row of X and runs the prologue on it.  Every ROLL
// branch is a compile-time one: the step's instantiations (ROLL false, the
// arguments they always had) compile to the instructions they had without it.
template <int NMAX, int MMAX, bool PIPE, bool ROLL = false>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(plant_min_waves(NMAX, MMAX, PIPE))))
k_plant_step(PlantData P, std::conditional_t<ROLL, PlantRollStep, PlantStep> S) {
    static_assert(NMAX % 4 == 0 && MMAX % 4 == 0 && NMAX <= 32 && MMAX <= 32, "one wave");
    static_assert(!(ROLL && PIPE), "the rollout has the plain iteration only");
    if ((int)blockIdx.x >= S.B) return;  // a wave without a state
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int N = P.N, M = P.M, nd = P.nd, ns = P.ns;
    const PlantLds L = plant_lds(N, M, nd, ns);
    const int lane = threadIdx.x, i = lane >> 1, side = lane & 1;
    float* const xs = lds + L.xs;
    float* const ds = lds + L.ds;
    float* const r0s = lds + L.r0;
    float* const r1s = lds + L.r1;
    float* const r3s = lds + L.r3;
    float* const fps = lds + L.fps;
    float* const tqs = lds + L.tqs;
    float* const fds = lds + L.fds;
    float* const ya = lds + L.ya;
    float* const yb = lds + L.yb;
    float* const rowb = lds + L.rowb;  // Y'Qd
    float* const tb = lds + L.tb;      // t = Gp'Y + Fp
    float* const ub = lds + L.ub;      // U
    float* const rpb = lds + L.rpb;    // U'Qp
    float* const junk = lds + L.junk;

    // ---- once per workgroup: the prologue's operands into LDS ----
    for (int e = lane; e < M * nd; e += 64) lds[L.Fp1 + (e / nd) * L.l1 + e % nd] = P.Fp1[e];
    for (int e = lane; e < M * ns; e += 64) lds[L.Fp2 + (e / ns) * L.l2 + e % ns] = P.Fp2[e];
    for (int e = lane; e < M; e += 64) lds[L.Fp3 + e] = P.Fp3[e];
    for (int e = lane; e < ns * ns; e += 64) lds[L.Mp1 + e] = P.Mp1[e];
    for (int e = lane; e < nd * ns; e += 64) lds[L.Mp2 + e] = P.Mp2[e];
    for (int e = lane; e < nd * nd; e += 64) lds[L.Mp3 + e] = P.Mp3[e];
    for (int e = lane; e < ns; e += 64) lds[L.Mp4 + e] = P.Mp4[e];
    for (int e = lane; e < nd; e += 64) lds[L.Mp5 + e] = P.Mp5[e];
    for (int e = lane; e < N * M; e += 64) lds[L.GQ + (e / M) * L.lg + e % M] = P.GQ[e];
    for (int e = lane; e < M * M; e += 64) lds[L.Qi + e] = P.Qinv[e];
    if constexpr (ROLL) {  // the dynamics, k-major as they are stored, behind the plant
        float* const dl = lds + L.total;
        for (int e = lane; e < ns * ns; e += 64) dl[e] = S.R.dyn.AT[e];
        for (int e = lane; e < M * ns; e += 64) dl[ns * ns + e] = S.R.dyn.BuT[e];
        for (int e = lane; e < nd * ns; e += 64) dl[ns * ns + M * ns + e] = S.R.dyn.BdT[e];
    }
    const float Mp6 = P.Mp6[0];

    // ---- once per wave: the solve loop's matrices (k_solve_wave's setup, with
    // the precomputed Theta; the Fd / Fp lanes are filled per state) ----
    pf2 mat[NMAX];
    pf2 gq[MMAX];
    float qinv[MMAX];
#pragma unroll
    for (int k = 0; k < NMAX; ++k) mat[k] = pf2{0.0f, 0.0f};
#pragma unroll
    for (int j = 0; j < MMAX; ++j) {
        gq[j] = pf2{0.0f, 0.0f};
        qinv[j] = 0.0f;
    }
    const bool rowl = i < N;
    const int ir = rowl ? i : 0;
    const float th = P.theta[ir];  // computeTheta (:503-519)
    const bool colq = lane < N, colg = lane >= N && lane < N + M;
    const int jq = colq ? lane : 0, jg = colg ? lane - N : 0;
    // Fd . Y rides in the pass: on the free .x lane 2N, or (N = 32) the free .y lane N + M
    const int lf = (2 * N < 64) ? 2 * N : N + M;
    const bool fx = (2 * N < 64) && lane == lf, fy = (2 * N >= 64) && lane == lf;
#pragma unroll
    for (int k = 0; k < NMAX; ++k) {
        if (k % 4 == 0) __builtin_amdgcn_sched_barrier(0);
        const int kc = (k < N) ? k : 0;
        const float q = P.Qd[ir * N + kc];
        const float t = (ir == k) ? th : 0.0f;
        const float sp = (side ? max_ref(0.0f, q) : max_ref(0.0f, -q)) + 1.0f * t;  // :524-537
        mat[k].x = (k < N && rowl) ? sp : 0.0f;
        const float qc = P.Qd[kc * N + jq];  // Qd column (Y'Qd)
        const float gc = P.Gp[kc * M + jg];  // Gp column (Gp'Y)
        mat[k].y = (k < N) ? (colq ? qc : (colg ? gc : 0.0f)) : 0.0f;
    }
    const int jm = lane < M ? lane : 0, ig = lane < N ? lane : 0;
#pragma unroll
    for (int j = 0; j < MMAX; ++j) {
        if (j % 4 == 0) __builtin_amdgcn_sched_barrier(0);
        const int jc = (j < M) ? j : 0;
        const float gr = P.Gp[ig * M + jc];    // Gp row (Gp U): row i = lane
        const float qp = P.Qp[jc * M + jm];    // Qp column (U'Qp)
        const float qi = P.Qinv[jm * M + jc];  // Qp_inv row (Qp_inv t)
        gq[j].x = (j < M && lane < N) ? gr : 0.0f;
        gq[j].y = (j < M && lane < M) ? qp : 0.0f;
        qinv[j] = (j < M && lane < M) ? qi : 0.0f;
    }
    __builtin_amdgcn_sched_barrier(0);
    const float kp_plant = (lane < N) ? P.Kp[lane] : 0.0f;
    const int ic = (i < N) ? i : 0;
    const bool wr_y = !side && i < N, wr_row = lane < N, wr_t = lane >= N && lane < N + M, wr_m = lane < MMAX;
    __syncthreads();

    // the fused pass over k: one v_pk_mul + v_pk_add per k
    auto pass = [&](const float* y_) {
        pf2 a = pf2{0.0f, 0.0f};
#pragma unroll
        for (int k = 0; k < NMAX; k += 4) {
            const pf4 y = *reinterpret_cast<const pf4*>(y_ + k);
            a += mat[k] * pf2{y.x, y.x};  // :608-609 / :354 / :652, k in order
            a += mat[k + 1] * pf2{y.y, y.y};
            a += mat[k + 2] * pf2{y.z, y.z};
            a += mat[k + 3] * pf2{y.w, y.w};
        }
        return a;
    };
    // PIPE: every store unconditional (lanes that do not own the word write
    // their own junk word), so no branch splits the iteration; plain: masked stores
    auto put = [&](bool own, float* dst, float v) {
        if constexpr (PIPE) {
            *(own ? dst : junk + lane) = v;
        } else {
            if (own) *dst = v;
        }
    };

    int steps = 1;
    if constexpr (ROLL) steps = S.R.K;
    float ycarry = 0.0f;  // ROLL: the previous step's Y, lanes < N
    for (long long b = blockIdx.x; b < S.B; b += gridDim.x) {
        int k = 0;
        do {  // ROLL: state b's K steps; else once (the body keeps the state loop's indentation)
        // ---- the state's prologue.  Its lane numbers, sizes and LDS offsets
        // are derived afresh from opaque copies, so that none of them is
        // hoisted out of the state loop and held in a register through the
        // solve loop below ----
        int ln = lane, Np = N, Mq = M, ndp = nd, nsp = ns;
        asm volatile("" : "+v"(ln), "+s"(Np), "+s"(Mq), "+s"(ndp), "+s"(nsp));
        const PlantLds Q = plant_lds(Np, Mq, ndp, nsp);
        const float* const Fp1s = lds + Q.Fp1;
        const float* const Fp2s = lds + Q.Fp2;
        const float* const Fp3s = lds + Q.Fp3;
        const float* const Mp1s = lds + Q.Mp1;
        const float* const Mp2s = lds + Q.Mp2;
        const float* const Mp3s = lds + Q.Mp3;
        const float* const Mp4s = lds + Q.Mp4;
        const float* const Mp5s = lds + Q.Mp5;
        const float* const GQs = lds + Q.GQ;
        const float* const Qis = lds + Q.Qi;
        const int pm = ln < Mq ? ln : 0, pn = ln < Np ? ln : 0, pns = ln < nsp ? ln : 0, pnd = ln < ndp ? ln : 0;
        // x, D, the bounds, and the solve loop's vectors as a fresh workgroup has them
        if constexpr (ROLL) {  // x: row 0 of X, then the x+ the previous step left in xs; D: this step's
            if (k == 0 && ln < nsp) xs[ln] = S.R.X[(size_t)b * nsp + ln];
            const float* const Dk = S.D + (S.R.d_steps > 1 ? (size_t)k * S.B * ndp : (size_t)0);
            if (ln < ndp) ds[ln] = Dk[(size_t)b * ndp + ln];
        } else {
            if (ln < nsp) xs[ln] = S.x[(size_t)b * nsp + ln];
            if (ln < ndp) ds[ln] = S.D[(size_t)b * ndp + ln];
        }
        const float kp = S.Kp ? ((lane < N) ? S.Kp[(size_t)b * N + (ROLL ? ln : lane)] : 0.0f) : kp_plant;
        if (ln < 32) {
            if constexpr (ROLL) {  // warm from the previous step's Y (k > 0); floored before every warm start
                float y0 = (k > 0) ? ycarry : ((ln < Np) ? (S.warm ? S.Y[(size_t)b * Np + ln] : 1000.0f) : 0.0f);
                if ((k > 0 || S.warm) && S.R.y_floor > 0.0f && ln < Np) y0 = S.R.y_floor > y0 ? S.R.y_floor : y0;
                ya[ln] = y0;
            } else {
                ya[ln] = (ln < Np) ? (S.warm ? S.Y[(size_t)b * Np + ln] : 1000.0f) : 0.0f;  // initMat(Y, 1000) :710
            }
            yb[ln] = 0.0f;
            rowb[ln] = 0.0f;
            tb[ln] = ub[ln] = rpb[ln] = 0.0f;
        }
        __syncthreads();
        // ---- computeFp (:373) on lanes j < M; x'Mp1, D'Mp2, D'Mp3 one lane per column ----
        float sf2 = 0.0f, r0 = 0.0f;
#pragma unroll 4
        for (int k = 0; k < nsp; ++k) {
            const float xk = xs[k];
            sf2 += Fp2s[pm * Q.l2 + k] * xk;  // Fp2 x
            r0 += xk * Mp1s[k * nsp + pns];   // x' Mp1
        }
        float sf1 = 0.0f, r1 = 0.0f, r3 = 0.0f;
#pragma unroll 4
        for (int k = 0; k < ndp; ++k) {
            const float dk = ds[k];
            sf1 += Fp1s[pm * Q.l1 + k] * dk;  // Fp1 D
            r1 += dk * Mp2s[k * nsp + pns];   // D' Mp2
            r3 += dk * Mp3s[k * ndp + pnd];   // D' Mp3
        }
        float fp = sf1 + 1.0f * sf2;        // matrixAdd(Fp, Fp, tmp, 1)
        fp = fp + -1.0f * Fp3s[pm];         // matrixAdd(Fp, Fp, Fp3, -1)
        if (ln < 32) fps[ln] = (ln < Mq) ? fp : 0.0f;
        r0s[ln] = r0;
        r1s[ln] = r1;
        r3s[ln] = r3;
        if (S.Fp && ln < Mq) S.Fp[(size_t)b * Mq + ln] = fp;
        __syncthreads();
        // ---- Fd = (Gp Qp_inv) Fp + Kp on lanes i < N (:456-459); Fp'Qp_inv one lane per column ----
        float fd = 0.0f, tq = 0.0f;
#pragma unroll 4
        for (int k = 0; k < Mq; ++k) {
            const float fk = fps[k];
            fd += GQs[pn * Q.lg + k] * fk;
            tq += fk * Qis[k * Mq + pm];
        }
        fd = fd + 1.0f * kp;  // matrixAdd(Fd, Fd, Kp, 1) :459
        if (ln < 32) {
            fds[ln] = (ln < Np) ? fd : 0.0f;
            tqs[ln] = (ln < Mq) ? tq : 0.0f;
        }
        if (S.Fd && ln < Np) S.Fd[(size_t)b * Np + ln] = fd;
        __syncthreads();
        // ---- Mp (:397-425) and Md (:475-478): the six ordered dots that end
        // them, one lane each, then the scalars ----
        const float* da = xs;
        const float* db = xs;
        int dlen = 0;
        if (ln == 0) da = r0s, db = xs, dlen = nsp;   // (x'Mp1) . x
        if (ln == 1) da = r1s, db = xs, dlen = nsp;   // (D'Mp2) . x
        if (ln == 2) da = Mp4s, db = xs, dlen = nsp;  // Mp4' x
        if (ln == 3) da = r3s, db = ds, dlen = ndp;   // (D'Mp3) . D
        if (ln == 4) da = Mp5s, db = ds, dlen = ndp;  // Mp5' D
        if (ln == 5) da = tqs, db = fps, dlen = Mq;   // (Fp'Qp_inv) . Fp
        const int dmax = max(max(nsp, ndp), Mq);
        float dot = 0.0f;
#pragma unroll 4
        for (int k = 0; k < dmax; ++k)
            if (k < dlen) dot += da[k] * db[k];
        float Mp = 0.0f;
#pragma unroll
        for (int s = 0; s < 5; ++s) Mp += __int_as_float(__builtin_amdgcn_readlane(__float_as_int(dot), s)) / 2;
        Mp += Mp6 / 2;
        const float Md = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(dot), 5)) + -1.0f * Mp;  // :478
        if (lane == 0) {
            if (S.Mp) S.Mp[b] = Mp;
            if (S.Md) S.Md[b] = Md;
        }
        // ---- this state's lanes of the solve loop's registers ----
#pragma unroll
        for (int k = 0; k < NMAX; k += 4) {
            const pf4 f = *reinterpret_cast<const pf4*>(fds + k);  // Fd (Fd . Y)
            const float fv[4] = {f.x, f.y, f.z, f.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                mat[k + e].x = fx ? fv[e] : mat[k + e].x;
                mat[k + e].y = fy ? fv[e] : mat[k + e].y;
            }
        }
#pragma unroll
        for (int j = 0; j < MMAX; j += 4) {
            const pf4 f = *reinterpret_cast<const pf4*>(fps + j);  // Fp (Fp . U) on the free .x lane N
            const float fv[4] = {f.x, f.y, f.z, f.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) gq[j + e].x = (lane == N) ? fv[e] : gq[j + e].x;
        }
        float fd_own, fp_own;
        {
            const float f = fds[ir];
            fd_own = rowl ? (side ? max_ref(0.0f, f) : max_ref(0.0f, -f)) : 0.0f;  // Fdp / Fdn (:703-704)
            const float g = fps[jg];
            fp_own = colg ? g : 0.0f;
        }

        // ---- solveQuadraticDual's loop (:718-747), k_solve_wave's iteration ----
        long long h = 1;
        int status = kStatusContinue;
        int cb = 0;
        float u_last = 0.0f, Jp_last = 0.0f, Jd_last = 0.0f;
        bool have = false;
        pf2 acc = pf2{0.0f, 0.0f};
        if constexpr (PIPE) acc = pass(ya);
        for (;;) {
            // PIPE (software-pipelined): the pass over the NEXT iterate
            // (speculative: used only if this terminate() says go on) runs
            // beside this iterate's terminate() chains
            const float* cur = cb ? yb : ya;
            float* nxt = cb ? ya : yb;
            float yi = cur[ic];
            asm volatile("" : "+v"(yi));  // read early: its latency hides under the pass
            if constexpr (!PIPE) acc = pass(cur);
            // ---- updateY2's epilogue ----
            {
                const float v = acc.x + 1.0f * fd_own;  // even lane: num (:611), odd lane: den (:612)
                const float den = __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0xB1, 0xF, 0xF, true));
                put(wr_y, nxt + i, v / den * yi);  // :594
            }
            pf2 acc_next = pf2{0.0f, 0.0f};
            if constexpr (PIPE) acc_next = pass(nxt);
            // ---- terminate(): computeUfromY (:352-360) ----
            put(wr_row, rowb + lane, acc.y);
            put(wr_t, tb + (lane - N), acc.y + 1.0f * fp_own);  // tmp = Gp'Y ; tmp += Fp
            const float lin_d = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(fx ? acc.x : acc.y), lf));  // Fd . Y
            // Y'Qd . Y (computeCost, Jd) first: its chain is independent of U's
            float s2 = 0.0f;
#pragma unroll
            for (int k = 0; k < NMAX; k += 4) {
                const pf4 r = *reinterpret_cast<const pf4*>(rowb + k);
                const pf4 y = *reinterpret_cast<const pf4*>(cur + k);
                const pf2 lo = pf2{r.x, r.y} * pf2{y.x, y.y};
                const pf2 hi = pf2{r.z, r.w} * pf2{y.z, y.w};
                s2 += lo.x;
                s2 += lo.y;
                s2 += hi.x;
                s2 += hi.y;
            }
            float ua = 0.0f;
#pragma unroll
            for (int j = 0; j < MMAX; j += 4) {
                const pf4 t = *reinterpret_cast<const pf4*>(tb + j);
                ua += qinv[j] * t.x;
                ua += qinv[j + 1] * t.y;
                ua += qinv[j + 2] * t.z;
                ua += qinv[j + 3] * t.w;
            }
            const float u = (lane < M) ? -ua : 0.0f;  // U = -U
            put(wr_m, ub + lane, u);
            // ---- checkFeas (Gp U vs Kp) and U'Qp in one pass over j ----
            pf2 g = pf2{0.0f, 0.0f};
            float uv[MMAX];
#pragma unroll
            for (int j = 0; j < MMAX; j += 4) {
                const pf4 t = *reinterpret_cast<const pf4*>(ub + j);
                uv[j] = t.x;
                uv[j + 1] = t.y;
                uv[j + 2] = t.z;
                uv[j + 3] = t.w;
            }
#pragma unroll
            for (int j = 0; j < MMAX; ++j) g += gq[j] * pf2{uv[j], uv[j]};
            const int bad = (lane < N) && (g.x > kp + max_ref((float)(kTol * kp), (float)kTol));
            const bool infeasible = __any(bad);
            put(wr_m, rpb + lane, g.y);
            const float lin_p = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(g.x), N));  // Fp . U
            // ---- computeCost (:648-666): U'Qp . U and Y'Qd . Y, sequential ----
            float quad = 0.0f;
#pragma unroll
            for (int j = 0; j < MMAX; j += 4) {
                const pf4 r = *reinterpret_cast<const pf4*>(rpb + j);
                quad += r.x * uv[j];
                quad += r.y * uv[j + 1];
                quad += r.z * uv[j + 2];
                quad += r.w * uv[j + 3];
            }
            u_last = u;
            // ---- the gap tests (:673-687), wave-uniform ----
            int stop = 0;
            if (!infeasible) {
                float Jp = 0.0f;
                Jp = (float)((double)Jp + 0.5 * (double)quad);
                Jp += lin_p;
                Jp += Mp / 2;
                float Jd = 0.0f;
                Jd = (float)((double)Jd + 0.5 * (double)s2);
                Jd += lin_d;
                Jd += Md / 2;
                stop = gap_stop(Jp, Jd);  // :683-685
                Jp_last = Jp;
                Jd_last = Jd;
                have = true;
            }
            if (stop) {
                status = kStatusDone;
                break;
            }
            if (h - 1 >= S.max_updates) {
                status = kStatusCapped;
                break;
            }
            cb ^= 1;  // accept the update
            if constexpr (PIPE) acc = acc_next;
            ++h;
        }
        // ---- the state's results ----
        const float* yfin = cb ? yb : ya;
        if constexpr (ROLL) {
            // ---- the step's results, row k of the [K][B] arrays; Y is the last step's.  Lane
            // numbers, sizes and offsets from opaque copies, as the prologue's ----
            int l2 = lane, N2 = N, M2 = M, nd2 = nd, ns2 = ns;
            asm volatile("" : "+v"(l2), "+s"(N2), "+s"(M2), "+s"(nd2), "+s"(ns2));
            const size_t kb = (size_t)k * S.B + b;
            if (k == steps - 1 && l2 < N2) S.Y[(size_t)b * N2 + l2] = yfin[l2];
            if (l2 < M2) S.U[kb * M2 + l2] = u_last;
            if (l2 == 0) {
                if (S.h) S.h[kb] = h;
                if (S.status) S.status[kb] = status;
                if (S.Jp) S.Jp[kb] = have ? Jp_last : __builtin_nanf("");
                if (S.Jd) S.Jd[kb] = have ? Jd_last : __builtin_nanf("");
            }
            // ---- x+ = (A x + 1 Bu U) + 1 Bd D, one lane per row: three matrixMultiply (:84), two
            // matrixAdd (:157), from the x, U (the last terminate()'s, in ub) and D in LDS.  Not
            // unrolled: a few hundred products per step, beside the solve loop's live registers ----
            const float* const ATs = lds + plant_lds(N2, M2, nd2, ns2).total;
            const float* const BuTs = ATs + ns2 * ns2;
            const float* const BdTs = BuTs + M2 * ns2;
            const int pr = l2 < ns2 ? l2 : 0;
            float t = 0.0f, v = 0.0f, w = 0.0f;
#pragma unroll 1
            for (int j = 0; j < ns2; ++j) t += ATs[j * ns2 + pr] * xs[j];
#pragma unroll 1
            for (int j = 0; j < M2; ++j) v += BuTs[j * ns2 + pr] * ub[j];
#pragma unroll 1
            for (int j = 0; j < nd2; ++j) w += BdTs[j * ns2 + pr] * ds[j];
            float xn = t + 1.0f * v;
            xn = xn + 1.0f * w;
            const float yc = (l2 < N2) ? yfin[l2] : 0.0f;
            __syncthreads();  // x, U, D and Y are read: xs and, in the next prologue, the rest are rewritten
            ycarry = yc;
            if (l2 < ns2) {
                xs[l2] = xn;
                S.R.X[((size_t)(k + 1) * S.B + b) * ns2 + l2] = xn;
            }
        } else {
            if (lane < N) S.Y[(size_t)b * N + lane] = yfin[lane];
            if (lane < M) S.U[(size_t)b * M + lane] = u_last;  // computeUfromY wrote U on every terminate(): the last one stands
            if (lane == 0) {
                if (S.h) S.h[b] = h;
                if (S.status) S.status[b] = status;
                if (S.Jp) S.Jp[b] = have ? Jp_last : __builtin_nanf("");
                if (S.Jd) S.Jd[b] = have ? Jd_last : __builtin_nanf("");
            }
        }
        __syncthreads();  // the next state's stores come after this one's reads
        } while (ROLL && ++k < steps);
    }
}

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

typedef void (*PlantKernel)(PlantData, PlantStep);

template <int NMAX, bool PIPE>
PlantKernel plant_kernel_m(int M) {
    if (M <= 8) return k_plant_step<NMAX, 8, PIPE>;
    if (M <= 16) return k_plant_step<NMAX, 16, PIPE>;
    return k_plant_step<NMAX, 32, PIPE>;
}
template <bool PIPE>
PlantKernel plant_kernel_n(int N, int M) {
    // the unrolled sums run to the next instantiated width >= N (>= M), as launch_tiny_grid's
    if (N <= 8) return plant_kernel_m<8, PIPE>(M);
    if (N <= 16) return plant_kernel_m<16, PIPE>(M);
    if (N <= 24) return plant_kernel_m<24, PIPE>(M);
    if (N <= 28) return plant_kernel_m<28, PIPE>(M);
    return plant_kernel_m<32, PIPE>(M);
}
PlantKernel plant_kernel(int N, int M, bool pipe) {
    return pipe ? plant_kernel_n<true>(N, M) : plant_kernel_n<false>(N, M);
}

typedef void (*RollKernel)(PlantData, PlantRollStep);

template <int NMAX>
RollKernel roll_kernel_m(int M) {
    if (M <= 8) return k_plant_step<NMAX, 8, false, true>;
    if (M <= 16) return k_plant_step<NMAX, 16, false, true>;
    return k_plant_step<NMAX, 32, false, true>;
}
RollKernel roll_kernel(int N, int M) {  // plant_kernel's widths
    if (N <= 8) return roll_kernel_m<8>(M);
    if (N <= 16) return roll_kernel_m<16>(M);
    if (N <= 24) return roll_kernel_m<24>(M);
    if (N <= 28) return roll_kernel_m<28>(M);
    return roll_kernel_m<32>(M);
}

}  // namespace

int g_plant_roll_chain = 0;

size_t plant_dyn_lds_bytes(int M, int nd, int ns) { return sizeof(float) * ((size_t)ns * ns + (size_t)M * ns + (size_t)nd * ns); }

bool plant_roll_shape_ok(int N, int M, int nd, int ns) {
    return plant_shape_ok(N, M, nd, ns) && plant_lds_bytes(N, M, nd, ns) + plant_dyn_lds_bytes(M, nd, ns) <= kPlantLdsBudget;
}

int plant_roll_resident_wgs(int N, int M, int nd, int ns) {
    int dev = 0, cus = 0, per_cu = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, roll_kernel(N, M), 64,
                                                     plant_lds_bytes(N, M, nd, ns) + plant_dyn_lds_bytes(M, nd, ns)) !=
        hipSuccess)
        return 0;
    return cus * per_cu;
}

hipError_t launch_plant_roll(const PlantData& P, const PlantStep& S, const PlantRoll& R, int slots, hipStream_t s) {
    int grid = S.B < slots ? S.B : slots;
    if (g_plant_grid > 0 && grid > g_plant_grid) grid = g_plant_grid;
    if (grid < 1) grid = 1;
    PlantRollStep SR{};
    static_cast<PlantStep&>(SR) = S;
    SR.R = R;
    hipLaunchKernelGGL(roll_kernel(P.N, P.M), dim3(grid), dim3(64),
                       plant_lds_bytes(P.N, P.M, P.nd, P.ns) + plant_dyn_lds_bytes(P.M, P.nd, P.ns), s, P, SR);
    return hipGetLastError();
}

hipError_t launch_plant_advance(const DynData& d, const PlantAdvance& a, hipStream_t s) {
    const long long groups = ((long long)a.B + kAdvWaves - 1) / kAdvWaves;
    int grid = (int)(groups < 2048 ? groups : 2048);
    if (g_plant_grid > 0 && grid > g_plant_grid) grid = g_plant_grid;
    if (grid < 1) grid = 1;
    hipLaunchKernelGGL(k_plant_advance, dim3(grid), dim3(64 * kAdvWaves),
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
    int dev = 0, cus = 0, per_cu = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, plant_kernel(N, M, pipe), 64,
                                                     plant_lds_bytes(N, M, nd, ns)) != hipSuccess)
        return 0;
    return cus * per_cu;
}

hipError_t launch_plant_step(const PlantData& P, const PlantStep& S, int slots, bool pipe, hipStream_t s) {
    int grid = S.B < slots ? S.B : slots;
    if (g_plant_grid > 0 && grid > g_plant_grid) grid = g_plant_grid;
    if (grid < 1) grid = 1;
    hipLaunchKernelGGL(plant_kernel(P.N, P.M, pipe), dim3(grid), dim3(64), plant_lds_bytes(P.N, P.M, P.nd, P.ns), s, P,
                       S);
    return hipGetLastError();
}

}  // namespace pqp
