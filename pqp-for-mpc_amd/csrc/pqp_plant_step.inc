// pqp_plant_step.inc -- the text of k_plant_step (pqp_plant.hip), which includes it twice:
//   PQP_PLANT_STEP_KERNEL k_plant_step,     PQP_PLANT_STEP_TOL false: the reference's stopping rule alone
//   PQP_PLANT_STEP_KERNEL k_plant_step_tol, PQP_PLANT_STEP_TOL true:  then the caller's gap tolerances (pqp.h 2k)
// Two kernels of one text, not a flag in the arguments: with the flag compiled out, k_plant_step's 45
// instantiations keep the instructions they had before the tolerances existed (DESIGN.md 4k), and their
// names.  Not a wrapper around a shared inline body either, which changes all of them (DESIGN.md 4j).
//
// ROLL (the fused rollout, pqp.h 2j; S is then a PlantRollStep): a step loop
// inside the state loop.  The wave carries state b through S.R.K steps: after
// each it writes the step's outputs, floors Y, forms x+ = (A x + Bu U) + Bd D
// from the dynamics staged in LDS behind the plant and from the x, U and D it
// still holds, stores the row of X and runs the prologue on it.  Every ROLL
// branch is a compile-time one: the step's instantiations (ROLL false, the
// arguments they always had) compile to the instructions they had without it.
template <int NMAX, int MMAX, bool PIPE, bool ROLL = false>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(plant_min_waves(NMAX, MMAX, PIPE))))
PQP_PLANT_STEP_KERNEL(PlantData P, std::conditional_t<ROLL, PlantRollStep, PlantStep> S) {
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
                stop = gap_stop(Jp, Jd) ? kStatusDone : 0;  // :683-685
                if constexpr (PQP_PLANT_STEP_TOL)  // then the caller's tolerances (pqp.h 2k), wave-uniform
                    if (!stop) stop = tol_stop(Jp, Jd, S.abs_tol, S.rel_tol);
                Jp_last = Jp;
                Jd_last = Jd;
                have = true;
            }
            if (stop) {
                status = PQP_PLANT_STEP_TOL ? stop : kStatusDone;  // (kStatusDone or kStatusTol)
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
