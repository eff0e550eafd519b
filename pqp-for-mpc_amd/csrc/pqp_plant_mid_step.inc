// pqp_plant_mid_step.inc -- the text of k_plant_step_mid (pqp_plant_mid.hip), which includes it twice:
//   PQP_PLANT_MID_KERNEL k_plant_step_mid,     PQP_PLANT_MID_TOL false: the reference's stopping rule alone
//   PQP_PLANT_MID_KERNEL k_plant_step_mid_tol, PQP_PLANT_MID_TOL true:  then the caller's gap tolerances (pqp.h 2k)
// Two kernels of one text, as pqp_plant_step.inc: with the flag compiled out, k_plant_step_mid's four builds
// keep the instructions they had before the tolerances existed (DESIGN.md 4k).
//
// and twice more with PQP_PLANT_MID_ROLL true (false above), the fused rollout of pqp.h 2l:
//   PQP_PLANT_MID_KERNEL k_plant_roll_mid,     PQP_PLANT_MID_TOL false
//   PQP_PLANT_MID_KERNEL k_plant_roll_mid_tol, PQP_PLANT_MID_TOL true
// ROLL (the argument is then a PlantMidRollArgs): a step loop inside the state loop.  The workgroup carries
// state b through R.K steps on the plant it staged once: step k's prologue reads row k of X and this step's D,
// every start but a cold step 0 is d_Y[b] (floored on load), the results go to row k of the [K][B] arrays and Y
// to d_Y[b], and one wave forms x+ = (A x + Bu U) + Bd D into row k + 1 of X (k_plant_advance's arithmetic, the
// dynamics read through L2) before the barrier that ends the step.  Every ROLL branch is a compile-time one and
// the step loop a do ... while (ROLL && ...), so the step's eight kernels keep their instructions (DESIGN.md 4l).
//
template <int MAXT, bool PAIR, int MINW = 1, bool BAND = true>
__global__ void __launch_bounds__(MAXT, MINW)
PQP_PLANT_MID_KERNEL(std::conditional_t<PQP_PLANT_MID_ROLL, PlantMidRollArgs, PlantMidArgs> A0) {
    extern __shared__ __attribute__((aligned(16))) float lds_raw[];
    if ((int)blockIdx.x >= A0.S.B) return;  // a workgroup without a state (uniform)
    const PlantData& P = A0.P;
    const PlantMidFlags& F = A0.F;
    const int N = P.N, M = P.M, nd = P.nd, ns = P.ns;
    const int front = plant_mid_front(N);
    float* const lds = lds_raw + front;
    const Mid2Layout L = mid2_layout(N, M, true);
    const int ldn = L.ldn, ldm = L.ldm, ldg = L.ldg, ldi = L.ldi, nk = L.nk, mk = L.mk;
    float* Qd = lds + L.Qd;
    float* Gp = lds + L.Gp;
    float* Qi = lds + L.Qi;
    float* Qp = lds + L.Qp;
    float* Yr = lds + L.y;
    float* tq = lds + L.tq;
    float* Fdp = lds + L.Fdp;
    float* Fdn = lds + L.Fdn;
    float* Kp = lds + L.Kp;
    float* tM = lds + L.tM;
    float* Us = lds + L.Us;
    float* tu = lds + L.tu;
    float* fu = lds + L.fu;
    float* Fp = lds + L.Fp;
    float* fdy = lds + L.fdy;
    float* sums = lds + L.sums;
    int* flag = reinterpret_cast<int*>(lds + L.flag);
    int* band = reinterpret_cast<int*>(lds + L.band);
    float* xs = lds_raw + kPmX;
    float* ds = lds_raw + kPmD;
    float* r0s = lds_raw + kPmR0;
    float* r1s = lds_raw + kPmR1;
    float* r3s = lds_raw + kPmR3;
    float* tqp = lds_raw + kPmTq;    // Fp'Qp_inv
    float* dots = lds_raw + kPmDots;  // the five ordered dots that end Mp
    float* scal = fdy + 2;            // [0] Mp, [1] Md: the two words of fdy's four that its ring leaves free
    const int NT = blockDim.x;  // 64 * mid2_waves(N, true, PAIR, 64)
    const int tid = threadIdx.x, lane = tid & 63;
    const int hw = tid >> 6, nW = NT >> 6;  // the hardware wave: the prologue's split
    const int nUW = mid2_uw(N, PAIR), wT = nUW, wC0 = nUW + 1;
    // the roles over the hardware waves, as k_solve_mid2 permutes them
    int wave = hw;
    if constexpr (PQP_M2_PERM && !PAIR && MINW == 1)
        if (NT == 512 && nUW == 3) wave = wave < 2 ? wave + 4 : (wave < 6 ? wave - 2 : wave);
    if constexpr (PQP_M2_PERM4 && PAIR && MINW == 1)
        if (NT == 512 && nUW == 4) {
            wave = wave < 3 ? wave + 5 : (wave == 3 ? 4 : (wave == 4 ? 3 : wave - 5));
        }
    const int crows = (NT / 64 - nUW - 2 >= (N + 31) / 32) ? 32 : 64;
    const int nCR = mid2_cr(N, crows);
    const int wDec = wC0 + nCR;
    const bool tsum = PQP_M2_TSUM && !PAIR && M < 63;
    constexpr bool PK = MINW == 1;
    constexpr int RD = MINW == 1 ? PQP_M2_RING : PQP_M2_RING_LEAN;
    constexpr int RDD = MINW == 1 ? PQP_M2_RINGD : PQP_M2_RINGD_LEAN;
    constexpr bool DEC1 = PQP_M2_DEC1 && PAIR && MINW == 1;
    const bool sym = F.sym != 0, fast = F.fast != 0, qfinite = F.qfinite != 0;

    // ---- once per workgroup: the plant (padding zero) ----
    for (int e = tid; e < front + L.total; e += NT) lds_raw[e] = 0.0f;
    __syncthreads();
    for (int e = tid; e < N * N; e += NT) {
        const int i = e / N, k = e - i * N;
        Qd[i * ldn + k] = P.Qd[e];
    }
    for (int e = tid; e < N * M; e += NT) {
        const int i = e / M, j = e - i * M;
        Gp[j * ldg + i] = P.Gp[e];
    }
    for (int e = tid; e < M * M; e += NT) {
        const int i = e / M, j = e - i * M;
        Qi[i * ldi + j] = P.Qinv[e];
        if (PQP_M2_QPT) Qp[j * ldm + i] = P.Qp[e];
        else Qp[i * ldm + j] = P.Qp[e];
    }
    if (PQP_M2_TSUM)
        for (int k = tid; k < nk; k += NT) lds[L.ones + k] = 1.0f;
    __syncthreads();
    // the band of each row group (mid2_band), which depends on Qd only
    for (int i = tid; i < N; i += NT) {
        const float* row = Qd + i * ldn;
        int lo = i, hi = i;
        for (int k = 0; k < N; ++k) {
            if (row[k] != 0.0f || Qd[k * ldn + i] != 0.0f) {
                lo = k < lo ? k : lo;
                hi = k > hi ? k : hi;
            }
        }
        if (F.dense) {
            lo = 0;
            hi = nk - 1;
        }
        const int lo8 = lo & ~7, hi8 = (hi + 8) & ~7;
        atomicMax(&band[i >> 6], nk - lo8);
        atomicMax(&band[3 + (i >> 6)], hi8);
        if (i < 160) {  // the table's five 32-row groups (read by the lane-side build only, N <= 128)
            atomicMax(&band[6 + (i >> 5)], nk - lo8);
            atomicMax(&band[11 + (i >> 5)], hi8);
        }
    }
    __syncthreads();

    // per-lane constants of the update role that the plant fixes: the row, its
    // diagonal literals (:524-537, Theta precomputed), the masks' base
    const int side = lane & 1;
    const int urow = PAIR ? 32 * wave + (lane >> 1) : 64 * wave + lane;
    const bool uw = wave < nUW && urow < N;
    const float lim = side ? __builtin_inff() : -__builtin_inff();
    float dpr = 0.0f, dnr = 0.0f;
    if (uw) {
        const float th = P.theta[urow], qii = Qd[urow * ldn + urow];
        dpr = max_ref(0.0f, qii) + 1.0f * th;
        dnr = max_ref(0.0f, -qii) + 1.0f * th;
    }
    const float dv = side ? dpr : -dnr;
    const int w0 = __builtin_amdgcn_readfirstlane(PAIR ? 32 * wave : 64 * wave);
    const float Mp6 = P.Mp6[0];
    const int h0 = 1;  // every state starts at h = 1 (cold, or warm as a chunked relaunch does)
    const int nB = A0.S.B;

    for (int b = blockIdx.x; b < nB; b += gridDim.x) {
        // ROLL: the step of state b's trajectory.  Through the phase loop it lies in sums[3], the one word of
        // `sums` that the solve leaves alone, not in a register: the results read it back
        int k = 0;
        do {  // ROLL: state b's K steps; else once (the body keeps the state loop's indentation)
        // ================= the state's prologue =================
        const PlantMidArgsPtr ap = plant_mid_args();
        const auto& P = ap->P;  // (shadow the kernel's: see plant_mid_args)
        const auto& S = ap->S;
        const long long max_updates = S.max_updates;
        if constexpr (PQP_PLANT_MID_ROLL) {  // x: row k of X; D: this step's
            const PlantMidRollArgsPtr ar = plant_mid_roll_args();
            const size_t kb = (size_t)k * ar->S.B + b;
            if (tid < ns) xs[tid] = ar->R.X[kb * ns + tid];
            if (hw == 1 && lane < nd) ds[lane] = S.D[(ar->R.d_steps > 1 ? kb : (size_t)b) * nd + lane];
        } else {
            if (tid < ns) xs[tid] = S.x[(size_t)b * ns + tid];
            if (hw == 1 && lane < nd) ds[lane] = S.D[(size_t)b * nd + lane];
        }
        __syncthreads();
        // computeFp (:373) on wave 0; x'Mp1, D'Mp2 on wave 1, D'Mp3 on wave 2: one lane per column
        if (hw == 0) {
            if (lane < M) {
                float sf2 = 0.0f;
#pragma unroll 8
                for (int k = 0; k < ns; ++k) sf2 += P.Fp2[lane * ns + k] * xs[k];  // Fp2 x
                float sf1 = 0.0f;
#pragma unroll 8
                for (int k = 0; k < nd; ++k) sf1 += P.Fp1[lane * nd + k] * ds[k];  // Fp1 D
                float fp = sf1 + 1.0f * sf2;      // matrixAdd(Fp, Fp, tmp, 1)
                fp = fp + -1.0f * P.Fp3[lane];    // matrixAdd(Fp, Fp, Fp3, -1)
                Fp[lane] = fp;
                if (S.Fp) S.Fp[(size_t)b * M + lane] = fp;
            }
        } else if (hw == 1) {
            if (lane < ns) {
                float r0 = 0.0f, r1 = 0.0f;
#pragma unroll 8
                for (int k = 0; k < ns; ++k) r0 += xs[k] * P.Mp1[k * ns + lane];  // x' Mp1
#pragma unroll 8
                for (int k = 0; k < nd; ++k) r1 += ds[k] * P.Mp2[k * ns + lane];  // D' Mp2
                r0s[lane] = r0;
                r1s[lane] = r1;
            }
        } else if (hw == 2) {
            if (lane < nd) {
                float r3 = 0.0f;
#pragma unroll 8
                for (int k = 0; k < nd; ++k) r3 += ds[k] * P.Mp3[k * nd + lane];  // D' Mp3
                r3s[lane] = r3;
            }
        }
        __syncthreads();
        // Fd = (Gp Qp_inv) Fp + Kp one thread per row (:456-459; tid < N lies in
        // the waves before the last two); Fp'Qp_inv on the last wave, one lane
        // per column; the five ordered dots that end Mp (:397-425) on the wave
        // before it
        if (tid < N) {
            float fd = 0.0f;
#pragma unroll 8
            for (int k = 0; k < M; ++k) fd += P.GQ[tid * M + k] * Fp[k];
            const float kp = S.Kp ? S.Kp[(size_t)b * N + tid] : P.Kp[tid];
            fd = fd + 1.0f * kp;  // matrixAdd(Fd, Fd, Kp, 1) :459
            Fdp[tid] = max_ref(0.0f, fd);   // matrixPos(Fdp, Fd) :703
            Fdn[tid] = max_ref(0.0f, -fd);  // matrixNeg(Fdn, Fd) :704
            Gp[mk * ldg + tid] = fd;        // Fd.Y rides as row mk
            Kp[tid] = kp;
            if (S.Fd) S.Fd[(size_t)b * N + tid] = fd;
        }
        if (hw == nW - 1) {
            if (lane < M) {
                float t = 0.0f;
#pragma unroll 8
                for (int k = 0; k < M; ++k) t += Fp[k] * Qi[k * ldi + lane];
                tqp[lane] = t;
            }
        } else if (hw == nW - 2) {
            if (lane < 5) {
                const float* da = lane == 0 ? r0s : (lane == 1 ? r1s : (lane == 2 ? P.Mp4 : (lane == 3 ? r3s : P.Mp5)));
                const float* db = lane < 3 ? xs : ds;  // (x'Mp1).x, (D'Mp2).x, Mp4'x, (D'Mp3).D, Mp5'D
                const int dlen = lane < 3 ? ns : nd;
                float dot = 0.0f;
#pragma unroll 8
                for (int k = 0; k < dlen; ++k) dot += da[k] * db[k];
                dots[lane] = dot;
            }
        }
        // every other per-state word of the layout, as a fresh workgroup has it (the
        // rings, which the prologue's words lie over, after them)
        for (int e = tid; e < mk; e += NT) {
            tM[e] = 0.0f;
            Us[e] = 0.0f;
            Us[mk + e] = 0.0f;
            tu[e] = 0.0f;
            fu[e] = 0.0f;
        }
        if (tid < 16) flag[tid] = 0;
        if (tid < 4) {
            fdy[tid] = 0.0f;
            sums[tid] = 0.0f;
            // (the four lanes store one value, after lane 3's zero: no lane mask of its own to keep)
            if constexpr (PQP_PLANT_MID_ROLL) reinterpret_cast<int*>(sums)[3] = k;
        }
        __syncthreads();
        // Mp's halved terms in k_mp_finish's order, Md = (Fp'Qp_inv) Fp - Mp (:475-478)
        if (tid == 0) {
            float dot = 0.0f;
            for (int k = 0; k < M; ++k) dot += tqp[k] * Fp[k];
            float mp = 0.0f;
            for (int t = 0; t < 5; ++t) mp += dots[t] / 2;
            mp += Mp6 / 2;
            const float md = dot + -1.0f * mp;  // :478
            scal[0] = mp;
            scal[1] = md;
            if (S.Mp) S.Mp[b] = mp;
            if (S.Md) S.Md[b] = md;
        }
        __syncthreads();  // the prologue's words are dead: the rings, zero but for Y_1
        int ynf = 0;
        // ROLL: every step but a cold step 0 starts from d_Y[b], which the step before stored (a barrier since:
        // one workgroup reads its own global stores), floored on load as k_plant_advance / k_plant_floor floor it
        bool warm_k = false;
        float yfl = 0.0f;
        if constexpr (PQP_PLANT_MID_ROLL) {
            warm_k = k > 0 || S.warm;
            yfl = plant_mid_roll_args()->R.y_floor;
        }
        for (int e = tid; e < 5 * nk; e += NT) {
            const int i = e - (h0 % 3) * nk;
            float y = 0.0f;
            if (i >= 0 && i < N) {
                if constexpr (PQP_PLANT_MID_ROLL) {
                    y = warm_k ? S.Y[(size_t)b * N + i] : 1000.0f;
                    if (warm_k && yfl > 0.0f) y = yfl > y ? yfl : y;  // (a NaN stays)
                } else
                y = S.warm ? S.Y[(size_t)b * N + i] : 1000.0f;  // initMat(Y,1000) :710
                if (!(PQP_M2_PF ? (y >= 0.0f && y <= 3.402823466e38f) : fabsf(y) <= 3.402823466e38f)) ynf = 1;
            }
            Yr[e] = y;  // (the tq ring follows the Y ring)
        }
        bool y_nonfinite = __syncthreads_or(ynf);
        const float Mp = scal[0], Md = scal[1];
        const float fdv = uw ? (side ? Fdp[urow] : Fdn[urow]) : 0.0f;
        const float fdp = uw ? Fdp[urow] : 0.0f, fdn = uw ? Fdn[urow] : 0.0f;

        // ================= the solve: k_solve_mid2's phase loop =================
        float Jp_last = 0.0f, Jd_last = 0.0f;
        bool costs = false;
        int status = kStatusContinue;
        int t_out = h0;
        // after phase s's first barrier: terminate(s-1)'s decision (:673-687)
        auto decide = [&](int s) -> bool {
            if (s == h0) return false;  // nothing pending in the state's first phase
            const int t = s - 1;
            int infeasible = 0;
            for (int c = 0; c < nCR; ++c) infeasible |= flag[c];
            int stop = 0;
            if (!infeasible) {
                float Jd = 0.0f;
                Jd = (float)((double)Jd + 0.5 * (double)sums[0]);
                Jd += fdy[t & 1];
                Jd += Md / 2;
                float Jp = 0.0f;
                Jp = (float)((double)Jp + 0.5 * (double)sums[1]);
                Jp += sums[2];
                Jp += Mp / 2;
                stop = gap_stop(Jp, Jd) ? 1 : 0;  // :683-685
                if constexpr (PQP_PLANT_MID_TOL) {  // then the caller's tolerances (pqp.h 2k), workgroup-uniform
                    const PlantMidArgsPtr at = plant_mid_args();
                    if (!stop) stop = tol_stop(Jp, Jd, at->S.abs_tol, at->S.rel_tol);
                }
                Jp_last = Jp;
                Jd_last = Jd;
                costs = true;
            }
            t_out = t;
            if (stop) { status = PQP_PLANT_MID_TOL ? stop : kStatusDone; return true; }  // (kStatusDone or kStatusTol)
            if ((long long)(t - 1) >= max_updates) { status = kStatusCapped; return true; }
            return false;
        };
        // the phase's end: two barriers; between them the decision (DEC1: on the
        // cost wave alone, posted in flag[14] / flag[15]) and Y_{s+1}'s flag
        auto phase_end = [&](int s) -> bool {
            __syncthreads();
            bool leave;
            if (DEC1) {
                if (wave == wDec) {
                    const bool d = decide(s);
                    if (lane == 0) {
                        flag[14] = d ? 1 : 0;
                        flag[15] = t_out - h0;
                    }
                }
                y_nonfinite = flag[12 + ((s + 1) & 1)] != 0;
                __syncthreads();
                leave = flag[14] != 0;
                if (leave) t_out = h0 + flag[15];
            } else {
                leave = decide(s);
                y_nonfinite = flag[12 + ((s + 1) & 1)] != 0;
                __syncthreads();
            }
            return leave;
        };

        if (wave < nUW) {
            // ---------------- UW: Y_{s+1} = updateY2(Y_s) ----------------
            const float* q = Qd + (uw ? urow : 0) * ldn;
            const int bg = PAIR ? 6 + wave : wave;
            const int blo = BAND ? __builtin_amdgcn_readfirstlane(nk - band[bg]) : 0;
            const int bhi = BAND ? __builtin_amdgcn_readfirstlane(band[bg + (PAIR ? 5 : 3)]) : nk;
            for (int s = h0;; ++s) {
                const float* ycur = Yr + (s % 3) * nk;
                float* ynext = Yr + ((s + 1) % 3) * nk;
                if (wave == 0 && lane == 0) flag[12 + (s & 1)] = 0;
                const int klo = (BAND && !y_nonfinite) ? blo : 0, khi = (BAND && !y_nonfinite) ? bhi : nk;
                if (uw) {
                    if constexpr (PAIR) {
                        float acc = (fast && !y_nonfinite) ? mid2_side<true>(q, ycur, klo, khi, urow, side, lim, dv, w0)
                                                           : mid2_side<false>(q, ycur, klo, khi, urow, side, lim, side ? dv : -dv, w0);
                        if (fast && !y_nonfinite && !side) acc = 0.0f - acc;  // num's terms were summed negated
                        const float v = acc + 1.0f * fdv;                     // num += Fdn :611; den += Fdp :612
                        const float other = __shfl_xor(v, 1);
                        if (side) {
                            const float y = ycur[urow];
                            const float yn = other / v * y;  // updY :594
                            ynext[urow] = yn;
                            if (!(PQP_M2_PF ? (yn >= 0.0f && yn <= 3.402823466e38f) : fabsf(yn) <= 3.402823466e38f))
                                flag[12 + ((s + 1) & 1)] = 1;
                        }
                    } else {
                        float yn;
                        if (PQP_M2_PF && MINW == 1 && qfinite && !y_nonfinite)
                            yn = mid2_row<true, MINW == 1, PQP_M2_PF && MINW == 1>(q, ycur, klo, khi, urow, dpr, dnr, fdn, fdp, w0);
                        else if (fast)
                            yn = mid2_row<true, MINW == 1>(q, ycur, klo, khi, urow, dpr, dnr, fdn, fdp, w0);
                        else
                            yn = mid2_row<false, MINW == 1>(q, ycur, klo, khi, urow, dpr, dnr, fdn, fdp, w0);
                        ynext[urow] = yn;
                        if (!(PQP_M2_PF ? (yn >= 0.0f && yn <= 3.402823466e38f) : fabsf(yn) <= 3.402823466e38f))
                            flag[12 + ((s + 1) & 1)] = 1;
                    }
                }
                if (phase_end(s)) break;
            }
        } else if (wave == wT) {
            // ------------- T: tM = Gp'Y_s + Fp, Fd.Y_s, U_s = -Qp_inv tM -------------
            const float* grow = Gp + (lane < M ? lane : mk) * ldg;
            const float* qirow = Qi + (lane < M ? lane : 0) * ldi;
            const float fpl = lane < M ? Fp[lane] : 0.0f;
            const bool l63 = tsum && lane == 63;
            for (int s = h0;; ++s) {
                const float* ycur = Yr + (s % 3) * nk;
                if (lane <= M || l63) {
                    const float d = m2_dot_row<PK && PQP_M2PK_T, RD>(l63 ? tq + ((s - 1) & 1) * nk : grow,
                                                                     l63 ? lds + L.ones : ycur, nk);
                    if (lane < M) tM[lane] = d + 1.0f * fpl;  // :355-356
                    else if (lane == M) fdy[s & 1] = d;       // Fd.Y :656
                    else sums[0] = d;                         // (Y'Qd).Y of iterate s-1
                }
                __builtin_amdgcn_wave_barrier();
                if (lane < M) Us[(s & 1) * mk + lane] = -m2_dot_row<PK && PQP_M2PK_T, RD>(qirow, tM, mk);  // :357-358
                if (phase_end(s)) break;
            }
        } else {
            // ---------------- C: terminate(Y_{s-1}); Y_s'Qd ----------------
            const int cw = wave - wC0;
            const int cg = cw < nCR ? (crows == 64 ? cw : 6 + cw) : 0;
            const int clo = BAND ? __builtin_amdgcn_readfirstlane(nk - band[cg]) : 0;
            const int chi = BAND ? __builtin_amdgcn_readfirstlane(band[cg + (crows == 64 ? 3 : 5)]) : nk;
            for (int s = h0;; ++s) {
                const float* ycur = Yr + (s % 3) * nk;
                const bool pend = s > h0;
                const float* Uo = Us + ((s - 1) & 1) * mk;
                if (cw < nCR) {
                    const int l = cw * crows + lane;
                    const int lend = lane < crows ? N : 0;
                    int bad = 0;
                    if (pend)
                        for (int i = l; i < lend; i += crows * nCR) {
                            const float g = m2_dot<PK && PQP_M2PK_F, RDD>(Gp + i, ldg, Uo, mk);  // row i of Gp . U  :636
                            const float kp = Kp[i];
                            if (g > kp + max_ref((float)(kTol * kp), (float)kTol)) bad = 1;  // compare :338
                        }
                    const bool any_bad = __any(bad);
                    if (pend && lane == 0) flag[cw] = any_bad ? 1 : 0;
                    float* tqs = tq + (s & 1) * nk;  // for terminate(s), next phase
                    const bool cb = BAND && !y_nonfinite;
                    const int klo = cb ? clo : 0, kn = (cb ? chi : nk) - klo;
                    for (int j = l; j < lend; j += crows * nCR)
                        tqs[j] = (sym ? m2_dot_row<PK && PQP_M2PK_C, RD>(Qd + j * ldn + klo, ycur + klo, kn)
                                      : m2_dot<PK && PQP_M2PK_C, RDD>(Qd + klo * ldn + j, ldn, ycur + klo, kn)) * ycur[j];
                } else if (pend && cw == nCR) {
                    if (lane < M) {
                        tu[lane] = (PQP_M2_QPT ? m2_dot_row<PK && PQP_M2PK_Q, RD>(Qp + lane * ldm, Uo, mk)
                                               : m2_dot<PK && PQP_M2PK_Q, RDD>(Qp + lane, ldm, Uo, mk)) *
                                   Uo[lane];  // (U'Qp).U terms :652-655
                        fu[lane] = Fp[lane] * Uo[lane];  // Fp'U :656-657
                    }
                    __builtin_amdgcn_wave_barrier();
                    if (lane < 3 && !(tsum && lane == 0)) {
                        const float* v = lane == 0 ? tq + ((s - 1) & 1) * nk : (lane == 1 ? tu : fu);
                        const float r = m2_sum<RD>(v, lane == 0 ? nk : mk);
                        sums[lane] = r;
                    }
                }
                if (phase_end(s)) break;
            }
        }
        // ================= the state's results =================
        {
            const PlantMidArgsPtr ao = plant_mid_args();
            const auto& S = ao->S;
            const float* yo = Yr + (t_out % 3) * nk;
            for (int i = tid; i < N; i += NT) S.Y[(size_t)b * N + i] = yo[i];
            if constexpr (PQP_PLANT_MID_ROLL) {
                // ---- the step's results in row k of the [K][B] arrays; then x+ into row k + 1 of X ----
                k = __builtin_amdgcn_readfirstlane(reinterpret_cast<const int*>(sums)[3]);
                const size_t kb = (size_t)k * S.B + b;
                for (int i = tid; i < M; i += NT) S.U[kb * M + i] = Us[(t_out & 1) * mk + i];
                if (DEC1 ? (wave == wDec && lane == 0) : tid == 0) {
                    if (S.h) S.h[kb] = t_out;
                    if (S.status) S.status[kb] = status;
                    if (S.Jp) S.Jp[kb] = costs ? Jp_last : __builtin_nanf("");
                    if (S.Jd) S.Jd[kb] = costs ? Jd_last : __builtin_nanf("");
                }
                // x+ = (A x + 1 Bu U) + 1 Bd D on the first wave, k_plant_advance's sums: one lane per row, every
                // sum from +0.0f in index order, every product rounded before its add.  x (row k of X: the LDS copy
                // is dead), D and U (the ring slot stored above) one word per lane, handed round the wave; AT, BuT,
                // BdT k-major from memory, consecutive over the lanes, eight rows loaded ahead of their adds.  The
                // thread number and the sizes come from opaque copies, as k_plant_step's ROLL form takes them: no
                // lane mask or per-lane address of this block is formed before the phase loop and held through it
                int t2 = tid;
                asm volatile("" : "+v"(t2));
                if (t2 < 64) {
                    const PlantMidRollArgsPtr ar = plant_mid_roll_args();
                    const auto& R = ar->R;
                    const int ns2 = ar->P.ns, nd2 = ar->P.nd, M2 = ar->P.M;
                    const float xl = t2 < ns2 ? R.X[kb * ns2 + t2] : 0.0f;
                    const float dl = t2 < nd2 ? S.D[(R.d_steps > 1 ? kb : (size_t)b) * nd2 + t2] : 0.0f;
                    const float ul = t2 < M2 ? Us[(t_out & 1) * mk + t2] : 0.0f;
                    const int pr = t2 < ns2 ? t2 : 0;
                    const float t = plant_mid_dot_lanes(R.dyn.AT, ns2, pr, ns2, xl);
                    const float v = plant_mid_dot_lanes(R.dyn.BuT, ns2, pr, M2, ul);
                    const float w = plant_mid_dot_lanes(R.dyn.BdT, ns2, pr, nd2, dl);
                    float xn = t + 1.0f * v;
                    xn = xn + 1.0f * w;
                    if (t2 < ns2) R.X[(kb + S.B) * ns2 + t2] = xn;
                }
            } else {
            for (int i = tid; i < M; i += NT) S.U[(size_t)b * M + i] = Us[(t_out & 1) * mk + i];
            if (DEC1 ? (wave == wDec && lane == 0) : tid == 0) {  // a thread that took the decisions
                if (S.h) S.h[b] = t_out;
                if (S.status) S.status[b] = status;
                if (S.Jp) S.Jp[b] = costs ? Jp_last : __builtin_nanf("");
                if (S.Jd) S.Jd[b] = costs ? Jd_last : __builtin_nanf("");
            }
            }
        }
        __syncthreads();  // the next state's (ROLL: step's) stores and loads come after this one's reads and stores
        } while (PQP_PLANT_MID_ROLL && ++k < plant_mid_roll_args()->R.K);
    }
}
