/*
 * include/pqp.h -- C ABI of libpqp (pqp-for-mpc_amd), the MI355X-native
 * drop-in for the PQP dual-update hot path of yashsoni501/PQP-for-MPC.
 *
 * Two layers:
 *
 *  1. Drop-in entry points.  Same names, argument order and meaning as the
 *     reference's C functions (PQP_CPU.c), on caller-owned HOST buffers of
 *     row-major fp32.  They run on the GPU (HIP, gfx950) and return results
 *     identical to PQP_CPU.c.  Like the reference they have no status return;
 *     on a HIP/allocation failure they print a message and exit(EXIT_FAILURE)
 *     (the reference's own failure behaviour, PQP_GPU_optimized.cu:83-89).
 *
 *  2. pqp_* entry points.  Status-returning (PQP_OK or a negative PQP_ERR_*;
 *     pqp_last_error() explains), explicit sizes, and the batched device API
 *     that works on DEVICE pointers on the caller's hipStream_t (passed as
 *     void*).  Nothing here takes framework types.
 *
 * Device layout of a batch of B dual problems of size N:
 *   QdT   [B][N][ldq]  Qd stored column-major per instance: element (i,k)
 *                      of Qd is QdT[b*qstride + k*ldq + i]; ldq >= N, ldq % 4 == 0
 *   theta, Fd, Y       [B][ldv] fp32 vectors, ldv >= N
 *
 * Padding belongs to the caller.  The layout has three kinds of it: rows
 * N..ldq-1 of each column k < N, the stride gap [N*ldq, qstride) after each
 * problem (qstride >= N*ldq, qstride % 4 == 0), and the vector tails [N, ldv)
 * (no alignment rule on ldv: an odd one is fine).  None of them is ever read
 * into a result -- they may hold anything, NaN included -- and none is
 * written, with two exceptions: pqp_batch_generate and pqp_batch_pack store +0
 * in the padded rows, and pqp_batch_generate stores +0 in Fd's tail.  d_Y0 of
 * pqp_batch_iterate may be NULL, a separate buffer, or d_Y itself
 * (tests/test_gpu_layout.py pins all of this).
 */
#ifndef PQP_H
#define PQP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PQP_OK 0
#define PQP_ERR_ARG (-1)           /* bad size / pointer / layout                 */
#define PQP_ERR_HIP (-2)           /* a HIP runtime call or kernel launch failed  */
#define PQP_ERR_ALLOC (-3)         /* device allocation failed                    */
#define PQP_ERR_IO (-4)            /* input file missing or short                 */
#define PQP_ERR_NOT_CONVERGED (-5) /* converge mode hit its update cap            */
#define PQP_ERR_NO_DEVICE (-6)     /* no gfx950 device visible                    */
#define PQP_ERR_NEEDS_QDT (-7)     /* pqp_batch_prepare: pass d_QdT (see there)   */

/* Solve modes of pqp_solve_dual. */
#define PQP_MODE_CONVERGE 0 /* while(!terminate(Y)) update  (PQP_CPU.c:718)            */
#define PQP_MODE_FIXED 1    /* while(h < num_iter) update   (testing/ harness, no terminate) */

const char *pqp_last_error(void);
int pqp_version(void);

/* ======================================================================
 * 1. Drop-in entry points (reference signatures, host pointers)
 * ==================================================================== */

/* PQP_CPU.c:694-750.  Runs the whole solve on the GPU in one persistent
 * workgroup (setup, terminate() before every update, updateY2) and prints
 * "Printing number of iterations = %ld\n" exactly as the reference does.
 * Y (N) and U (M) are outputs; the rest are inputs. */
void solveQuadraticDual(float *Y, float *Qd, float *Fd, float *Md, float *U, float *Qp, float *Qp_inv,
                        float *Fp, float *Mp, float *Gp, float *Kp, int N, int M);

/* PQP_CPU.c:603-618.  One multiplicative update from the stored split
 * matrices Qdp_theta = max(0,Qd)+Theta, Qdn_theta = max(0,-Qd)+Theta and
 * Fdp = max(0,Fd), Fdn = max(0,-Fd).  Fd is accepted and unused, as in the
 * reference. */
void updateY2(float *Y_next, float *Y, float *Qdp_theta, float *Qdn_theta, float *Fd, float *Fdp,
              float *Fdn, int N);

/* PQP_CPU.c:673-687.  Writes U = -Qp_inv(Gp'Y + Fp) and returns 1 when the
 * feasibility and duality-gap tests all pass. */
int terminate(float *Y, float *Qd, float *Fd, float *Md, float *U, float *Qp, float *Qp_inv, float *Fp,
              float *Mp, float *Gp, float *Kp, int N, int M);

/* PQP_CPU.c:489-498: Qd = (Gp Qp_inv) Gp', Fd = (Gp Qp_inv) Fp + Kp,
 * Md = (Fp' Qp_inv) Fp - Mp.
 * NaN operands: where an operand is NaN, the output is NaN wherever the
 * reference's is, but the NaN's sign and payload may differ (the host's and the
 * GPU's multiply carry a NaN operand's bits differently); every non-NaN output
 * is bit-identical.  DESIGN.md section 2. */
void convertToDual(float *Qd, float *Fd, float *Md, float *Qp_inv, float *Gp, float *Kp, float *Fp,
                   float *Mp, int N, int M);

/* PQP_CPU.c:352-360: U = -Qp_inv (Gp'Y + Fp). */
void computeUfromY(float *U, float *Y, float *Fp, float *Gp, float *Qp_inv, int N, int M);

/* PQP_CPU.c:648-666: J = 0.5 (Z'Q) Z + F'Z + M[0]/2. */
float computeCost(float *Z, float *Q, float *F, float *M, int N);

/* PQP_CPU.c:632-641: 1 iff Gp U <= Kp + max(1e-6 Kp, 1e-6) element-wise. */
int checkFeas(float *U, float *Gp, float *Kp, int N, int M);

/* PQP_CPU.c:503-519: theta (N x N, caller-zeroed as in the reference) gets
 * theta[i][i] = max(sum_j max(0,-Qd[i][j]), 5); other entries untouched. */
void computeTheta(float *theta, float *Qd, int N);

/* PQP_CPU.c:84-147: output[a x c] = op(mat1)[a x b] * op(mat2)[b x c];
 * output may alias an input.
 * NaN operands: where an operand is NaN, the output is NaN wherever the
 * reference's is, but the NaN's sign and payload may differ (the host's and the
 * GPU's multiply carry a NaN operand's bits differently); every non-NaN output
 * is bit-identical.  DESIGN.md section 2. */
void matrixMultiply(float *output, float *mat1, int transpose1, float *mat2, int transpose2, int a, int b,
                    int c);

/* PQP_CPU.c:251-326: res = inverse(A) by the reference's Gauss-Jordan
 * (one bubble pass on column 0, no pivoting). */
void Gauss_Jordan(float *A, float *res, int N);

/* PQP_CPU.c:373-382 / 395-428, with the reference's compile-time problem
 * dimensions (pHorizon=1, nState=29, nInput=7, nDis=1; PQP_CPU.c:13-17). */
void computeFp(float *Fp, float *Fp1, float *Fp2, float *Fp3, float *D, float *x);
void computeMp(float *Mp, float *Mp1, float *Mp2, float *Mp3, float *Mp4, float *Mp5, float *Mp6, float *D,
               float *x);

/* PQP_CPU.c:757-930: reads ./example/{Qp_inv,Fp1,Fp2,Fp3,Mp1..Mp6,Gp,Kp,Z,Theta,D,x}.txt
 * relative to the current directory, with the reference's transposed
 * layout and compile-time dimensions.  (Host I/O; no GPU work.) */
void input(float *qp_inv, float *Fp1, float *Fp2, float *Fp3, float *Mp1, float *Mp2, float *Mp3, float *Mp4,
           float *Mp5, float *Mp6, float *Gp, float *Kp, float *x, float *D, float *theta, float *Z);

/* ======================================================================
 * 2a. Status-returning host-pointer API
 * ==================================================================== */

/* solveQuadraticDual without the printf and with explicit control:
 *   mode PQP_MODE_CONVERGE: iterate until terminate() passes; gives up with
 *     PQP_ERR_NOT_CONVERGED after max_updates updates (<= 0: no cap).
 *   mode PQP_MODE_FIXED: num_iter-1 updates, no terminate (testing/ harness).
 * On return *h_out is the reference's printed h (updates + 1), Y and U hold
 * the final iterate, Jp_out and Jd_out get the costs of the last terminate() that
 * got past the feasibility test (NaN if none).  Any of the out pointers
 * except Y may be NULL. */
int pqp_solve_dual(const float *Qd, const float *Fd, const float *Md, const float *Qp, const float *Qp_inv,
                   const float *Fp, const float *Mp, const float *Gp, const float *Kp, int N, int M, int mode,
                   long long num_iter, long long max_updates, float *Y, float *U, long long *h_out,
                   float *Jp_out, float *Jd_out);

/* A dual problem resident in HBM: upload and prepare once, then solve any
 * number of times (each solve restarts from Y = 1000).  Same semantics and
 * outputs as pqp_solve_dual, which is create + solve + destroy.  Problems
 * that fit LDS run in one persistent workgroup; larger ones (N up to 38016)
 * run over many workgroups, each solve replaying a captured hipGraph.  The
 * terminate() drop-in also needs the one-workgroup solver, which limits it
 * to 12N + 12M bytes <= 150 KiB. */
typedef struct pqp_problem pqp_problem;
int pqp_problem_create(const float *Qd, const float *Fd, const float *Md, const float *Qp, const float *Qp_inv,
                       const float *Fp, const float *Mp, const float *Gp, const float *Kp, int N, int M,
                       pqp_problem **out);
/* The same on an explicit device (-1: the calling thread's current one) and
 * stream (a hipStream_t of that device; NULL: the handle creates and owns
 * one).  A handle is bound to its device and stream: every call on it runs
 * there, whatever device the calling thread has current, and restores the
 * caller's device before returning.  Calls on one handle are serialized by a
 * lock of that handle; different handles (one host thread per GPU, or several
 * per GPU) run concurrently -- the reference's solver keeps no globals
 * (PQP_CPU.c:694) and neither does this one. */
int pqp_problem_create_on(int device, void *stream, const float *Qd, const float *Fd, const float *Md,
                          const float *Qp, const float *Qp_inv, const float *Fp, const float *Mp, const float *Gp,
                          const float *Kp, int N, int M, pqp_problem **out);
/* The device a handle is bound to. */
int pqp_problem_device(const pqp_problem *p);
int pqp_problem_solve(pqp_problem *p, int mode, long long num_iter, long long max_updates, float *Y, float *U,
                      long long *h_out, float *Jp_out, float *Jd_out);
int pqp_problem_destroy(pqp_problem *p);

/* One update on host buffers from Qd/theta-diag/Fd (the fused form used by
 * the solver: Qd+-, Theta and Fd+- derived on the fly). */
int pqp_update_host(const float *Qd, const float *theta_diag, const float *Fd, const float *Y, float *Y_next,
                    int N);

/* Bundled-example reader with explicit dimensions: m = nInput*pHorizon,
 * nd = nDis*pHorizon, ns = nState, N = 4m.  Files are read from `dir`. */
int pqp_read_example(const char *dir, int m, int nd, int ns, float *Qp_inv, float *Fp1, float *Fp2,
                     float *Fp3, float *Mp1, float *Mp2, float *Mp3, float *Mp4, float *Mp5, float *Mp6,
                     float *Gp, float *Kp, float *x, float *D);

/* The testing/ sample-test format ("testing/sample test/test*.txt"; reader at
 * testing/GPU unoptimized version/PQP_GPU_unoptimized.cu:751-794 and
 * testing/CPU version/PQP_CPU_test.c:936-978): header "M N", M diagonal
 * entries of Qp_inv, M of Fp, Mp, N of Kp, N x M integers for Gp mapped by C's
 * `v % 3` (0 -> 0, 2 -> -1, otherwise +1, so a file -1 becomes +1).  With
 * glibc_kp != 0 the file's Kp is replaced, as the harness does, by
 * fabs(10.0*rand()/RAND_MAX) from glibc's unseeded rand() sequence.
 * Call with NULL arrays to get (*M_out, *N_out) first; then call again with the
 * arrays (Qp_inv is M x M dense) and *M_out / *N_out still holding those
 * dimensions: a file whose header no longer matches them gives PQP_ERR_IO and
 * nothing is written.  Headers beyond M, N <= 65536 (or N*M + M*M > 2^30) are
 * rejected with PQP_ERR_IO.  (Host I/O; no GPU work.) */
int pqp_read_testfile(const char *path, int glibc_kp, int *M_out, int *N_out, float *Qp_inv, float *Fp, float *Mp,
                      float *Gp, float *Kp);

/* main() of PQP_CPU.c:935-1013 on the GPU: read `dir`, build the dual, solve,
 * recompute U, print the reference's stdout to `out` (a FILE*; NULL = stdout). */
int pqp_run_example(const char *dir, void *out);

/* ======================================================================
 * 2b. Batched device API (device pointers, caller's stream; async)
 * ==================================================================== */

/* Synthetic dual problems: instance b of the batch is problem
 * number inst0+b of `seed`; primal Qp_inv = diag(0.1+u), Gp in {-1,0,1},
 * Kp = 10u, Fp = 20u-10, Mp = 1, converted to the dual with
 * convertToDual's exact arithmetic.  Writes QdT (column-major, padded rows
 * zeroed), Fd, Md (may be NULL) and theta.  Of the padding it writes +0 into
 * the padded rows N..ldq-1 of QdT and into Fd's tail [N, ldv); the stride gap
 * [N*ldq, qstride) and theta's tail [N, ldv) are left as the caller had them. */
int pqp_batch_generate(uint32_t seed, long long inst0, int B, int N, int M, float *d_QdT, int ldq,
                       long long qstride, float *d_Fd, float *d_Md, float *d_theta, int ldv, void *stream);

/* The primal problems behind pqp_batch_generate's duals, in the layout of
 * 2c below: Qp_inv [B][M*M] (diagonal), Gp [B][N*M], Kp [B][N], Fp [B][M],
 * Mp [B] (= 1).  With pqp_batch_gauss_jordan and pqp_batch_convert_to_dual
 * this gives complete problems for converge-mode solves. */
int pqp_batch_synth_primal(uint32_t seed, long long inst0, int B, int N, int M, float *d_Qp_inv, float *d_Gp,
                           float *d_Kp, float *d_Fp, float *d_Mp, void *stream);

/* Pack B row-major N x N Qd matrices (device, contiguous) into QdT layout. */
int pqp_batch_pack(int B, int N, const float *d_Qd, float *d_QdT, int ldq, long long qstride, void *stream);

/* theta[b][i] = max(sum_j max(0,-Qd_b[i][j]), 5)  (computeTheta). */
int pqp_batch_theta(int B, int N, const float *d_QdT, int ldq, long long qstride, float *d_theta, int ldv,
                    void *stream);

/* One updateY2 for every instance: Y_next = num/den * Y. */
int pqp_batch_update(int B, int N, const float *d_QdT, int ldq, long long qstride, const float *d_theta,
                     const float *d_Fd, int ldv, const float *d_Y, float *d_Ynext, void *stream);

/* `updates` consecutive updateY2 per instance in ONE launch, the iterate
 * resident in LDS (fixed-iteration mode).  d_Y0 == NULL starts from the
 * reference's Y = 1000.  Requires 8*ldq bytes of LDS (ldq <= 20480). */
int pqp_batch_iterate(int B, int N, const float *d_QdT, int ldq, long long qstride, const float *d_theta,
                      const float *d_Fd, int ldv, const float *d_Y0, float *d_Y, int updates, void *stream);

/* Per-problem bit-symmetry of Qd in the QdT layout: d_sym[b] (device, [B]; may
 * be NULL) is nonzero iff Qd_b(i,k) and Qd_b(k,i) hold the same bits for all
 * i, k < N (+0 and -0 differ; a NaN equals itself only with the same payload).
 * *all_sym_out = 1 iff every problem is symmetric.  Reads entries i, k < N
 * only: never the padded rows or the stride gap.  Synchronises `stream` (the
 * flag comes back to the host), as pqp_batch_prepare does. */
int pqp_batch_symmetric(int B, int N, const float *d_QdT, int ldq, long long qstride, int *d_sym, int *all_sym_out,
                        void *stream);

/* pqp_batch_iterate for a batch in which EVERY Qd is bit-symmetric (the
 * caller's contract: pqp_batch_symmetric's all_sym_out, which holds for
 * pqp_batch_generate and for convertToDual with a diagonal Qp_inv).  Same
 * arguments, same d_Y0 rules (NULL, a separate buffer, or d_Y itself), same
 * bits.  At N == ldq == 1024 each 64 x 64 tile of Qd is read from HBM once
 * for itself and its mirror (k_batch_half; a tile off the diagonal is summed
 * in a cheaper form while its entries and the iterate's entries it meets are
 * finite and the latter non-negative, which the kernel tests itself: the bits
 * do not depend on it); other shapes, and the tuning knob iterate_half = 0,
 * forward to pqp_batch_iterate.  With a Qd that is not
 * symmetric the result is that of the matrix whose upper triangle mirrors the
 * stored lower one in some tiles: wrong, but nothing is read out of bounds. */
int pqp_batch_iterate_sym(int B, int N, const float *d_QdT, int ldq, long long qstride, const float *d_theta,
                          const float *d_Fd, int ldv, const float *d_Y0, float *d_Y, int updates, void *stream);

/* ----------------------------------------------------------------------
 * 2b'. B states of ONE dual problem: Qd and theta shared, Fd and Y per state
 * (the MPC workload: one plant at B states).  One Qd is read once per
 * pqp_batch_shared_states states instead of once per state, and it stays in
 * cache: no [B][N][ldq] copies, no HBM stream (k_batch_shared).
 * -------------------------------------------------------------------- */

/* States per workgroup the shared update uses for this shape; 0 when the shape is
 * not supported (no error set).  Depends on (N, ldq) only: 16 up to ldq = 1280,
 * 8 up to ldq = 2560 (two LDS images of the states' iterates, 160 KiB), else 0. */
int pqp_batch_shared_states(int N, int ldq);

/* pqp_batch_iterate for B states of ONE dual problem: d_QdT [N][ldq] and d_theta [N]
 * are one problem's (2b's layout with B = 1: ldq >= N, ldq % 4 == 0, 16-byte aligned);
 * d_Fd, d_Y0, d_Y are [B][ldv], ldv >= N.  State b gets, bit for bit, what
 * pqp_batch_iterate gives problem b of a batch whose every problem holds this Qd and
 * theta.  d_Y0 NULL (Y = 1000), a separate buffer, or d_Y itself.  updates >= 0
 * (0 copies Y0, or 1000, to Y).  One launch (per 256 updates, as pqp_batch_iterate),
 * asynchronous on `stream`, no allocation, no synchronisation.  Qd need not be
 * symmetric.  Padding as in 2b: rows N..ldq-1 of each column and the vector tails
 * [N, ldv) are never read into a result and never written.  NaN operands: the
 * output is NaN wherever pqp_batch_iterate's is (sign and payload may differ) and
 * every non-NaN output is bit-identical.  Argument errors give PQP_ERR_ARG before
 * any device is looked for; a shape with pqp_batch_shared_states(N, ldq) == 0 is
 * one of them. */
int pqp_batch_iterate_shared(int B, int N, const float *d_QdT, int ldq, const float *d_theta,
                             const float *d_Fd, int ldv, const float *d_Y0, float *d_Y,
                             int updates, void *stream);

/* ----------------------------------------------------------------------
 * 2c. Batched small problems: many independent MPC problems (batched
 * horizons / states), one workgroup each.  Every array holds B problems back
 * to back in the reference's row-major layout (e.g. Qd is [B][N*N], Kp is
 * [B][N], Md is [B]).  Synchronous: returns when every problem has finished.
 * -------------------------------------------------------------------- */

/* Gauss_Jordan (PQP_CPU.c:251-326) on B n x n matrices. */
int pqp_batch_gauss_jordan(int B, int n, const float *d_A, float *d_res, void *stream);

/* convertToDual (PQP_CPU.c:489-498) on B primal problems (NaN operands: as
 * convertToDual above). */
int pqp_batch_convert_to_dual(int B, int N, int M, const float *d_Qp_inv, const float *d_Gp, const float *d_Kp,
                              const float *d_Fp, const float *d_Mp, float *d_Qd, float *d_Fd, float *d_Md,
                              void *stream);

/* pqp_batch_convert_to_dual keeps ONE grow-only device workspace per device
 * (4*(B*N*M + B*M) bytes at its largest call: 128 MiB at B = 64, N = 1024,
 * M = 512), shared by every calling thread (calls on one device take turns
 * while they use it).  This frees every device's workspace; the next call
 * allocates again; a setup call in progress finishes first. */
int pqp_release_workspaces(void);

/* computeFp / computeMp (PQP_CPU.c:373-428) for B (D, x) pairs of one plant:
 * m = nInput*pHorizon, nd = nDis*pHorizon, ns = nState.  The plant matrices
 * (Fp1 [m*nd], Fp2 [m*ns], Fp3 [m], Mp1 [ns*ns], Mp2 [nd*ns], Mp3 [nd*nd],
 * Mp4 [ns], Mp5 [nd], Mp6 [1]) are shared; D is [B][nd], x is [B][ns]. */
int pqp_batch_compute_fp(int B, int m, int nd, int ns, const float *d_Fp1, const float *d_Fp2, const float *d_Fp3,
                         const float *d_D, const float *d_x, float *d_Fp, void *stream);
int pqp_batch_compute_mp(int B, int nd, int ns, const float *d_Mp1, const float *d_Mp2, const float *d_Mp3,
                         const float *d_Mp4, const float *d_Mp5, const float *d_Mp6, const float *d_D,
                         const float *d_x, float *d_Mp, void *stream);

/* solveQuadraticDual for B problems at once (converge or fixed mode, as
 * pqp_solve_dual).  Outputs: Y [B][N], U [B][M] (converge mode), h [B]
 * (int64, the reference's printed h) and status [B] (1 converged / done,
 * 2 hit max_updates); h and status may be NULL. */
int pqp_batch_solve(int B, int N, int M, const float *d_Qd, const float *d_Fd, const float *d_Md, const float *d_Qp,
                    const float *d_Qp_inv, const float *d_Fp, const float *d_Mp, const float *d_Gp, const float *d_Kp,
                    int mode, long long num_iter, long long max_updates, float *d_Y, float *d_U, long long *d_h,
                    int *d_status, void *stream);

/* Which batched solver pqp_batch_solve uses for (N, M): 0 one wave or one small
 * workgroup per problem (N, M <= 32), 3 one workgroup per problem with each
 * matrix held in LDS once (k_solve_mid: mid-size, about N <= 165 at M = N/4),
 * 1 the problem staged in LDS with its split copies (k_solve_small; only with
 * the mid_off knob), 2 one workgroup per problem from HBM (uses
 * pqp_batch_prepare's data: k_solve_pipe, which reads every matrix once per
 * iteration, in converge mode when d_QinvT is given, N, M are multiples of 4
 * and M >= N/3; k_solve_single otherwise), or PQP_ERR_ARG when (N, M) exceeds every
 * solver's LDS budget. */
int pqp_batch_solve_path(int N, int M);

/* Path 2's converge-mode kernel for (N, M), from the shape alone: 1 when
 * pqp_batch_solve_prepared (given d_QinvT and 16-byte-aligned arrays) runs
 * k_solve_pipe, which never reads d_GpT -- so a caller need not allocate it
 * (B*N*M floats) -- and 0 when it runs k_solve_single (d_GpT, when given, makes
 * its walks of Gp coalesced); 0 as well for the other paths.  Tuning knobs
 * (pipe_off, pipe_force) move the answer. */
int pqp_batch_solve_kernel(int N, int M);

/* pqp_batch_solve in two steps, so that what depends only on the problems is
 * computed once per batch instead of once per call (path 2 above):
 *   pqp_batch_prepare: per-problem bit-symmetry flags of Qd into d_sym [B]
 *     (int), Theta (computeTheta, PQP_CPU.c:503-519) into d_theta [B][N], and
 *     *all_sym_out = 1 when every Qd is bit-symmetric and N % 4 == 0 (Qd is
 *     then its own column-major copy).  Otherwise the column-major copy goes to
 *     d_QdT [B][N][round4(N)], which must then be given: with d_QdT NULL the
 *     call returns PQP_ERR_NEEDS_QDT with *all_sym_out = 0 (d_sym filled) --
 *     call again with it.  Optional d_GpT [B][M][N] and d_QinvT [B][M][M] (with
 *     d_Gp / d_Qp_inv) receive transposed copies: terminate()'s row walks of
 *     Gp and Qp_inv (PQP_CPU.c:357, :635) then read coalesced.  k_solve_pipe
 *     needs d_QinvT only (it walks Gp's rows from LDS tiles); d_GpT serves
 *     k_solve_single.
 *   pqp_batch_solve_prepared: pqp_batch_solve on those (d_QdT NULL when
 *     *all_sym_out was 1; d_GpT / d_QinvT NULL when not prepared).  The
 *     prepared data stay valid until Qd (or Gp, Qp_inv) change.
 * Paths 0 and 1 need none of it (NULLs are fine there). */
int pqp_batch_prepare(int B, int N, int M, const float *d_Qd, const float *d_Gp, const float *d_Qp_inv, float *d_QdT,
                      float *d_theta, int *d_sym, float *d_GpT, float *d_QinvT, int *all_sym_out, void *stream);
int pqp_batch_solve_prepared(int B, int N, int M, const float *d_Qd, const float *d_QdT, const float *d_theta,
                             const int *d_sym, const float *d_GpT, const float *d_QinvT, const float *d_Fd,
                             const float *d_Md, const float *d_Qp, const float *d_Qp_inv, const float *d_Fp,
                             const float *d_Mp, const float *d_Gp, const float *d_Kp, int mode, long long num_iter,
                             long long max_updates, float *d_Y, float *d_U, long long *d_h, int *d_status,
                             void *stream);

/* ----------------------------------------------------------------------
 * 2d. Row blocks of one large problem (a single problem
 * row-sharded across GPUs).  A pqp_rowblock holds rows [row0, row0+rows) of
 * updateY2's stored split matrices (PQP_CPU.c:524-537 Qdp_theta/Qdn_theta
 * rows, :703-704 Fdp/Fdn) on the current device.  One step reads the FULL
 * iterate Y (N, device) and writes the block's rows of Y_next
 * (PQP_CPU.c:603-618 restricted to those rows); between steps the caller
 * assembles Y_next from every block (e.g. an RCCL all-gather).  Every row's
 * sums still run over k = 0..N-1 in order, so the assembled Y_next is
 * bit-identical to updateY2's whatever the partition.  N <= 38016 (the full
 * y is staged in LDS).
 * -------------------------------------------------------------------- */
typedef struct pqp_rowblock pqp_rowblock;

/* d_Qd_rows: the block's rows of Qd, row-major with leading dimension ld >= N
 * (a pointer into a full row-major Qd works); d_Fd: the full Fd (N).  Theta_ii
 * of the block's rows is computed from them (computeTheta, PQP_CPU.c:503-519).
 * The inputs may be freed once this returns.  rows == 0 gives an empty block
 * whose update is a no-op. */
int pqp_rowblock_create(const float *d_Qd_rows, int ld, const float *d_Fd, int N, int row0, int rows, void *stream,
                        pqp_rowblock **out);
/* d_Y_rows[i] = updateY2(Y)[row0 + i] for i < rows.  d_Y must hold N floats
 * (more is allowed and ignored).  Async on `stream`. */
int pqp_rowblock_update(pqp_rowblock *b, const float *d_Y, float *d_Y_rows, void *stream);
/* Synchronizes `stream` and reports whether any pqp_rowblock_update of this
 * block since the last check hit an expired wait inside the kernel (a
 * workgroup's wave-to-wave hand-off that never arrived): PQP_ERR_HIP when one
 * did -- the rows it wrote are then not valid -- else PQP_OK.  The check clears
 * the block's error word.  No reference counterpart (the CPU loop cannot
 * fail); call it at the end of a run of updates. */
int pqp_rowblock_check(pqp_rowblock *b, void *stream);
int pqp_rowblock_destroy(pqp_rowblock *b);

/* Rows [row0, row0+rows) of synthetic problem `inst` of `seed` (the
 * generator of pqp_batch_generate), row-major with leading dimension ld >= N
 * (columns N..ld-1 zeroed), so that a rank can build its row block without
 * materialising the whole N x N matrix.  d_Fd (N) and d_Md (1) receive the
 * full Fd / Md when not NULL. */
int pqp_synth_rows(uint32_t seed, long long inst, int N, int M, int row0, int rows, float *d_Qd_rows, int ld,
                   float *d_Fd, float *d_Md, void *stream);

/* ----------------------------------------------------------------------
 * 2e. Receding-horizon re-solve: the NEXT control step of a resident problem.
 * Between two steps of linear MPC only the measured state (and perhaps the
 * bounds Kp) changes: that moves Fp and Mp, and through them Fd = (Gp Qp_inv)
 * Fp + Kp and Md = (Fp' Qp_inv) Fp - Mp (PQP_CPU.c:456-479).  Qd, Theta, the
 * packed matrices and the captured graphs stay.
 *
 * Warm start, everywhere below: the solve is solveQuadraticDual with line :710
 * (initMat(Y, 1000)) replaced by Y = Y0 and nothing else changed -- h still
 * starts at 1, converge mode calls terminate(Y0) before the first update,
 * fixed mode runs num_iter - 1 updates from Y0.  Y0 is taken as given: no
 * clamping, no validation of sign or finiteness.  The update is
 * multiplicative, so an entry of Y0 that is exactly 0 stays 0 for the whole
 * solve ("Receding-horizon re-solve").
 * -------------------------------------------------------------------- */

/* New linear terms for a resident problem: uploads Fp (M), Mp (1) and, when
 * not NULL, Kp (N); recomputes Fd and Md on the device exactly as
 * convertToDual would (PQP_CPU.c:456-479, :491-492; NaN operands: as
 * convertToDual above) and refreshes, in place, everything the solve paths
 * derived from Fd.  Qd, Theta, packed matrices and captured graphs are kept.
 * The first call on a problem also builds Gp Qp_inv (N x M), once. */
int pqp_problem_update_linear(pqp_problem *p, const float *Fp, const float *Mp, const float *Kp);
/* The handle's current Fd (N) and Md (1); either may be NULL. */
int pqp_problem_get_dual(pqp_problem *p, float *Fd, float *Md);
#define PQP_START_COLD 0 /* Y = 1000: identical to pqp_problem_solve                       */
#define PQP_START_HOST 1 /* Y = Y0 (N host floats)                                           */
#define PQP_START_LAST 2 /* Y = the final iterate of this handle's previous solve (device-resident, no
                            upload); PQP_ERR_ARG if the handle has not solved yet */
/* pqp_problem_solve from a chosen start; a warm solve takes the same solver
 * path as a cold solve of the same shape and mode. */
int pqp_problem_solve_from(pqp_problem *p, int start, const float *Y0, int mode, long long num_iter,
                           long long max_updates, float *Y, float *U, long long *h_out, float *Jp_out, float *Jd_out);

/* The batch: device pointers on the caller's stream, in the layout of 2c. */

/* d_GQ [B][N*M] (16-byte aligned) <- Gp Qp_inv per problem (convertToDual's
 * temporary, :491-492), in a layout private to the library (it belongs to
 * the batch as a whole: not sliceable per problem).  Valid until Gp or Qp_inv
 * change.  Synchronous; uses pqp_batch_convert_to_dual's workspace. */
int pqp_batch_relin_prepare(int B, int N, int M, const float *d_Gp, const float *d_Qp_inv, float *d_GQ, void *stream);
/* Fd [B][N] and Md [B] from new Fp [B][M], Mp [B], Kp [B][N]: ONE launch on
 * `stream`, asynchronous, no allocation, no workspace lock, no
 * synchronisation.  Bit-identical to pqp_batch_convert_to_dual's Fd, Md. */
int pqp_batch_relinearize(int B, int N, int M, const float *d_GQ, const float *d_Qp_inv, const float *d_Kp,
                          const float *d_Fp, const float *d_Mp, float *d_Fd, float *d_Md, void *stream);
/* pqp_batch_solve_prepared started from d_Y0 [B][N] (it may be d_Y itself;
 * NULL: cold, identical to pqp_batch_solve_prepared).  Every batched path
 * (0, 1, 2 with both kernels, 3) honours it. */
int pqp_batch_solve_from(int B, int N, int M, const float *d_Qd, const float *d_QdT, const float *d_theta,
                         const int *d_sym, const float *d_GpT, const float *d_QinvT, const float *d_Fd,
                         const float *d_Md, const float *d_Qp, const float *d_Qp_inv, const float *d_Fp,
                         const float *d_Mp, const float *d_Gp, const float *d_Kp, int mode, long long num_iter,
                         long long max_updates, float *d_Y, float *d_U, long long *d_h, int *d_status,
                         const float *d_Y0, void *stream);

/* ----------------------------------------------------------------------
 * 2f. One plant, many states: a resident plant and a one-launch control step.
 * In the MPC workload every problem of a batch is the same plant at another
 * state: Qp_inv, Gp, Kp -- and so Qp, Qd, Theta and Gp Qp_inv -- are shared,
 * only x and D differ, and through them Fp, Mp, Fd and Md.  A pqp_plant keeps
 * the shared data on its device once; pqp_plant_step takes B states through
 * computeFp, computeMp, convertToDual's Fd and Md and the converge solve in
 * ONE asynchronous launch, so steps can be chained on a stream or captured in
 * a graph.
 *
 * Bit-exactness: state b of a step gives exactly what pqp_batch_compute_fp,
 * pqp_batch_compute_mp and pqp_batch_relinearize at that state, followed by
 * pqp_batch_solve_from in PQP_MODE_CONVERGE with the same cap, give for
 * problem b -- that is computeFp (PQP_CPU.c:373), computeMp (:395),
 * convertToDual's Fd and Md (:456-479) and solveQuadraticDual (:694-750, line
 * :710 replaced when warm) -- bit for bit, Jp and Jd included.  NaN operands:
 * as convertToDual above.
 *
 * Shapes: N <= 32, M <= 32, N + M < 64 (one wave per state), nd <= 64,
 * ns <= 64.  Other shapes: the batched entry points of 2c / 2e.  Converge
 * mode only.
 *
 * The plant is immutable after create.  A step writes only the caller's
 * buffers, so steps on different streams may run concurrently without a lock;
 * it runs on the plant's device whatever device the caller has current (and
 * restores the caller's), and does no allocation, no synchronisation and no
 * copy to the host.  The stopping rule is the reference's; pqp_plant_step_tol
 * (2k) adds a caller-set tolerance on the gap.
 * -------------------------------------------------------------------- */
typedef struct pqp_plant pqp_plant;

/* 1 when (N, M, nd, ns) is a shape pqp_plant_step runs, else 0 (no error set). */
int pqp_plant_supported(int N, int M, int nd, int ns);

/* Host pointers, reference layouts (pqp_read_example's): Qp_inv [M*M], Gp [N*M], Kp [N],
 * Fp1 [M*nd], Fp2 [M*ns], Fp3 [M], Mp1 [ns*ns], Mp2 [nd*ns], Mp3 [nd*nd], Mp4 [ns], Mp5 [nd], Mp6 [1].
 * device -1: the current one.  Synchronous.  Derives, once, with the bits of the existing entry
 * points: Qp = Gauss_Jordan(Qp_inv), Qd and Gp Qp_inv as convertToDual forms them
 * (PQP_CPU.c:440-455, :491-492), Theta (computeTheta).  An unsupported shape: PQP_ERR_ARG. */
int pqp_plant_create(int device, int N, int M, int nd, int ns, const float *Qp_inv, const float *Gp,
                     const float *Kp, const float *Fp1, const float *Fp2, const float *Fp3,
                     const float *Mp1, const float *Mp2, const float *Mp3, const float *Mp4,
                     const float *Mp5, const float *Mp6, pqp_plant **out);
int pqp_plant_destroy(pqp_plant *p);
/* Host copies of what create derived; any pointer may be NULL: Qd [N*N], Qp [M*M], theta [N]. */
int pqp_plant_get(pqp_plant *p, float *Qd, float *Qp, float *theta);
/* Largest max_updates a step accepts: one launch never runs longer than the batched
 * solvers' existing per-launch budget for the shape (batch_chunk_for(N, M)). */
long /* (the return type is long long; tests/test_capi.py's prototype scanner reads the last word before the name) */
long pqp_plant_max_updates(const pqp_plant *p);

/* One control step of B states, converge mode, ONE launch on `stream`, asynchronous.
 * In:  d_x [B][ns], d_D [B][nd]; d_Kp NULL (the plant's Kp for every state) or [B][N];
 *      warm 0: Y = 1000 (PQP_CPU.c:710), 1: Y = d_Y's current rows, taken as given (2e's rules).
 * Out: d_Y [B][N] (in/out when warm), d_U [B][M], and, each optional (NULL: not written),
 *      d_h [B] int64 (the reference's printed h), d_status [B] (1 converged, 2 hit max_updates),
 *      d_Fp [B][M], d_Mp [B], d_Fd [B][N], d_Md [B], d_Jp [B], d_Jd [B] (costs of the last
 *      terminate() that passed checkFeas; NaN if none, as pqp_solve_dual).
 * 1 <= max_updates <= pqp_plant_max_updates(p), else PQP_ERR_ARG. */
int pqp_plant_step(pqp_plant *p, int B, const float *d_x, const float *d_D, const float *d_Kp, int warm,
                   long long max_updates, float *d_Y, float *d_U, long long *d_h, int *d_status,
                   float *d_Fp, float *d_Mp, float *d_Fd, float *d_Md, float *d_Jp, float *d_Jd, void *stream);

/* ----------------------------------------------------------------------
 * 2g. The resident plant at horizon sizes.  A plant of H >= 2 stacked stages
 * (the bundled plant: N = 28 H, M = 7 H) is past 2f's one wave per state.
 * pqp_plant_create_horizon also takes those shapes: the same pqp_plant, whose
 * step runs one WORKGROUP per state at a time -- the plant's matrices staged
 * in LDS once per workgroup, only the per-state vectors refreshed between
 * states -- still in ONE asynchronous launch.  pqp_plant_supported and
 * pqp_plant_create accept exactly 2f's shapes as before: the new shapes are
 * opt-in through the two names below.
 *
 * pqp_plant_step, pqp_plant_get, pqp_plant_max_updates and pqp_plant_destroy
 * work on either kind of handle, and pqp_plant_step's contract holds word for
 * word: one launch on `stream`, asynchronous, no allocation, no
 * synchronisation, no copy to the host, the caller's device restored, so it
 * can be chained on a stream or captured in a graph.  (The tuning key
 * plant_pipe has no meaning for the one-workgroup step and is ignored there;
 * plant_grid caps its grid too.)
 *
 * Bit-exactness, as 2f: state b of a step gives exactly what
 * pqp_batch_compute_fp, pqp_batch_compute_mp and pqp_batch_relinearize at
 * that state, followed by pqp_batch_solve_from in PQP_MODE_CONVERGE with the
 * same cap (cold: d_Y0 NULL; warm: from d_Y's rows), give for problem b --
 * Y, U, h, status, Fp, Mp, Fd, Md, bit for bit, Jp and Jd included.  NaN
 * operands: as convertToDual above (which NaN payload a sum propagates is the
 * hardware's choice; positions and every non-NaN bit agree).
 *
 * Shapes of the one-workgroup step (kind 2): N or M above 32, M < 64,
 * nd <= 64, ns <= 64, N <= 192, and (N, M) one that the batched path 3
 * (pqp_batch_solve_path(N, M) == 3 at default tuning) solves within one
 * workgroup's LDS with the plant step's own words added -- 140 x 35 and
 * 40 x 12 among them.  Converge mode only.  pqp_plant_step_tol (2k) runs on
 * either kind of handle too.
 * -------------------------------------------------------------------- */

/* 0: (N, M, nd, ns) is no shape pqp_plant_step runs; 1: the one-wave step of 2f
 * (pqp_plant_supported); 2: the one-workgroup step.  No error set. */
int pqp_plant_kind(int N, int M, int nd, int ns);

/* pqp_plant_create's arguments and derivations (Qp, Gp Qp_inv, Qd, Theta, by the same
 * launchers: the same bits), for a shape of kind 1 or 2; for kind 2 it also finds, once,
 * whether Qd is bit-symmetric and whether it holds a NaN or an inf (which forms of the
 * sums the step may take; no bit depends on them).  Kind 0: PQP_ERR_ARG, *out NULL, the
 * limits in the message. */
int pqp_plant_create_horizon(int device, int N, int M, int nd, int ns, const float *Qp_inv, const float *Gp,
                             const float *Kp, const float *Fp1, const float *Fp2, const float *Fp3,
                             const float *Mp1, const float *Mp2, const float *Mp3, const float *Mp4,
                             const float *Mp5, const float *Mp6, pqp_plant **out);

/* ----------------------------------------------------------------------
 * 2h. The shared-plant converge solve: B states of ONE plant past the plant
 * step's shapes (the bundled plant over 8 to 36 stages: N = 224 .. 1008).
 * A pqp_shared keeps Qp_inv, Gp, Kp and what follows from them alone -- Qp,
 * Qd, Theta, Gp Qp_inv -- on its device once, about 4 (2 N^2 + 5 N M + 5 M^2)
 * bytes (the reference layouts and the kernels' padded ones); a state brings only Fp [M], Mp, Fd [N], Md (and perhaps its own Kp).
 * No replicated ProblemBatch, no d_GQ [B][N*M].  One workgroup solves
 * pqp_shared_states(N, M) states at a time and reads every shared matrix once
 * for all of them (k_solve_shared).
 *
 * Bit-exactness: state b of pqp_shared_solve gives Y, U, h, status, Jp and Jd
 * bit for bit equal to what pqp_batch_solve_from in PQP_MODE_CONVERGE gives
 * problem b of a batch whose every problem holds the handle's Qd, Qp, Qp_inv,
 * Gp and this state's Fd, Md, Fp, Mp, Kp and Y0 -- solveQuadraticDual
 * (PQP_CPU.c:694-750) with terminate() before every update.
 * pqp_shared_relinearize gives pqp_batch_relinearize's (that is
 * pqp_batch_convert_to_dual's) Fd and Md.  NaN operands: as convertToDual
 * above (positions and every non-NaN bit agree; a NaN's sign and payload may
 * differ).
 *
 * Shapes: every 1 <= N <= 1024, 1 <= M <= 1024, and beyond that whatever lets
 * two states' vectors, 2 * 4 * (4 round4(N) + 3 round4(M)) bytes, fit 160 KiB
 * of LDS less 1 KiB; pqp_shared_states is the single answer.  Converge mode
 * only (fixed mode: pqp_batch_iterate_shared, 2b').
 *
 * The handle is immutable after create and bound to its device; calls run
 * there whatever device the caller has current, and restore the caller's.
 * Calls on different streams may run concurrently: a solve's per-state resume
 * words are allocated per call.  Argument errors (a null handle or pointer,
 * B <= 0) are PQP_ERR_ARG before any device is looked for.  A gap tolerance
 * beside the reference's stopping rule: pqp_shared_solve_tol (2k).
 * -------------------------------------------------------------------- */
typedef struct pqp_shared pqp_shared;

/* States per workgroup the shared solve uses for (N, M); 0: unsupported shape.  No error set, no device needed. */
int pqp_shared_states(int N, int M);

/* Host pointers, reference layouts: Qp_inv [M*M], Gp [N*M], Kp [N].  device -1: the current one.
 * Synchronous.  Derives, once, by the launchers pqp_plant_create uses (the bits of the existing entry
 * points): Qp = Gauss_Jordan(Qp_inv), Gp Qp_inv and Qd as convertToDual forms them, Theta, and whether Qd
 * is bit-symmetric.  An unsupported shape: PQP_ERR_ARG, *out NULL, the limit in the message. */
int pqp_shared_create(int device, int N, int M, const float *Qp_inv, const float *Gp, const float *Kp,
                      pqp_shared **out);
int pqp_shared_destroy(pqp_shared *p);
/* Host copies of what create derived; any may be NULL: Qd [N*N], Qp [M*M], theta [N], GQ [N*M] (Gp Qp_inv,
 * row-major); *sym_out = 1 iff Qd is bit-symmetric. */
int pqp_shared_get(pqp_shared *p, float *Qd, float *Qp, float *theta, float *GQ, int *sym_out);

/* Fd [B][N], Md [B] from Fp [B][M], Mp [B]; d_Kp NULL (the handle's Kp for every state) or [B][N].
 * ONE launch, asynchronous on `stream`, no allocation, no synchronisation. */
int pqp_shared_relinearize(pqp_shared *p, int B, const float *d_Fp, const float *d_Mp, const float *d_Kp,
                           float *d_Fd, float *d_Md, void *stream);

/* solveQuadraticDual, converge mode, for B states.
 * In:  d_Fd [B][N], d_Md [B], d_Fp [B][M], d_Mp [B]; d_Kp NULL or [B][N]; d_Y0 NULL (Y = 1000), a separate
 *      [B][N] buffer, or d_Y itself (2e's warm-start rules: Y0 taken as given).  max_updates <= 0: no cap.
 * Out: d_Y [B][N], d_U [B][M], and, each optional (NULL: not written), d_h [B] int64 (the reference's
 *      printed h), d_status [B] (1 converged, 2 hit max_updates), d_Jp [B], d_Jd [B] (costs of the last
 *      terminate() that passed checkFeas; NaN if none).
 * Synchronous like pqp_batch_solve: a sequence of bounded launches on `stream` that resume from device
 * state (the batch_chunk tuning key sets the iterates per launch, as for pqp_batch_solve). */
int pqp_shared_solve(pqp_shared *p, int B, const float *d_Fd, const float *d_Md, const float *d_Fp,
                     const float *d_Mp, const float *d_Kp, long long max_updates, const float *d_Y0,
                     float *d_Y, float *d_U, long long *d_h, int *d_status, float *d_Jp, float *d_Jd,
                     void *stream);

/* ----------------------------------------------------------------------
 * 2i. The shared plant's control step: x, D to U for B states in ONE launch.
 * 2f / 2g give the two small size classes a control step; this is the one of
 * the third (2h's shapes: the bundled plant over 8 to 36 stages, N up to
 * 1024).  pqp_shared_create_plant makes a pqp_shared that also holds the
 * plant's nine linear-term matrices; pqp_shared_step then takes B states
 * through computeFp, computeMp, convertToDual's Fd and Md and the converge
 * solve in one asynchronous launch (k_step_shared), where 2h's
 * pieces take four calls, about 16 launches, 5 allocations and 3 host
 * synchronisations.
 *
 * pqp_shared_step's contract is pqp_plant_step's, word for word: one launch on
 * `stream`, asynchronous, no allocation, no synchronisation, no copy to the
 * host, the caller's device restored, so steps can be chained on a stream or
 * captured in a graph.  Converge mode only.  One difference: d_Fp and d_Fd are
 * required -- one workgroup's LDS is full of iterates, so they are the step's
 * working storage as well as its outputs.
 *
 * Bit-exactness: state b of a step gives exactly what pqp_batch_compute_fp and
 * pqp_batch_compute_mp at that state, pqp_shared_relinearize and
 * pqp_shared_solve with the same cap and start give -- Fp, Mp, Fd, Md, Y, U,
 * h, status, Jp, Jd, bit for bit; that is computeFp (PQP_CPU.c:373), computeMp
 * (:395), convertToDual's Fd and Md (:456-479) and solveQuadraticDual
 * (:694-750, line :710 replaced when warm).  NaN operands: as convertToDual
 * above (positions and every non-NaN bit agree; payloads may differ).
 *
 * pqp_shared_get, pqp_shared_relinearize, pqp_shared_solve and
 * pqp_shared_destroy work on either kind of handle, with the same results.
 * Argument errors (a null handle or required pointer, B <= 0, a cap out of
 * range, a handle without plant matrices) are PQP_ERR_ARG before any device is
 * looked for.  A gap tolerance beside the reference's stopping rule:
 * pqp_shared_step_tol (2k).
 * -------------------------------------------------------------------- */

/* States per workgroup the step uses for (N, M, nd, ns): pqp_shared_states(N, M) where the
 * step's own words for that many states (x, D, x'Mp1, D'Mp2, D'Mp3, Fp, Fp'Qp_inv:
 * 4 * (3 round4(ns) + 2 round4(nd) + 2 round4(M)) bytes each) fit the launch's LDS too, which
 * they do for every nd, ns <= 64; else 0.  nd, ns >= 1.  No error set, no device needed. */
int pqp_shared_step_states(int N, int M, int nd, int ns);

/* pqp_plant_create's arguments; the result is a pqp_shared that holds everything
 * pqp_shared_create derives (by the same launchers: the same bits) and the nine linear-term
 * matrices in the kernel's padded layouts.  An unsupported shape (pqp_shared_step_states 0):
 * PQP_ERR_ARG, *out NULL, the limit in the message. */
int pqp_shared_create_plant(int device, int N, int M, int nd, int ns, const float *Qp_inv, const float *Gp,
                            const float *Kp, const float *Fp1, const float *Fp2, const float *Fp3,
                            const float *Mp1, const float *Mp2, const float *Mp3, const float *Mp4,
                            const float *Mp5, const float *Mp6, pqp_shared **out);

/* Largest max_updates a step accepts (batch_chunk_for(N, M)), as pqp_plant_max_updates. */
long /* (the return type is long long; see pqp_plant_max_updates) */
long pqp_shared_max_updates(const pqp_shared *p);

/* One control step of B states: pqp_plant_step's arguments and meaning (2f), except that d_Fp [B][M]
 * and d_Fd [B][N] are required.  d_h, d_status, d_Mp, d_Md, d_Jp, d_Jd stay optional (NULL: not
 * written).  1 <= max_updates <= pqp_shared_max_updates(p), else PQP_ERR_ARG: every state finishes
 * in this launch.  A handle made by pqp_shared_create (no plant matrices): PQP_ERR_ARG. */
int pqp_shared_step(pqp_shared *p, int B, const float *d_x, const float *d_D, const float *d_Kp, int warm,
                    long long max_updates, float *d_Y, float *d_U, long long *d_h, int *d_status,
                    float *d_Fp, float *d_Mp, float *d_Fd, float *d_Md, float *d_Jp, float *d_Jd, void *stream);

/* ----------------------------------------------------------------------
 * 2j. The closed loop: K control steps of B plant states in one call.
 * 2e to 2i solve the step; what takes a state to the next sample time is the
 * plant's own dynamics x+ = A x + Bu U + Bd D.  A pqp_dynamics keeps A, Bu and
 * Bd on its device; pqp_dynamics_advance takes B states one sample time
 * forward in one launch, and pqp_plant_rollout runs K steps of B states of a
 * pqp_plant -- step, state update, warm step, ... -- without leaving the
 * device: for the one-wave plants of 2f in ONE launch, in which a wave carries
 * its state through all K steps with Y, x and the plant in LDS; for the
 * one-workgroup plants of 2g (and for 2f's under the tuning key
 * plant_roll_chain = 1) as a chain of 2 K launches, k_plant_step or
 * k_plant_step_mid then k_plant_advance, K times (one more launch, the floor,
 * when warm != 0 and y_floor > 0), with no host work in between.  (2l: the
 * one-workgroup plants' own one-launch form, and the caller's choice of form.)
 *
 * The state update is the reference's own primitives, three matrixMultiply
 * (PQP_CPU.c:84) and two matrixAdd (:157): t = A x, v = Bu U, w = Bd D, every
 * sum from +0.0f in index order, every product rounded before its add (no
 * FMA); x+ = (t + 1.0f * v) + 1.0f * w.  Bu acts on the whole U and Bd on the
 * whole D: no stage ordering is assumed.
 *
 * Bit-exactness of the rollout: step k of state b gives exactly what
 * pqp_plant_step gives at x = X[k][b], the D of step k, d_Kp[b] and the same
 * cap -- Y, U, h, status, Jp, Jd, NaN rules included -- started warm whenever
 * k > 0 and as `warm` says at k = 0; before every warm start each entry of Y
 * is replaced by y_floor > Y_i ? y_floor : Y_i when y_floor > 0 (y_floor <= 0:
 * Y is taken as given, as in 2e).  X[k + 1][b] is the state update of X[k][b]
 * with the step's U, whatever its status.  The fused launch and the chain give
 * the same bits.
 *
 * pqp_plant_rollout's contract is pqp_plant_step's, word for word:
 * asynchronous on `stream`, no allocation, no synchronisation, no copy to the
 * host, the caller's device restored, so it can be captured in a graph; it
 * works on both kinds of pqp_plant.  Every argument error is PQP_ERR_ARG
 * before any device is looked for.  Steps with active bounds often settle one
 * ulp above the reference's exact-float stop and run to the cap:
 * pqp_plant_rollout_tol (2k) takes a tolerance on the gap.
 * -------------------------------------------------------------------- */
typedef struct pqp_dynamics pqp_dynamics;

/* Host pointers, row-major: A [ns*ns], Bu [ns*M], Bd [ns*nd].  1 <= ns, nd <= 64, 1 <= M <= 1024
 * (every M of a pqp_plant or a pqp_shared), else PQP_ERR_ARG.  device -1: the current one.
 * Synchronous.  Immutable after create and bound to its device. */
int pqp_dynamics_create(int device, int ns, int M, int nd, const float *A, const float *Bu, const float *Bd,
                        pqp_dynamics **out);
int pqp_dynamics_destroy(pqp_dynamics *d);

/* d_xnext [B][ns] = the state update of d_x [B][ns] with d_U [B][M] and d_D [B][nd].  ONE launch on
 * `stream`, asynchronous, no allocation, no synchronisation; runs on the handle's device and restores
 * the caller's.  d_xnext must not overlap d_x (PQP_ERR_ARG).  The chain's building block; with
 * pqp_shared_step in a graph it closes the shared plant's loop (2i). */
int pqp_dynamics_advance(const pqp_dynamics *d, int B, const float *d_x, const float *d_U, const float *d_D,
                         float *d_xnext, void *stream);

/* 1 when pqp_plant_rollout of that shape is a single launch at default tuning: kind 1 (2f's
 * shapes) with the dynamics within the launch's LDS beside the plant, which holds for every such
 * shape today.  0 when it is the chain (kind 2) or the shape is no plant's.  No device needed, no
 * error set.  (A plant made on a device where that launch has no occupancy takes the chain.) */
int pqp_plant_rollout_fused(int N, int M, int nd, int ns);

/* K steps of B states.
 * In:  d_X [K+1][B][ns]: row 0 the states, never written; rows 1..K are outputs.
 *      d_D [B][nd], used at every step (D_steps == 1), or [K][B][nd] (D_steps == K); any other
 *      D_steps: PQP_ERR_ARG.  d_Kp NULL or [B][N], constant over the steps.  warm, y_floor: above.
 *      1 <= max_updates <= pqp_plant_max_updates(p), per step.  dyn: the plant's ns, M, nd, on
 *      the plant's device.
 * Out: d_Y [B][N], in/out: it ends as step K-1's Y (not floored).  d_U [K][B][M].  d_h, d_status,
 *      d_Jp, d_Jd [K][B], each optional (NULL: not written). */
int pqp_plant_rollout(pqp_plant *p, const pqp_dynamics *dyn, int B, int K, float *d_X, const float *d_D,
                      int D_steps, const float *d_Kp, int warm, float y_floor, long long max_updates,
                      float *d_Y, float *d_U, long long *d_h, int *d_status, float *d_Jp, float *d_Jd,
                      void *stream);

/* ----------------------------------------------------------------------
 * 2k. A gap tolerance for the plant family's stopping rule (2f to 2j).
 * terminate() (PQP_CPU.c:673-687) stops when the float32 gap Jp + Jd is <= 0:
 * its tolerances eaj = erj = 1e-6 never decide at the plants' costs (|Jd| about
 * 1.5e5, where one float32 ulp is 0.0156), so a gap that settles one ulp above
 * zero runs to the cap.  The four _tol entry points below take a caller-set
 * tolerance on that gap; the reference's rule stays the default and stays bit
 * for bit (the entry points of 2f to 2j ARE these with abs_tol = rel_tol = 0).
 *
 * The rule, for an iterate that passed checkFeas (nothing else is evaluated
 * for any other), in this order:
 *   1. the reference's own tests (:682-685) pass: stop, status PQP_STATUS_DONE;
 *   2. both tolerances 0: go on;
 *   3. gap = (double)(Jp + Jd), the float32 sum as :683;
 *      gap <= abs_tol, or gap <= (double)rel_tol * fabs((double)Jd): stop,
 *      status PQP_STATUS_TOL;
 *   4. go on.
 * The reference's test is tried first, so a tolerance can only stop a solve
 * earlier, never later; a NaN gap or a NaN Jd matches no tolerance.  Y, U, h,
 * Jp and Jd of a state are those of the iterate it stopped at, as before: the
 * iterates themselves do not depend on the tolerances.  PQP_STATUS_TOL appears
 * only when a tolerance is positive.
 *
 * A tolerance that is negative, NaN or infinite is PQP_ERR_ARG before any
 * device is looked for (and before any other argument is looked at).  The
 * single-problem handles, pqp_batch_solve* and the drop-ins keep the
 * reference's rule.
 * -------------------------------------------------------------------- */
#define PQP_STATUS_DONE 1   /* the reference's terminate() returned 1                         */
#define PQP_STATUS_CAPPED 2 /* max_updates reached                                             */
#define PQP_STATUS_TOL 3    /* within abs_tol / rel_tol where the reference's test had not passed */

/* The rule above on the host, the same inline function the kernels call: 0 go on, 1 the
 * reference's tests pass, 3 within the tolerances.  No device needed, no error set, no
 * validation: the tolerances are taken as given (a negative or NaN one never matches). */
int pqp_stop_decide(float Jp, float Jd, float abs_tol, float rel_tol);

/* pqp_plant_step (2f, 2g), pqp_plant_rollout (2j), pqp_shared_solve (2h) and pqp_shared_step (2i)
 * with the two tolerances before `stream`.  Every other word of those contracts holds: the
 * launches, asynchrony, no allocation (pqp_shared_solve_tol: as pqp_shared_solve), graph
 * capture, both kinds of pqp_plant, the fused rollout and the chain, which give the same bits. */
int pqp_plant_step_tol(pqp_plant *p, int B, const float *d_x, const float *d_D, const float *d_Kp, int warm,
                       long long max_updates, float *d_Y, float *d_U, long long *d_h, int *d_status,
                       float *d_Fp, float *d_Mp, float *d_Fd, float *d_Md, float *d_Jp, float *d_Jd,
                       float abs_tol, float rel_tol, void *stream);
int pqp_plant_rollout_tol(pqp_plant *p, const pqp_dynamics *dyn, int B, int K, float *d_X, const float *d_D,
                          int D_steps, const float *d_Kp, int warm, float y_floor, long long max_updates,
                          float *d_Y, float *d_U, long long *d_h, int *d_status, float *d_Jp, float *d_Jd,
                          float abs_tol, float rel_tol, void *stream);
int pqp_shared_solve_tol(pqp_shared *p, int B, const float *d_Fd, const float *d_Md, const float *d_Fp,
                         const float *d_Mp, const float *d_Kp, long long max_updates, const float *d_Y0,
                         float *d_Y, float *d_U, long long *d_h, int *d_status, float *d_Jp, float *d_Jd,
                         float abs_tol, float rel_tol, void *stream);
int pqp_shared_step_tol(pqp_shared *p, int B, const float *d_x, const float *d_D, const float *d_Kp, int warm,
                        long long max_updates, float *d_Y, float *d_U, long long *d_h, int *d_status,
                        float *d_Fp, float *d_Mp, float *d_Fd, float *d_Md, float *d_Jp, float *d_Jd,
                        float abs_tol, float rel_tol, void *stream);

/* ----------------------------------------------------------------------
 * 2l. The rollout's form, chosen by the caller.
 * pqp_plant_rollout (2j) and pqp_plant_rollout_tol (2k) pick the form of the
 * closed loop themselves: ONE launch for the one-wave plants of 2f, the chain
 * of 2 K launches for the one-workgroup plants of 2g.  The one-workgroup plants
 * have a fused form too (k_plant_roll_mid: k_plant_step_mid with a step loop
 * inside its state loop).  A workgroup stages the plant once and carries its
 * state through all K steps: step k's Y goes to d_Y[b] and is read back,
 * floored, for step k + 1 after a barrier, and one wave forms X[k + 1][b] with
 * 2j's arithmetic from the dynamics' device copies.  The launch takes the
 * step's LDS, so every shape of 2g has it.  pqp_plant_rollout_form is
 * pqp_plant_rollout_tol with that choice as an argument; the defaults of 2j
 * and 2k, pqp_plant_rollout_fused's answers and the tuning keys keep their
 * meaning.
 *
 * The contract is pqp_plant_rollout_tol's, word for word, in every form:
 * asynchronous on `stream`, no allocation, no synchronisation, no copy to the
 * host, the caller's device restored, capturable in a graph, and the same bits
 * in all seven outputs (X, Y, U, h, status, Jp, Jd) whatever the form.  Every
 * argument error is PQP_ERR_ARG before any device is looked for: the tolerances
 * first (2k), then a `form` outside 0..2, then 2j's.  PQP_ROLL_FUSED on a plant
 * made on a device where the fused launch has no occupancy is PQP_ERR_ARG too.
 * -------------------------------------------------------------------- */
#define PQP_ROLL_DEFAULT 0 /* what pqp_plant_rollout_tol does (fused for kind 1, the chain for kind 2; tuning keys honoured) */
#define PQP_ROLL_CHAIN 1   /* the chain of step and advance launches, either kind */
#define PQP_ROLL_FUSED 2   /* ONE launch, either kind */

/* Bit (1 << form) set for each of PQP_ROLL_CHAIN, PQP_ROLL_FUSED that a plant of that shape can run
 * (6 for every shape of 2f and 2g today); 0: no plant's shape.  No device needed, no error set. */
int pqp_plant_rollout_forms(int N, int M, int nd, int ns);

/* pqp_plant_rollout_tol's arguments, then `form` before `stream`. */
int pqp_plant_rollout_form(pqp_plant *p, const pqp_dynamics *dyn, int B, int K, float *d_X, const float *d_D,
                           int D_steps, const float *d_Kp, int warm, float y_floor, long long max_updates,
                           float *d_Y, float *d_U, long long *d_h, int *d_status, float *d_Jp, float *d_Jd,
                           float abs_tol, float rel_tol, int form, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PQP_H */
