// pqp_capi.cpp -- the C ABI of libpqp (include/pqp.h): a thin host shim that
// validates arguments, moves caller buffers to/from HBM and launches the
// gfx950 kernels of pqp_kernels.hip.  No arithmetic of the solver runs on the
// host: every drop-in function is computed on the GPU and fails loudly (status
// code, or exit(EXIT_FAILURE) for the void drop-ins) when no gfx950 device or
// kernel is available -- there is no CPU fallback.
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <memory>
#include <mutex>
#include <thread>
#include <string>
#include <vector>

#include "pqp_device.h"  // stop_decide: pqp_stop_decide is the kernels' own inline function, on the host
#include "pqp_internal.h"
#include "pqp_launch.h"
#include "pqp_plant.h"
#include "pqp_relin.h"
#include "pqp_shared.h"
#include "pqp_shared_solve.h"

namespace pqp {

namespace {

inline int round4(int n) { return (n + 3) & ~3; }

// RAII device allocation.
struct DevBuf {
    void* p = nullptr;
    size_t bytes_ = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    // moves swap the pointer and its size together (the moved-from buffer
    // frees what this one held)
    DevBuf(DevBuf&& o) noexcept { swap(o); }
    DevBuf& operator=(DevBuf&& o) noexcept {
        swap(o);
        return *this;
    }
    ~DevBuf() { reset(); }
    void swap(DevBuf& o) {
        std::swap(p, o.p);
        std::swap(bytes_, o.bytes_);
    }
    // (re)allocate; a buffer of the same size is kept (same address: no
    // hipMalloc/hipFree pair, and graphs captured over it stay valid)
    int alloc(size_t bytes) {
        if (bytes == 0) bytes = 16;
        if (p && bytes == bytes_) return PQP_OK;
        reset();
        hipError_t e = hipMalloc(&p, bytes);
        if (e != hipSuccess) {
            p = nullptr;
            return set_error(PQP_ERR_ALLOC, "hipMalloc(%zu bytes): %s", bytes, hipGetErrorString(e));
        }
        bytes_ = bytes;
        return PQP_OK;
    }
    int floats(size_t n) { return alloc(n * sizeof(float)); }
    float* f() const { return static_cast<float*>(p); }
    void reset() {
        if (p) (void)hipFree(p);
        p = nullptr;
        bytes_ = 0;
    }
};

// One pinned host block, grow-only: a request no larger than the block keeps
// it (and its address).  `dev` is its device address when it was mapped
// (hipHostMallocMapped).
struct PinnedBuf {
    void* p = nullptr;
    void* dev = nullptr;
    size_t bytes_ = 0;
    PinnedBuf() = default;
    PinnedBuf(const PinnedBuf&) = delete;
    PinnedBuf& operator=(const PinnedBuf&) = delete;
    ~PinnedBuf() { reset(); }
    int reserve(size_t bytes, unsigned flags = hipHostMallocDefault) {
        if (p && bytes <= bytes_) return PQP_OK;
        reset();
        PQP_HIP(hipHostMalloc(&p, bytes, flags));
        bytes_ = bytes;
        if (flags & hipHostMallocMapped) PQP_HIP(hipHostGetDevicePointer(&dev, p, 0));
        return PQP_OK;
    }
    template <class T>
    T* as() const { return static_cast<T*>(p); }
    float* f() const { return as<float>(); }
    void reset() {
        if (p) (void)hipHostFree(p);
        p = dev = nullptr;
        bytes_ = 0;
    }
};

// One instantiated hipGraph.
struct GraphExec {
    hipGraphExec_t exec = nullptr;
    GraphExec() = default;
    GraphExec(const GraphExec&) = delete;
    GraphExec& operator=(const GraphExec&) = delete;
    GraphExec(GraphExec&& o) noexcept { std::swap(exec, o.exec); }
    GraphExec& operator=(GraphExec&& o) noexcept {
        std::swap(exec, o.exec);
        return *this;
    }
    ~GraphExec() { reset(); }
    void reset() {
        if (exec) (void)hipGraphExecDestroy(exec);
        exec = nullptr;
    }
    // Replace the graph by what body() (-> hipError_t) enqueues on s.  A
    // failing body is reported before a failing end of the capture.
    template <class Body>
    int capture(hipStream_t s, Body&& body) {
        reset();
        hipGraph_t g = nullptr;
        PQP_HIP(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
        const hipError_t e = body();
        const hipError_t e2 = hipStreamEndCapture(s, &g);
        if (e != hipSuccess || e2 != hipSuccess) {
            if (g) (void)hipGraphDestroy(g);
            PQP_HIP(e != hipSuccess ? e : e2);
        }
        const hipError_t e3 = hipGraphInstantiate(&exec, g, nullptr, nullptr, 0);
        (void)hipGraphDestroy(g);
        PQP_HIP(e3);
        return PQP_OK;
    }
};

// The relay update's operand for a block of rows of one problem (a whole
// problem, or one pqp_rowblock): the stored split matrices with lw row sides
// per workgroup and {Fdp, Fdn}, or (lean) Qd packets with lw / 2 rows per
// workgroup (k_lean_relay, half the bytes) and the {Fdn, Fdp, Theta, 0} words.
struct RelayBlock {
    DevBuf SP, fdpn;
    DevBuf err;  // sticky relay hand-off error word
    int lw = 64;
    bool lean = false;
};

// Verify that the current device is a gfx950 (the only code object we ship).
int ensure_device() {
    static std::mutex mu;
    static int checked[64] = {0};  // 0 unknown, 1 ok, <0 error code
    int dev = 0;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) return set_error(PQP_ERR_NO_DEVICE, "libpqp: no HIP device visible");
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64)
        return set_error(PQP_ERR_NO_DEVICE, "libpqp: cannot query the current device");
    std::lock_guard<std::mutex> lk(mu);
    if (checked[dev] == 0) {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, dev) != hipSuccess) {
            checked[dev] = PQP_ERR_NO_DEVICE;
        } else if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
            checked[dev] = PQP_ERR_NO_DEVICE;
            return set_error(PQP_ERR_NO_DEVICE, "libpqp is built for gfx950 only; device %d is %s", dev,
                             prop.gcnArchName);
        } else {
            checked[dev] = 1;
        }
    }
    if (checked[dev] < 0) return set_error(checked[dev], "libpqp: device %d is not a usable gfx950", dev);
    return PQP_OK;
}

// The stream of the drop-ins and of handles made without one: one per host
// thread and device, so calls from different threads never share a stream
// (or a lock); the drop-ins keep no other state between calls.  A thread's
// streams are destroyed when the thread exits (short-lived caller
// threads must not leak one stream each); the loading thread's stay until the
// process ends, where the HIP runtime may already be shutting down.
static const std::thread::id g_load_thread = std::this_thread::get_id();
struct ThreadStreams {
    hipStream_t s[64] = {nullptr};
    ~ThreadStreams() {
        if (std::this_thread::get_id() == g_load_thread) return;
        for (hipStream_t& x : s)
            if (x) (void)hipStreamDestroy(x);
    }
};
hipStream_t lib_stream() {
    thread_local ThreadStreams streams;
    int dev = 0;
    (void)hipGetDevice(&dev);
    if (dev < 0 || dev >= 64) dev = 0;
    if (!streams.s[dev]) (void)hipStreamCreateWithFlags(&streams.s[dev], hipStreamNonBlocking);
    return streams.s[dev];
}

// Make `dev` the calling thread's current device for a scope (a handle's calls
// run on the device it was made on, whatever the caller has current), and
// restore the caller's device after.
struct DeviceGuard {
    int prev = -1;
    bool changed = false;
    explicit DeviceGuard(int dev) {
        if (dev >= 0 && hipGetDevice(&prev) == hipSuccess && prev != dev) changed = hipSetDevice(dev) == hipSuccess;
    }
    ~DeviceGuard() {
        if (changed) (void)hipSetDevice(prev);
    }
    DeviceGuard(const DeviceGuard&) = delete;
    DeviceGuard& operator=(const DeviceGuard&) = delete;
};

int upload(DevBuf& d, const float* h, size_t n, hipStream_t s) {
    PQP_TRY(d.floats(n));
    if (n) PQP_HIP(hipMemcpyAsync(d.p, h, n * sizeof(float), hipMemcpyHostToDevice, s));
    return PQP_OK;
}
int download(float* h, const void* d, size_t n, hipStream_t s) {
    if (n) PQP_HIP(hipMemcpyAsync(h, d, n * sizeof(float), hipMemcpyDeviceToHost, s));
    return PQP_OK;
}

// ---- device compositions of the reference's helper functions -------------
int dev_matmul(float* out, const float* A, int tA, const float* B, int tB, int a, int b, int c, hipStream_t s) {
    PQP_HIP(launch_matmul_seq(out, A, tA, B, tB, a, b, c, s));
    return PQP_OK;
}

// convertToDual (PQP_CPU.c:489-498)
int dev_convert_to_dual(float* Qd, float* Fd, float* Md, const float* Qinv, const float* Gp, const float* Kp,
                        const float* Fp, const float* Mp, int N, int M, hipStream_t s) {
    DevBuf GQ, fq;
    PQP_TRY(GQ.floats((size_t)N * M));
    PQP_TRY(fq.floats(M));
    PQP_TRY(dev_matmul(GQ.f(), Gp, 0, Qinv, 0, N, M, M, s));  // Gp_Qp_inv          :492
    PQP_TRY(dev_matmul(Qd, GQ.f(), 0, Gp, 1, N, M, N, s));    // computeQd          :442
    PQP_TRY(dev_matmul(Fd, GQ.f(), 0, Fp, 0, N, M, 1, s));    // computeFd          :458
    PQP_HIP(launch_axpy(Fd, Kp, 1.0f, N, s));                  //                    :459
    PQP_TRY(dev_matmul(fq.f(), Fp, 1, Qinv, 0, 1, M, M, s));  // computeMd          :475
    PQP_TRY(dev_matmul(Md, fq.f(), 0, Fp, 0, 1, M, 1, s));    //                    :476
    PQP_HIP(launch_axpy(Md, Mp, -1.0f, 1, s));                 // Md[0] -= Mp[0]     :478
    PQP_HIP(hipStreamSynchronize(s));                          // before scratch is freed
    return PQP_OK;
}

// computeUfromY (PQP_CPU.c:352-360)
int dev_u_from_y(float* U, const float* Y, const float* Fp, const float* Gp, const float* Qinv, int N, int M,
                 hipStream_t s) {
    DevBuf t;
    PQP_TRY(t.floats(M));
    PQP_TRY(dev_matmul(t.f(), Gp, 1, Y, 0, M, N, 1, s));
    PQP_HIP(launch_axpy(t.f(), Fp, 1.0f, M, s));
    PQP_TRY(dev_matmul(U, Qinv, 0, t.f(), 0, M, M, 1, s));
    PQP_HIP(launch_negate(U, M, s));
    PQP_HIP(hipStreamSynchronize(s));
    return PQP_OK;
}

// checkFeas (PQP_CPU.c:632-641) -> host int
int dev_check_feas(const float* U, const float* Gp, const float* Kp, int N, int M, int* out, hipStream_t s) {
    DevBuf gu, flag;
    PQP_TRY(gu.floats(N));
    PQP_TRY(flag.alloc(sizeof(int)));
    const int one = 1;
    PQP_HIP(hipMemcpyAsync(flag.p, &one, sizeof(int), hipMemcpyHostToDevice, s));
    PQP_TRY(dev_matmul(gu.f(), Gp, 0, U, 0, N, M, 1, s));
    PQP_HIP(launch_compare(gu.f(), Kp, N, static_cast<int*>(flag.p), s));
    PQP_HIP(hipMemcpyAsync(out, flag.p, sizeof(int), hipMemcpyDeviceToHost, s));
    PQP_HIP(hipStreamSynchronize(s));
    return PQP_OK;
}

// computeCost (PQP_CPU.c:648-666) -> device scalar J
int dev_cost(float* J, const float* Z, const float* Q, const float* F, const float* Mc, int n, hipStream_t s) {
    DevBuf row, quad, lin;
    PQP_TRY(row.floats(n));
    PQP_TRY(quad.floats(1));
    PQP_TRY(lin.floats(1));
    PQP_TRY(dev_matmul(row.f(), Z, 1, Q, 0, 1, n, n, s));
    PQP_TRY(dev_matmul(quad.f(), row.f(), 0, Z, 0, 1, n, 1, s));
    PQP_TRY(dev_matmul(lin.f(), F, 1, Z, 0, 1, n, 1, s));
    PQP_HIP(launch_cost_finish(quad.f(), lin.f(), Mc, J, s));
    PQP_HIP(hipStreamSynchronize(s));
    return PQP_OK;
}

// computeFp (PQP_CPU.c:373-382)
int dev_compute_fp(float* Fp, const float* Fp1, const float* Fp2, const float* Fp3, const float* D, const float* x,
                   int m, int nd, int ns, hipStream_t s) {
    DevBuf t;
    PQP_TRY(t.floats(m));
    PQP_TRY(dev_matmul(Fp, Fp1, 0, D, 0, m, nd, 1, s));
    PQP_TRY(dev_matmul(t.f(), Fp2, 0, x, 0, m, ns, 1, s));
    PQP_HIP(launch_axpy(Fp, t.f(), 1.0f, m, s));
    PQP_HIP(launch_axpy(Fp, Fp3, -1.0f, m, s));
    PQP_HIP(hipStreamSynchronize(s));
    return PQP_OK;
}

// computeMp (PQP_CPU.c:395-428)
int dev_compute_mp(float* Mp, const float* Mp1, const float* Mp2, const float* Mp3, const float* Mp4,
                   const float* Mp5, const float* Mp6, const float* D, const float* x, int nd, int ns,
                   hipStream_t s) {
    DevBuf row, terms;
    PQP_TRY(row.floats(ns > nd ? ns : nd));
    PQP_TRY(terms.floats(5));
    float* T = terms.f();
    PQP_TRY(dev_matmul(row.f(), x, 1, Mp1, 0, 1, ns, ns, s));     // x' Mp1
    PQP_TRY(dev_matmul(T + 0, row.f(), 0, x, 0, 1, ns, 1, s));    //  . x
    PQP_TRY(dev_matmul(row.f(), D, 1, Mp2, 0, 1, nd, ns, s));     // D' Mp2
    PQP_TRY(dev_matmul(T + 1, row.f(), 0, x, 0, 1, ns, 1, s));    //  . x
    PQP_TRY(dev_matmul(T + 2, Mp4, 1, x, 0, 1, ns, 1, s));        // Mp4' x
    PQP_TRY(dev_matmul(row.f(), D, 1, Mp3, 0, 1, nd, nd, s));     // D' Mp3
    PQP_TRY(dev_matmul(T + 3, row.f(), 0, D, 0, 1, nd, 1, s));    //  . D
    PQP_TRY(dev_matmul(T + 4, Mp5, 1, D, 0, 1, nd, 1, s));        // Mp5' D
    PQP_HIP(launch_mp_finish(T, Mp6, Mp, s));
    PQP_HIP(hipStreamSynchronize(s));
    return PQP_OK;
}

// Gauss_Jordan (PQP_CPU.c:251-326)
int dev_gauss_jordan(float* res, const float* A, int n, hipStream_t s) {
    DevBuf aug, fac;
    PQP_TRY(aug.floats(gauss_jordan_aug_floats(n)));
    PQP_TRY(fac.floats(n));
    PQP_HIP(launch_gauss_jordan(A, aug.f(), fac.f(), res, n, s));
    PQP_HIP(hipStreamSynchronize(s));
    return PQP_OK;
}

// ---- single-problem solve ---------------------------------------------------
struct SolveOut {
    long long h = 0;
    float Jp = NAN, Jd = NAN;
    int have_costs = 0, last_stop = 0, status = 0;
    bool staged = false;  // Y (and U) already copied to the problem's pinned staging buffer
};

}  // namespace
}  // namespace pqp

// A dual problem resident in HBM, prepared once and solved any number of times
// (include/pqp.h: pqp_problem_create / _solve / _destroy).  Bound to the
// device it was made on and to its own stream; calls on one handle are
// serialized by its own lock, calls on different handles run concurrently
// (the reference's solver keeps no globals, PQP_CPU.c:694).
struct pqp_problem {
    // (Members are destroyed last to first: the pinned blocks, the work
    // buffers, what was derived, the inputs.  The order blocks go back to the
    // allocator in decides where the process's later allocations land.)

    // the problem: row-major device copies of the nine inputs
    int N = 0, M = 0;
    pqp::DevBuf Qd, Fd, Md, Qp, Qinv, Fp, Mp, Gp, Kp;
    bool small = false;  // fits k_solve_small (everything staged in LDS)

    // Everything built on first use from the problem's data.  The captured
    // graphs hold these buffers' addresses: the stream is idle when it is dropped.
    struct Derived {
        pqp::DevBuf QdT;    // the one-workgroup solver's column-major Qd (ensure_single)
        pqp::DevBuf theta;  // ensure_theta
        struct Relay {  // fixed mode on the graph-replayed relay; the wide chain's update
            pqp::RelayBlock block;          // rows 0 .. N-1
            pqp::GraphExec chunk, rem;      // kFixedChunk updates; the remainder
            bool chunk_ready = false;
            long long graph_updates = -1;   // updates `rem` was captured with
            long long graph_variant = -1;   // the settings both were captured with
        } relay;
        pqp::DevBuf Yb;  // the second iterate of the multi-workgroup paths
        struct Persist {  // persistent fixed mode: split matrices (lw = 32), y granules, error word
            pqp::DevBuf SP, fdpn, gran, err;
        } persist;
        struct Wide {  // converge mode over many workgroups (pqp_wide.hip)
            pqp::DevBuf QinvT, GpT, tM, tq, tu, gu, flag, cap;
            pqp::GraphExec first, g4, g8, full;  // chunks of kWideFirstChunk, 4, 8, kWideChunk iterations
            long long key = -1;                   // the settings they were captured with
        } wide;
        struct Converge {  // converge mode as one persistent pipelined launch (pqp_converge.hip)
            pqp::DevBuf A1, A2, A3, rings, words;
        } conv;
        pqp::DevBuf GQ;  // Gp Qp_inv in k_relin_pack's layout (pqp_problem_update_linear)
    } d;

    // handle-lifetime state: survives new data going into the handle
    int dev = -1;                  // the device every call of this handle runs on
    hipStream_t stream = nullptr;  // the handle's stream (owned unless the caller passed one)
    bool own_stream = false;
    std::mutex mu;
    pqp::DevBuf Y, U, state;
    pqp::DevBuf Y0;         // the iterate a warm solve starts from (a path that falls back starts from it again)
    bool has_last = false;  // P.Y holds the final iterate of a solve of the current problem (PQP_START_LAST)
    pqp::PinnedBuf hout;  // mapped output of the one-launch tiny solves (kTinyOut* layout)
    pqp::PinnedBuf hin;   // staging of small problems' inputs
    pqp::PinnedBuf hio;   // staging of Y (N floats) then U (M floats)
    pqp::PinnedBuf hst;   // host mirror of `state`
    unsigned out_tag = 0;  // the last tag a tiny launch was given (1 .. 2^31 - 1)

    ~pqp_problem() {
        if (own_stream && stream) (void)hipStreamDestroy(stream);
    }
};

// One row block of a large problem's stored split matrices (pqp_rowblock_*).
struct pqp_rowblock {
    int N = 0, row0 = 0, rows = 0;
    int dev = -1;  // the device it was made on (its calls run there)
    pqp::RelayBlock relay;
};

// What both plant handles (pqp_plant, pqp_shared) keep of one plant: Qp_inv, Gp and Kp as given, and what
// derive_plant_core makes of them once -- Qp, Qd, Gp Qp_inv, Theta and, where asked, sym: Qd bit-symmetric.
namespace pqp {
namespace {
struct PlantCore {
    DevBuf Qinv, Gp, Kp, Qp, Qd, GQ, theta;
    int sym = 0;
};
}  // namespace
}  // namespace pqp

// One plant resident on its device (pqp_plant_*): the primal data as given,
// what create derived from them, and the pointers a step hands its launch.
// Immutable after create; a step writes only the caller's buffers.
struct pqp_plant {
    int N = 0, M = 0, nd = 0, ns = 0;
    int kind = 1;            // pqp_plant_kind: 1 the one-wave step, 2 the one-workgroup step (2g)
    int dev = -1;            // the device it was made on (its steps run there)
    int slots[2] = {0, 0};   // workgroups resident at once: [0] the plain form, [1] the pipelined one (kind 2: both its one form)
    pqp::PlantMidFlags mid{};  // kind 2: what Qd alone decides in k_solve_mid2's staging
    pqp::PlantCore core;
    pqp::DevBuf Fp1, Fp2, Fp3, Mp1, Mp2, Mp3, Mp4, Mp5, Mp6;
    pqp::PlantData data{};
    int roll_slots = 0;      // kind 1: workgroups of the fused rollout resident at once (0: the rollout is the chain)
    int roll_mid_slots = 0;  // kind 2: workgroups of k_plant_roll_mid resident at once (0: PQP_ROLL_FUSED is refused)
};

// A plant's state update x+ = (A x + Bu U) + Bd D resident on its device (pqp_dynamics_*, 2j): the three
// matrices transposed, as k_plant_advance and the fused rollout read them.  Immutable after create.
struct pqp_dynamics {
    int ns = 0, M = 0, nd = 0;
    int dev = -1;  // the device it was made on (its calls run there)
    pqp::DevBuf AT, BuT, BdT;
    pqp::DynData data{};
};

// One plant's shared data for the shared-plant converge solve (pqp_shared_*, 2h): the primal data as
// given, what create derived, and the padded k-major layouts k_solve_shared / k_relin_shared read
// (pqp_shared_solve.h).  Immutable after create; a call writes only the caller's buffers.
struct pqp_shared {
    int N = 0, M = 0, ldq = 0, ldm = 0;
    int S = 0;     // states per workgroup (pqp_shared_states)
    int dev = -1;  // the device it was made on (its calls run there)
    pqp::PlantCore core;  // core.sym: QdR is its own column-major copy
    pqp::DevBuf QdR, QdT, GpP, GpT, QinvT, QinvR, QpP, GQT;
    // pqp_shared_create_plant only (2i): the linear-term matrices k_step_shared reads; nd = ns = 0 without them
    int nd = 0, ns = 0;
    pqp::DevBuf Fp1T, Fp2T, Fp3, Mp1P, Mp2P, Mp3P, Mp4, Mp5, Mp6;
};

namespace pqp {
Tuning g_tune;

namespace {

constexpr size_t kLdsBudget = 150 * 1024;
inline bool batch_unfused() { return (g_tune.batch_opts & 1) != 0; }

// Iterates per launch of a resumable solve: about `budget` element updates
// (one iterate is 3 N^2 + 2 N M + 2 M^2 + 1 of them), at least `floor`.  So a
// long fixed-mode solve or an uncapped converge solve is a sequence of
// launches that resume from the device state, not one kernel running for
// minutes.
long long updates_per_launch(int N, int M, long long budget, long long floor) {
    const double per_update = 3.0 * N * N + 2.0 * N * M + 2.0 * M * M + 1.0;
    return std::max(floor, (long long)((double)budget / per_update));
}

// Theta (computeTheta, PQP_CPU.c:503-519), built on first use: with the
// handle for a large problem, by the first multi-workgroup solve of a small one.
int ensure_theta(pqp_problem& P, hipStream_t s) {
    if (P.d.theta.p) return PQP_OK;
    PQP_TRY(P.d.theta.floats(P.N));
    PQP_HIP(launch_theta_rows(P.Qd.f(), P.N, P.N, P.N, P.d.theta.f(), s));
    return PQP_OK;
}

// Allocate the per-problem work buffers and, for the large path, theta.  The
// nine input buffers must already hold the problem.
int problem_finish(pqp_problem& P, hipStream_t s) {
    const int N = P.N, M = P.M;
    P.small = solve_small_lds_bytes(N, M) <= kLdsBudget;
    PQP_TRY(P.Y.floats(N));
    PQP_TRY(P.Y0.floats(N));
    PQP_TRY(P.U.floats(M));
    // the state, then the int error word a one-launch tiny solve stores behind it (kTinyDevErr)
    PQP_TRY(P.state.alloc(sizeof(SolveState) + 16));
    PQP_HIP(hipMemsetAsync(P.state.p, 0, sizeof(SolveState) + 16, s));
    PQP_HIP(hipMemsetAsync(P.U.p, 0, sizeof(float) * M, s));
    PQP_TRY(P.hst.reserve(sizeof(SolveState)));
    PQP_TRY(P.hio.reserve(sizeof(float) * ((size_t)N + M)));
    if (!P.small) PQP_TRY(ensure_theta(P, s));
    return PQP_OK;
}

// The one-workgroup solver's column-major copy of Qd, built on first use (the
// multi-workgroup paths do not need it).
int ensure_single(pqp_problem& P, hipStream_t s) {
    if (P.d.QdT.p) return PQP_OK;
    const int N = P.N, M = P.M, ldq = round4(N);
    if (solve_single_lds_bytes(ldq, round4(M)) > kLdsBudget)
        return set_error(PQP_ERR_ARG,
                         "N=%d, M=%d exceeds the one-workgroup solver's LDS budget (terminate() drop-in / resumed "
                         "solves); converge and fixed mode run over many workgroups", N, M);
    PQP_TRY(P.d.QdT.floats((size_t)N * ldq));
    PQP_HIP(launch_pack_colmajor(1, P.Qd.f(), N, (long long)N * N, P.d.QdT.f(), ldq, (long long)N * ldq, s));
    return PQP_OK;
}

// Drop everything derived from a problem's data (built on first use by the
// solve paths): called before new data goes into an existing handle.
void problem_reset_derived(pqp_problem& P) { P.d = pqp_problem::Derived{}; }

int problem_upload(pqp_problem& P, const float* qd, const float* fd, const float* md, const float* qp,
                   const float* qinv, const float* fp, const float* mp, const float* gp, const float* kp, int N, int M,
                   hipStream_t s) {
    if (P.Qd.p) {  // new data into an existing handle
        PQP_HIP(hipStreamSynchronize(s));  // the captured graphs hold the derived buffers' addresses
        problem_reset_derived(P);
    }
    P.N = N;
    P.M = M;
    P.has_last = false;
    const size_t nn = (size_t)N * N, mm = (size_t)M * M, nm = (size_t)N * M;
    const size_t total = nn + N + 1 + 2 * mm + M + 1 + nm + N;
    // small problems: every input through one pinned staging buffer, so the
    // nine H2D copies are asynchronous DMA instead of pageable copies
    float* h = nullptr;
    if (total <= (size_t)1 << 18) {
        PQP_TRY(P.hin.reserve(sizeof(float) * total));
        h = P.hin.f();
    }
    auto put = [&](DevBuf& d, const float* src, size_t n) -> int {
        if (!h) return upload(d, src, n, s);
        std::memcpy(h, src, sizeof(float) * n);
        PQP_TRY(upload(d, h, n, s));
        h += n;
        return PQP_OK;
    };
    PQP_TRY(put(P.Qd, qd, nn));
    PQP_TRY(put(P.Fd, fd, N));
    PQP_TRY(put(P.Md, md, 1));
    PQP_TRY(put(P.Qp, qp, mm));
    PQP_TRY(put(P.Qinv, qinv, mm));
    PQP_TRY(put(P.Fp, fp, M));
    PQP_TRY(put(P.Mp, mp, 1));
    PQP_TRY(put(P.Gp, gp, nm));
    PQP_TRY(put(P.Kp, kp, N));
    return problem_finish(P, s);
}

// Lanes per workgroup of the relay update of an n_dual = N problem: row sides
// of the stored split matrices, or rows of Qd for the lean relay.
int pick_lw(int N) { return use_lean(N, N) ? lean_pick_lw(N) : split_pick_lw(N); }

// A block's sticky error word, made (and cleared) once.
int relay_error_word(RelayBlock& b, hipStream_t s) {
    if (b.err.p) return PQP_OK;
    PQP_TRY(b.err.alloc(sizeof(int)));
    PQP_HIP(hipMemsetAsync(b.err.p, 0, sizeof(int), s));
    return PQP_OK;
}

// Build the relay update's operand for rows row0 .. row0 + rows - 1 of an
// n_dual = N problem from those rows of Qd (leading dimension ld) and their
// theta: the stored split matrices with lw row sides per workgroup, or, for a
// block of rows x N >= g_tune.lean_min_n^2 entries, the Qd rows themselves
// with lw / 2 rows per workgroup (k_lean_relay, half the bytes).  By the
// block's entries: the bytes the lean layout saves grow with rows x N, the
// chain both layouts run with N alone.
int relay_build(RelayBlock& b, const float* qd_rows, int ld, const float* theta, const float* Fd, int N, int rows,
                int row0, int lw, hipStream_t s) {
    PQP_TRY(relay_error_word(b, s));
    const bool lean = use_lean(N, rows);
    const size_t sp = lean ? lean_floats(N, rows, lw) : split_floats(N, rows, lw);
    PQP_TRY(b.SP.floats(sp));
    PQP_TRY(b.fdpn.floats(lean ? lean_aux_floats(N, rows, lw) : (size_t)2 * rows));
    PQP_HIP(hipMemsetAsync(b.SP.p, 0, sizeof(float) * sp, s));
    PQP_HIP((lean ? launch_build_lean : launch_build_split)(qd_rows, ld, theta, Fd, N, rows, row0, lw, b.SP.f(),
                                                            b.fdpn.f(), s));
    b.lw = lw;
    b.lean = lean;
    return PQP_OK;
}

// One relay update of a block's rows, Yin (N) -> Yout (rows), over the operand relay_build made.
hipError_t relay_update(const RelayBlock& b, int N, int rows, int row0, const float* Yin, float* Yout, hipStream_t s,
                        const int* gate = nullptr) {
    return (b.lean ? launch_lean_update : launch_split_update)(b.SP.f(), b.fdpn.f(), N, rows, row0, b.lw, Yin, Yout, s,
                                                               gate, static_cast<int*>(b.err.p));
}

// The relay update's operand of the whole problem (rows 0..N-1), built on
// first use (and rebuilt if lw or the layout changes).
int ensure_split(pqp_problem& P, int lw, hipStream_t s) {
    const int N = P.N;
    RelayBlock& b = P.d.relay.block;
    if (b.SP.p && b.lw == lw && b.lean == use_lean(N, N)) return PQP_OK;
    if (split_lds_bytes(N) > kLdsBudget)
        return set_error(PQP_ERR_ARG, "multi-workgroup solve: N=%d needs more than %zu B of LDS", N, kLdsBudget);
    PQP_TRY(ensure_theta(P, s));
    PQP_TRY(P.d.Yb.floats(N));
    return relay_build(b, P.Qd.f(), N, P.d.theta.f(), P.Fd.f(), N, N, 0, lw, s);
}

// One relay update of the whole problem, a -> b, over the operand ensure_split built.
hipError_t problem_update(pqp_problem& P, const float* a, float* b, hipStream_t s, const int* gate = nullptr) {
    return relay_update(P.d.relay.block, P.N, P.N, 0, a, b, s, gate);
}

// The relay kernels' sticky error word: read (the caller synchronizes s
// after this call) and, when set, cleared and turned into PQP_ERR_HIP.
int relay_error_check(DevBuf& word, int* host, hipStream_t s, const char* what) {
    PQP_HIP(hipStreamSynchronize(s));
    if (*host) {
        const int code = *host;
        *host = 0;
        PQP_HIP(hipMemsetAsync(word.p, 0, sizeof(int), s));
        PQP_HIP(hipStreamSynchronize(s));
        return set_error(PQP_ERR_HIP, "%s: a relay hand-off wait expired (code %d); the result is not valid", what,
                         code);
    }
    return PQP_OK;
}

// Capture `n` dependent updates P.Y -> Yb -> P.Y ... into g (plus a copy back
// into P.Y when n is odd).
int capture_updates(pqp_problem& P, long long n, GraphExec& g, hipStream_t s) {
    return g.capture(s, [&]() -> hipError_t {
        float* a = P.Y.f();
        float* b = P.d.Yb.f();
        hipError_t e = hipSuccess;
        for (long long u = 0; u < n && e == hipSuccess; ++u) {
            e = problem_update(P, a, b, s);
            std::swap(a, b);
        }
        if (e == hipSuccess && a != P.Y.f())
            e = hipMemcpyAsync(P.Y.p, a, sizeof(float) * P.N, hipMemcpyDeviceToDevice, s);
        return e;
    });
}

// The stored split matrices in the 32-lane layout (k_build_split), built once
// per problem: the persistent fixed-mode launch and the persistent converge
// launch's update role hold them in LDS.
int ensure_persist_split(pqp_problem& P, hipStream_t s) {
    const int N = P.N;
    auto& ps = P.d.persist;
    if (ps.SP.p) return PQP_OK;
    PQP_TRY(ensure_theta(P, s));
    PQP_TRY(P.d.Yb.floats(N));
    PQP_TRY(ps.SP.floats(split_floats(N, N, 32)));
    PQP_TRY(ps.fdpn.floats((size_t)2 * N));
    PQP_HIP(hipMemsetAsync(ps.SP.p, 0, sizeof(float) * split_floats(N, N, 32), s));
    PQP_HIP(launch_build_split(P.Qd.f(), N, P.d.theta.f(), P.Fd.f(), N, N, 0, 32, ps.SP.f(), ps.fdpn.f(), s));
    PQP_TRY(ps.gran.alloc(sizeof(unsigned long long) * 2 * N));
    PQP_TRY(ps.err.alloc(sizeof(int)));
    return PQP_OK;
}

// Which solver the last single-problem solve ran (pqp_tune_get("last_path")), and
// how many persistent launches fell back to the relay / graph path.
enum SolvePath : int {
    kPathFixedPersist = 1, kPathFixedRelay = 2, kPathConvergePersist = 3, kPathConvergeWide = 4, kPathOneWorkgroup = 5
};
thread_local int g_last_path = 0;               // of the calling thread's last solve
std::atomic<long long> g_persist_fallbacks{0};
std::atomic<long long> g_tiny_stale{0};  // tiny solves whose pinned output did not carry their tag
// problem_run_*_persist: a wait of the persistent launch expired (its
// workgroups were not all resident); the caller falls back
constexpr int kPersistStalled = 1;

// A persistent launch needs every one of its workgroups resident at once (they
// wait on each other).  Two of them from different handles on one device could
// each get part of the CUs and wait for the rest until their deadline, so the
// persistent launches of one device run one at a time; everything else of
// different handles runs concurrently.
std::mutex& persist_lock() {
    static std::mutex mu[64];
    int dev = 0;
    (void)hipGetDevice(&dev);
    return mu[dev >= 0 && dev < 64 ? dev : 0];
}

// What a solve reports, from the SolveState its last launch left.
void report(const SolveState& st, SolveOut& out) {
    out.h = st.h;
    out.status = st.status;
    out.have_costs = st.have_costs;
    out.last_stop = st.last_stop;
    if (st.have_costs) {
        out.Jp = st.Jp;
        out.Jd = st.Jd;
    }
}

// The iterate a solve starts from, into P.Y: initMat(Y, 1000) (:710), or for a
// warm solve y0 -- the handle's own P.Y0, which no path writes, so a path that
// falls back to another starts from it again.
hipError_t start_iterate(pqp_problem& P, const float* y0, hipStream_t s) {
    if (!y0) return launch_fill(P.Y.f(), 1000.0f, P.N, s);
    return hipMemcpyAsync(P.Y.p, y0, sizeof(float) * P.N, hipMemcpyDeviceToDevice, s);
}

// Fixed mode of a problem with N <= persist_max_n(): every update in ONE
// persistent launch (pqp_persist.hip), launches of at most kPersistChunk
// updates chained through P.Y.
constexpr long long kPersistChunk = 1 << 16;
int problem_run_fixed_persist(pqp_problem& P, long long updates, const float* y0, SolveOut& out, hipStream_t s) {
    const int N = P.N;
    PQP_TRY(ensure_persist_split(P, s));
    auto& ps = P.d.persist;
    float* Yb = P.d.Yb.f();
    auto* gran = static_cast<unsigned long long*>(ps.gran.p);
    int* err = static_cast<int*>(ps.err.p);
    PQP_HIP(start_iterate(P, y0, s));
    std::lock_guard<std::mutex> one_at_a_time(persist_lock());
    for (long long done = 0; done < updates;) {
        const long long n = std::min(kPersistChunk, updates - done);
        // the launch reads its initial iterate from Yb while it writes P.Y
        PQP_HIP(hipMemcpyAsync(Yb, P.Y.p, sizeof(float) * N, hipMemcpyDeviceToDevice, s));
        PQP_HIP(launch_split_persist(ps.SP.f(), ps.fdpn.f(), N, (int)n, Yb, P.Y.f(), gran, err, s));
        int herr = 0;
        PQP_HIP(hipMemcpyAsync(&herr, err, sizeof herr, hipMemcpyDeviceToHost, s));
        PQP_HIP(hipStreamSynchronize(s));
        if (herr) {  // not all workgroups resident (other work on the device): fall back
            set_error(PQP_ERR_HIP, "persistent fixed-mode update: workgroup hand-off timed out (code %d); "
                      "its %d workgroups must be resident at once", herr, (2 * N + 31) / 32);
            return kPersistStalled;
        }
        done += n;
    }
    PQP_HIP(hipStreamSynchronize(s));
    out.h = updates + 1;
    out.status = kStatusDone;
    g_last_path = kPathFixedPersist;
    return PQP_OK;
}

// Fixed mode of a large problem: one multi-workgroup launch per update
// (k_split_update / k_lean_relay), from hipGraphs (per-update host launch
// overhead would otherwise exceed the kernel itself): a chunk of kFixedChunk
// updates replayed as often as needed, then a graph of the remainder.
constexpr long long kFixedChunk = 256;  // even: a chunk starts and ends with the iterate in P.Y
int problem_run_fixed_split(pqp_problem& P, long long num_iter, const float* y0, SolveOut& out, hipStream_t s) {
    const int N = P.N;
    const long long updates = num_iter > 1 ? num_iter - 1 : 0;  // while(h < NUM_ITER)
    // one persistent launch when its workgroups can all be resident; if one of
    // its waits still expires (CUs held by other work), the solve restarts on
    // the graph-replayed relay below (from Y = 1000 again, or a warm solve's y0)
    if (!g_tune.persist_off && N <= persist_max_n() && split_persist_fits(N)) {
        const int rc = problem_run_fixed_persist(P, updates, y0, out, s);
        if (rc != kPersistStalled) return rc;
        ++g_persist_fallbacks;
    }
    const int lw = pick_lw(N);
    PQP_TRY(ensure_split(P, lw, s));
    auto& R = P.d.relay;
    // every setting the captured launches bake in as an argument, the relay
    // wait budget's value included
    const long long variant = ((long long)lw << 8) | ((long long)use_lean(N, N) << 16) |
                              ((long long)(unsigned)g_tune.relay_spin_max << 24);
    if (R.graph_variant != variant) {  // kernel selection changed: recapture both
        R.graph_updates = -1;
        R.chunk_ready = false;
        R.graph_variant = variant;
    }
    const long long full = updates / kFixedChunk, rem = updates % kFixedChunk;
    if (full > 0 && !R.chunk_ready) {
        PQP_TRY(capture_updates(P, kFixedChunk, R.chunk, s));
        R.chunk_ready = true;
    }
    if (rem > 0 && R.graph_updates != rem) {
        PQP_TRY(capture_updates(P, rem, R.rem, s));
        R.graph_updates = rem;
    }
    PQP_HIP(start_iterate(P, y0, s));
    for (long long c = 0; c < full; ++c) PQP_HIP(hipGraphLaunch(R.chunk.exec, s));
    if (rem > 0) PQP_HIP(hipGraphLaunch(R.rem.exec, s));
    int herr = 0;
    PQP_HIP(hipMemcpyAsync(&herr, R.block.err.p, sizeof herr, hipMemcpyDeviceToHost, s));
    PQP_TRY(relay_error_check(R.block.err, &herr, s, "fixed-mode relay update"));
    out.h = updates + 1;
    out.status = kStatusDone;
    g_last_path = kPathFixedRelay;
    return PQP_OK;
}

// Whether converge mode of (N, M) runs as one persistent launch on this device.
bool converge_persist_fits(int N, int M) {
    if (g_tune.converge_persist_off) return false;
    const int G = converge_persist_wgs(N, M, nullptr);
    if (G == 0) return false;
    int dev = 0, cus = 0, lds = 0;
    if (hipGetDevice(&dev) != hipSuccess) return false;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return false;
    if (hipDeviceGetAttribute(&lds, hipDeviceAttributeMaxSharedMemoryPerBlock, dev) != hipSuccess) return false;
    if (converge_persist_lds_bytes(N, M) > (size_t)lds) return false;
    if (g_tune.persist_fit_cus > 0) cus = g_tune.persist_fit_cus;
    // every workgroup of the launch resident at once (its roles wait on each other)
    return (long long)converge_persist_per_cu(N, M) * cus >= G;
}

// Converge mode of a problem with N, M <= 1024 as ONE persistent launch
// (pqp_converge.hip): the update and the stages of terminate() run as
// concurrent roles, terminate(Y_u) beside the update to Y_{u+1}.  Launches
// decide at most g_tune.converge_chunk iterates each and are chained through P.Y.
int problem_run_converge_persist(pqp_problem& P, long long max_updates, const float* y0, SolveOut& out,
                                 hipStream_t s) {
    const int N = P.N, M = P.M;
    PQP_TRY(ensure_persist_split(P, s));
    auto& C = P.d.conv;
    if (!C.A1.p) {
        const size_t n1 = converge_stage_floats(N, M, 1), n2 = converge_stage_floats(N, M, 2),
                     n3 = converge_stage_floats(N, M, 3);
        PQP_TRY(C.A1.floats(n1));
        PQP_TRY(C.A2.floats(n2));
        PQP_TRY(C.A3.floats(n3));
        PQP_HIP(hipMemsetAsync(C.A1.p, 0, sizeof(float) * n1, s));
        PQP_HIP(hipMemsetAsync(C.A2.p, 0, sizeof(float) * n2, s));
        PQP_HIP(hipMemsetAsync(C.A3.p, 0, sizeof(float) * n3, s));
        PQP_HIP(launch_converge_pack(P.Qd.f(), P.Gp.f(), P.Qinv.f(), P.Qp.f(), N, M, C.A1.f(), C.A2.f(), C.A3.f(), s));
        PQP_TRY(C.rings.alloc(sizeof(unsigned long long) * converge_ring_words(N, M)));
        PQP_TRY(C.words.alloc(32));  // ctl, err (int), decided (long long)
    }
    SolveState& st = *P.hst.as<SolveState>();
    st = SolveState{};
    st.h = 1;
    st.status = kStatusContinue;
    SolveState* dst = static_cast<SolveState*>(P.state.p);
    PQP_HIP(hipMemcpyAsync(dst, &st, sizeof st, hipMemcpyHostToDevice, s));
    PQP_HIP(start_iterate(P, y0, s));  // the launch's y_{u0}, u0 = 0: the entry a chunked relaunch takes
    char* words = static_cast<char*>(C.words.p);
    float* hio = P.hio.f();
    ConvergeLaunch L{};
    L.N = N;
    L.M = M;
    L.chunk = g_tune.converge_chunk;
    L.cap = max_updates;
    L.SP = P.d.persist.SP.f();
    L.A1 = C.A1.f();
    L.A2 = C.A2.f();
    L.A3 = C.A3.f();
    L.fdpn = P.d.persist.fdpn.f();
    L.Fp = P.Fp.f();
    L.Kp = P.Kp.f();
    L.Fd = P.Fd.f();
    L.Md = P.Md.f();
    L.Mp = P.Mp.f();
    L.rings = C.rings.p;
    L.st = dst;
    L.ctl = reinterpret_cast<int*>(words);
    L.err = reinterpret_cast<int*>(words + 4);
    L.decided = reinterpret_cast<long long*>(words + 8);
    L.Y = P.Y.f();
    L.U = P.U.f();
    std::lock_guard<std::mutex> one_at_a_time(persist_lock());
    for (long long u0 = 0;;) {
        L.u0 = u0;
        PQP_HIP(launch_converge_persist(L, s));
        int herr = 0;
        // Y and U ride with the state readback (pinned staging, one sync)
        PQP_HIP(hipMemcpyAsync(hio, P.Y.p, sizeof(float) * N, hipMemcpyDeviceToHost, s));
        PQP_HIP(hipMemcpyAsync(hio + N, P.U.p, sizeof(float) * M, hipMemcpyDeviceToHost, s));
        PQP_HIP(hipMemcpyAsync(&st, dst, sizeof st, hipMemcpyDeviceToHost, s));
        PQP_HIP(hipMemcpyAsync(&herr, L.err, sizeof herr, hipMemcpyDeviceToHost, s));
        PQP_HIP(hipStreamSynchronize(s));
        if (herr) {  // not all workgroups resident: the caller re-runs the solve on the graph chain
            set_error(PQP_ERR_HIP, "persistent converge launch: a wait timed out (code %d); its %d workgroups "
                      "must be resident at once", herr, converge_persist_wgs(N, M, nullptr));
            return kPersistStalled;
        }
        if (st.status != kStatusContinue) break;
        u0 = st.h - 1;  // the next launch starts from the iterate this one left in P.Y
    }
    out.staged = true;
    report(st, out);
    out.last_stop = 0;  // on purpose: this path reports no terminate() result, whatever the state holds
    g_last_path = kPathConvergePersist;
    return PQP_OK;
}

// Converge mode of a large problem over many workgroups (pqp_wide.hip): one
// iteration = terminate() as three multi-workgroup mat-vec launches and a
// one-workgroup decision, then the relay update.  Chunks of iterations are
// captured into hipGraphs and replayed until the device-side status leaves
// Continue; launches after that point return at once.
constexpr int kWideChunk = 16;      // even: each replay starts and ends with the iterate in P.Y
constexpr int kWideFirstChunk = 2;  // the first replay of a solve
int problem_run_wide(pqp_problem& P, long long max_updates, const float* y0, SolveOut& out, hipStream_t s,
                     bool try_persist = true) {
    const int N = P.N, M = P.M;
    if (try_persist && converge_persist_fits(N, M)) {
        const int rc = problem_run_converge_persist(P, max_updates, y0, out, s);
        if (rc != kPersistStalled) return rc;
        ++g_persist_fallbacks;  // converge mode restarts (Y = 1000, or y0) on the graph chain
    }
    const int lw = pick_lw(N);
    PQP_TRY(ensure_split(P, lw, s));
    auto& W = P.d.wide;
    if (!W.QinvT.p) {
        PQP_TRY(W.QinvT.floats((size_t)M * M));
        PQP_TRY(W.GpT.floats((size_t)M * N));
        PQP_TRY(W.tM.floats(M));
        PQP_TRY(W.tq.floats(N));
        PQP_TRY(W.tu.floats(M));
        PQP_TRY(W.gu.floats(N));
        PQP_TRY(W.flag.alloc(sizeof(int)));
        PQP_TRY(W.cap.alloc(sizeof(long long)));
        PQP_HIP(launch_transpose(P.Qinv.f(), M, M, W.QinvT.f(), s));  // QinvT[k][i] = Qp_inv[i][k]
        PQP_HIP(launch_transpose(P.Gp.f(), N, M, W.GpT.f(), s));      // GpT[k][i] = Gp[i][k]
    }
    SolveState* dst = static_cast<SolveState*>(P.state.p);
    int* flag = static_cast<int*>(W.flag.p);
    long long* cap = static_cast<long long*>(W.cap.p);
    float* Yb = P.d.Yb.f();
    DevBuf& rerr_word = P.d.relay.block.err;
    int* rerr = static_cast<int*>(rerr_word.p);
    // every launch argument the capture bakes in (cap: a device word)
    const long long key = (long long)(((unsigned long long)(unsigned)g_tune.relay_spin_max << 32) |
                                      ((unsigned long long)use_lean(N, N) << 24) | (unsigned long long)(lw & 0xff));
    if (W.key != key) {
        W.key = -1;  // never a key's value: stays until all four chunks are captured
        // One iteration: terminate()'s launches, then the update, each gated on
        // the status word (once an iteration stops or hits the cap, the rest do
        // nothing).  The update on a forked graph branch beside terminate()
        // measured slower and was removed in round 4.
        auto iteration = [&](const float* cur, float* nxt) -> hipError_t {
            hipError_t e = hipSuccess;
            GemvJobs j1{};  // tmp = Gp'Y + Fp (computeUfromY :354-356) and Y'Qd (computeCost :652, Jd)
            j1.job[0] = GemvJob{P.Gp.f(), cur, W.tM.f(), P.Fp.f(), M, N, M, kEpiAdd};
            j1.job[1] = GemvJob{P.Qd.f(), cur, W.tq.f(), nullptr, N, N, N, kEpiPlain};
            j1.gate = &dst->status;
            j1.err = rerr;
            if ((e = launch_gemv_relay(j1, s)) != hipSuccess) return e;
            GemvJobs j2{};  // U = -(Qp_inv tmp) (:357-358)
            j2.job[0] = GemvJob{W.QinvT.f(), W.tM.f(), P.U.f(), nullptr, M, M, M, kEpiNeg};
            j2.gate = &dst->status;
            j2.err = rerr;
            if ((e = launch_gemv_relay(j2, s)) != hipSuccess) return e;
            GemvJobs j3{};  // checkFeas (:632-641) and U'Qp (computeCost, Jp)
            j3.job[0] = GemvJob{W.GpT.f(), P.U.f(), W.gu.f(), P.Kp.f(), N, M, N, kEpiFeas};
            j3.job[1] = GemvJob{P.Qp.f(), P.U.f(), W.tu.f(), nullptr, M, M, M, kEpiPlain};
            j3.gate = &dst->status;
            j3.flag = flag;
            j3.err = rerr;
            if ((e = launch_gemv_relay(j3, s)) != hipSuccess) return e;
            const WideArgs w{dst, flag, W.tq.f(), W.tu.f(), cur, P.U.f(), P.Fd.f(), P.Fp.f(), P.Md.f(), P.Mp.f(),
                             N, M, cap};
            if ((e = launch_wide_decide(w, s)) != hipSuccess) return e;
            return problem_update(P, cur, nxt, s, &dst->status);
        };
        // replays of 2, 2, 4, 8, then kWideChunk iterations: a solve that stops
        // early launches at most about as many no-op iterations as it ran
        auto capture = [&](int iters, GraphExec& g) -> int {
            return g.capture(s, [&]() -> hipError_t {
                hipError_t e = hipSuccess;
                for (int it = 0; it < iters && e == hipSuccess; it += 2) {
                    e = iteration(P.Y.f(), Yb);
                    if (e == hipSuccess) e = iteration(Yb, P.Y.f());
                }
                return e;
            });
        };
        PQP_TRY(capture(kWideFirstChunk, W.first));
        PQP_TRY(capture(4, W.g4));
        PQP_TRY(capture(8, W.g8));
        PQP_TRY(capture(kWideChunk, W.full));
        W.key = key;
    }
    PQP_HIP(launch_wide_init(dst, flag, cap, max_updates, P.Y.f(), N, s));
    if (y0) PQP_HIP(start_iterate(P, y0, s));  // over the 1000s the init wrote
    SolveState& st = *P.hst.as<SolveState>();
    for (int launch = 0;; ++launch) {
        const GraphExec& g = launch < 2 ? W.first : (launch == 2 ? W.g4 : (launch == 3 ? W.g8 : W.full));
        PQP_HIP(hipGraphLaunch(g.exec, s));
        PQP_HIP(hipMemcpyAsync(&st, dst, sizeof st, hipMemcpyDeviceToHost, s));
        PQP_HIP(hipStreamSynchronize(s));
        if (st.status != kStatusContinue) break;
    }
    if ((st.h - 1) & 1)  // odd number of updates: the iterate is in Yb
        PQP_HIP(hipMemcpyAsync(P.Y.p, Yb, sizeof(float) * N, hipMemcpyDeviceToDevice, s));
    int herr = 0;
    PQP_HIP(hipMemcpyAsync(&herr, rerr, sizeof herr, hipMemcpyDeviceToHost, s));
    PQP_TRY(relay_error_check(rerr_word, &herr, s, "converge-mode relay chain"));
    g_last_path = kPathConvergeWide;
    report(st, out);
    return PQP_OK;
}

// The SolveArgs fields every one-workgroup solve of a handle shares; the
// caller adds its own (QdT, theta, chunk; the one-launch tiny solve's output).
SolveArgs solve_args(const pqp_problem& P, int mode, long long num_iter, long long max_updates) {
    SolveArgs a{};
    a.Qd = P.Qd.f();
    a.Fd = P.Fd.f();
    a.Md = P.Md.f();
    a.Qp = P.Qp.f();
    a.Qinv = P.Qinv.f();
    a.Fp = P.Fp.f();
    a.Mp = P.Mp.f();
    a.Gp = P.Gp.f();
    a.Kp = P.Kp.f();
    a.Y = P.Y.f();
    a.U = P.U.f();
    a.N = P.N;
    a.M = P.M;
    a.ldq = round4(P.N);
    a.ldm = round4(P.M);
    a.mode = mode;
    a.num_iter = num_iter;
    a.max_updates = max_updates;
    return a;
}

// One small problem (N, M <= 32) from Y = 1000 in ONE launch (pqp_tiny.hip:
// k_fixed_one / k_solve_quintet): the kernel starts from h = 1 itself (no state
// upload) and writes Y, U, the state and its error word to pinned host memory,
// so a solve is one launch and one synchronisation, no copy kernels.
int problem_run_tiny(pqp_problem& P, int mode, long long num_iter, long long max_updates, const float* y0,
                     SolveOut& out, hipStream_t s) {
    const int N = P.N, M = P.M;
    if (!P.hout.p) {
        // fine-grained (coherent) host memory: the kernel's stores reach it
        // without a cache write-back at the kernel's end
        PQP_TRY(P.hout.reserve(sizeof(float) * kTinyOutFloats, hipHostMallocMapped | hipHostMallocCoherent));
        std::memset(P.hout.p, 0, sizeof(float) * kTinyOutFloats);  // tag 0: no launch's
    }
    float* hout = P.hout.f();
    SolveArgs a = solve_args(P, mode, num_iter, max_updates);
    // about 2^26 element updates per launch (28.5 k iterates at the bundled
    // size, so its solves stay one launch); the tiny_chunk knob sets it for
    // the resume tests
    a.chunk = g_tune.tiny_chunk > 0 ? g_tune.tiny_chunk : updates_per_launch(N, M, 1 << 26, 1024);
    a.fresh = 1;
    if (y0) {  // a warm start enters as a chunked relaunch does: the device state (h = 1) and its iterate
        SolveState& st = *P.hst.as<SolveState>();
        st = SolveState{};
        st.h = 1;
        st.resume = 1;
        PQP_HIP(hipMemcpyAsync(P.state.p, &st, sizeof st, hipMemcpyHostToDevice, s));
        PQP_HIP(start_iterate(P, y0, s));
        a.fresh = 0;
    }
    a.hout = P.hout.dev;
    a.tiny_flags = (g_tune.tiny_dense ? kTinyDense : 0) | (g_tune.tiny_stall ? kTinyStall : 0);
    a.trace = g_tune.tiny_trace;  // k_solve_quintet timing (bundled size only): 4 words per wave
    SolveState* dst = static_cast<SolveState*>(P.state.p);
    const SolveState* hs = reinterpret_cast<const SolveState*>(hout + kTinyOutStateOffset);
    const int* herr = reinterpret_cast<const int*>(hout) + kTinyOutErrOffset;
    volatile const int* htag = reinterpret_cast<const int*>(hout) + kTinyOutTagOffset;
    for (;;) {
        P.out_tag = (P.out_tag + 1) & 0x7fffffffu;  // positive, never 0 (the zeroed buffer's tag)
        if (P.out_tag == 0) P.out_tag = 1;
        a.out_tag = (int)P.out_tag;
        PQP_HIP(launch_one_tiny(a, dst, s));
        // (polling hipStreamQuery instead measured 2 us slower per solve, 17.7 vs
        // 12.2 us for a bare launch: profiles/r06/doorbell_r06e.json)
        PQP_HIP(hipStreamSynchronize(s));
        if (*htag != a.out_tag || g_tune.tiny_fallback) {
            // not this launch's output (never seen so far; the tiny_fallback
            // knob forces this path in tests): read the device copies instead --
            // Y, U, the state and the error word behind it
            ++g_tiny_stale;
            PQP_HIP(hipMemcpyAsync(hout, P.Y.p, sizeof(float) * N, hipMemcpyDeviceToHost, s));
            if (mode == kModeConverge)
                PQP_HIP(hipMemcpyAsync(hout + kTinyOutUOffset, P.U.p, sizeof(float) * M, hipMemcpyDeviceToHost, s));
            PQP_HIP(hipMemcpyAsync(hout + kTinyOutStateOffset, dst, sizeof(SolveState), hipMemcpyDeviceToHost, s));
            PQP_HIP(hipMemcpyAsync(hout + kTinyOutErrOffset, reinterpret_cast<const char*>(dst) + kTinyDevErr,
                                   sizeof(int), hipMemcpyDeviceToHost, s));
            PQP_HIP(hipStreamSynchronize(s));
        }
        if (*herr) return set_error(PQP_ERR_HIP, "k_solve_quintet: a wave's hand-off wait expired (N=%d, M=%d)", N, M);
        if (hs->status != kStatusContinue) break;
        a.fresh = 0;  // (a chunk ran out) resume from the device state
    }
    std::memcpy(P.hio.p, hout, sizeof(float) * N);
    if (mode == kModeConverge) std::memcpy(P.hio.f() + N, hout + kTinyOutUOffset, sizeof(float) * M);
    out.staged = true;
    report(*hs, out);
    g_last_path = kPathOneWorkgroup;
    return PQP_OK;
}

// Route a solve to its path; the rest of this function is the one-workgroup
// solver (k_solve_tiny / _small / _single) run until it reports Done/Capped.
// Each launch is bounded (chunk updates) so no launch runs unbounded.
// `resume` = start from P.Y instead of Y = 1000 (used by the terminate()
// drop-in, mode 2).  `y0` (device, not P.Y) = a warm start: the solve takes
// the path a cold one takes and starts from y0 instead of Y = 1000.
int problem_run(pqp_problem& P, int mode, long long num_iter, long long max_updates, bool resume, SolveOut& out,
                hipStream_t s, const float* y0 = nullptr) {
    const int N = P.N, M = P.M;
    if (mode == kModeFixed && !P.small && !g_tune.force_single && !resume)
        return problem_run_fixed_split(P, num_iter, y0, out, s);
    if (mode == kModeConverge && !g_tune.force_single && !resume) {
        // the one-wave solver stays fastest for N, M <= 32 (0.65 us per iteration
        // at 32/16 against 2.3 on the persistent launch); from n_dual 48 up the
        // persistent launch wins (scripts/converge_crossover.py)
        const bool tiny = N <= 32 && M <= 32 && !g_tune.force_small;
        const bool wide_ok = N >= g_tune.wide_min_n && (!P.small || g_tune.wide_min_n <= 0);
        if (!tiny && converge_persist_fits(N, M)) {
            const int rc = problem_run_converge_persist(P, max_updates, y0, out, s);
            if (rc != kPersistStalled) return rc;
            ++g_persist_fallbacks;  // the solve restarts (Y = 1000, or y0) below
            if (wide_ok) return problem_run_wide(P, max_updates, y0, out, s, false);
        } else if (wide_ok) {
            return problem_run_wide(P, max_updates, y0, out, s);
        }
    }
    if (!resume && !g_tune.tiny_old && N <= 32 && M <= 32 && !g_tune.force_small && !g_tune.force_single &&
        (mode == kModeFixed || (mode == kModeConverge && N + M < 64)))
        return problem_run_tiny(P, mode, num_iter, max_updates, y0, out, s);
    if (!P.small) PQP_TRY(ensure_single(P, s));
    SolveState& st = *P.hst.as<SolveState>();
    st = SolveState{};
    st.h = 1;
    st.resume = resume || y0 ? 1 : 0;
    PQP_HIP(hipMemcpyAsync(P.state.p, &st, sizeof st, hipMemcpyHostToDevice, s));
    if (y0) PQP_HIP(start_iterate(P, y0, s));
    SolveArgs a = solve_args(P, mode, num_iter, max_updates);
    a.QdT = P.d.QdT.f();
    a.theta = P.d.theta.f();
    a.chunk = updates_per_launch(N, M, 1 << 26, 1);
    SolveState* dst = static_cast<SolveState*>(P.state.p);
    float* hio = P.hio.f();
    for (;;) {
        if (P.N <= 32 && P.M <= 32 && !g_tune.force_small)
            PQP_HIP(launch_solve_tiny(a, dst, s));
        else if (P.small)
            PQP_HIP(launch_solve_small(a, dst, s));
        else
            PQP_HIP(launch_solve_single(a, dst, s));
        // Y and U ride with the state readback (pinned, one sync per launch);
        // the copies of the launch that finishes are the ones that stand
        PQP_HIP(hipMemcpyAsync(hio, P.Y.p, sizeof(float) * N, hipMemcpyDeviceToHost, s));
        PQP_HIP(hipMemcpyAsync(hio + N, P.U.p, sizeof(float) * M, hipMemcpyDeviceToHost, s));
        PQP_HIP(hipMemcpyAsync(&st, dst, sizeof st, hipMemcpyDeviceToHost, s));
        PQP_HIP(hipStreamSynchronize(s));
        if (st.status != kStatusContinue) break;
    }
    out.staged = true;
    report(st, out);
    g_last_path = kPathOneWorkgroup;
    return PQP_OK;
}

[[noreturn]] void die(const char* fn) {
    std::fprintf(stderr, "libpqp: %s failed: %s\n", fn, pqp_last_error());
    std::exit(EXIT_FAILURE);
}

int check_dims(int N, int M) {
    if (N <= 0 || M <= 0) return set_error(PQP_ERR_ARG, "N and M must be positive (N=%d, M=%d)", N, M);
    return PQP_OK;
}

// The device a create call (`fn` in messages) makes its handle on: `device`, or the current one for device < 0.
int resolve_device(const char* fn, int device, int* dev) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return set_error(PQP_ERR_NO_DEVICE, "libpqp: no HIP device visible");
    if (device < 0 && hipGetDevice(&device) != hipSuccess)
        return set_error(PQP_ERR_NO_DEVICE, "libpqp: cannot query the current device");
    if (device >= n) return set_error(PQP_ERR_ARG, "%s: device %d of %d", fn, device, n);
    *dev = device;
    return PQP_OK;
}

// A plant's core on the current device: the three inputs uploaded, and what every state shares derived once, by
// the launchers the batched entry points use (B = 1).  want_sym: then Qd's bit symmetry, by their kernel too.
// The stream is idle when it returns: the host arrays and the Gauss_Jordan scratch are free.
int derive_plant_core(PlantCore& c, int N, int M, const float* Qp_inv, const float* Gp, const float* Kp, bool want_sym,
                      hipStream_t s) {
    PQP_TRY(upload(c.Qinv, Qp_inv, (size_t)M * M, s));
    PQP_TRY(upload(c.Gp, Gp, (size_t)N * M, s));
    PQP_TRY(upload(c.Kp, Kp, N, s));
    PQP_TRY(c.Qp.floats((size_t)M * M));
    PQP_TRY(c.Qd.floats((size_t)N * N));
    PQP_TRY(c.GQ.floats((size_t)N * M));
    PQP_TRY(c.theta.floats(N));
    DevBuf aug, fac, symd;
    PQP_TRY(aug.floats(gauss_jordan_aug_floats(M)));
    PQP_TRY(fac.floats(M));
    const long long nm = (long long)N * M, mm = (long long)M * M, nn = (long long)N * N;
    PQP_HIP(launch_gauss_jordan_b(1, c.Qinv.f(), aug.f(), fac.f(), c.Qp.f(), M, s));                     // Qp :251
    PQP_HIP(launch_matmul_seq_b(1, c.GQ.f(), c.Gp.f(), 0, c.Qinv.f(), 0, N, M, M, nm, mm, nm, s));      // Gp Qp_inv :492
    PQP_HIP(launch_matmul_seq_b(1, c.Qd.f(), c.GQ.f(), 0, c.Gp.f(), 1, N, M, N, nm, nm, nn, s));        // Qd :440-455
    PQP_HIP(launch_theta_rows(c.Qd.f(), N, N, N, c.theta.f(), s));                                      // Theta :503-519
    int hsym = 0;
    if (want_sym) {
        PQP_TRY(symd.alloc(sizeof(int)));
        PQP_HIP(launch_check_symmetric(1, c.Qd.f(), N, static_cast<int*>(symd.p), s));
        PQP_HIP(hipMemcpyAsync(&hsym, symd.p, sizeof(int), hipMemcpyDeviceToHost, s));
    }
    PQP_HIP(hipStreamSynchronize(s));
    c.sym = hsym != 0 ? 1 : 0;
    return PQP_OK;
}

// The three arrays both plant handles' _get download (each optional); the caller synchronises.
int download_plant_core(const PlantCore& c, int N, int M, float* Qd, float* Qp, float* theta, hipStream_t s) {
    if (Qd) PQP_TRY(download(Qd, c.Qd.p, (size_t)N * N, s));
    if (Qp) PQP_TRY(download(Qp, c.Qp.p, (size_t)M * M, s));
    if (theta) PQP_TRY(download(theta, c.theta.p, N, s));
    return PQP_OK;
}

}  // namespace
}  // namespace pqp

using namespace pqp;

extern "C" {

int pqp_version(void) { return 114; }  // ABI revision: INTEGRATION.md section 6

// ---------------------------------------------------------------------------
// 2a. status-returning host API
// ---------------------------------------------------------------------------
int pqp_problem_create_on(int device, void* stream, const float* Qd, const float* Fd, const float* Md,
                          const float* Qp, const float* Qp_inv, const float* Fp, const float* Mp, const float* Gp,
                          const float* Kp, int N, int M, pqp_problem** out) {
    if (!out) return set_error(PQP_ERR_ARG, "pqp_problem_create: null handle pointer");
    *out = nullptr;
    PQP_TRY(check_dims(N, M));
    if (!Qd || !Fd || !Md || !Qp || !Qp_inv || !Fp || !Mp || !Gp || !Kp)
        return set_error(PQP_ERR_ARG, "pqp_problem_create: null input");
    PQP_TRY(resolve_device("pqp_problem_create_on", device, &device));
    DeviceGuard on(device);
    PQP_TRY(ensure_device());
    std::unique_ptr<pqp_problem> P(new pqp_problem());
    P->dev = device;
    if (stream) {
        hipDevice_t sdev = -1;
        PQP_HIP(hipStreamGetDevice(static_cast<hipStream_t>(stream), &sdev));
        if (sdev != device)
            return set_error(PQP_ERR_ARG, "pqp_problem_create_on: the stream belongs to device %d, not %d", (int)sdev,
                             device);
        P->stream = static_cast<hipStream_t>(stream);
    } else {
        PQP_HIP(hipStreamCreateWithFlags(&P->stream, hipStreamNonBlocking));
        P->own_stream = true;
    }
    hipStream_t s = P->stream;
    int rc = problem_upload(*P, Qd, Fd, Md, Qp, Qp_inv, Fp, Mp, Gp, Kp, N, M, s);
    if (rc == PQP_OK && hipStreamSynchronize(s) != hipSuccess) rc = set_error(PQP_ERR_HIP, "problem setup failed");
    if (rc != PQP_OK) return rc;
    *out = P.release();
    return PQP_OK;
}

int pqp_problem_create(const float* Qd, const float* Fd, const float* Md, const float* Qp, const float* Qp_inv,
                       const float* Fp, const float* Mp, const float* Gp, const float* Kp, int N, int M,
                       pqp_problem** out) {
    return pqp_problem_create_on(-1, nullptr, Qd, Fd, Md, Qp, Qp_inv, Fp, Mp, Gp, Kp, N, M, out);
}

int pqp_problem_device(const pqp_problem* P) { return P ? P->dev : set_error(PQP_ERR_ARG, "pqp_problem_device: null handle"); }

int pqp_problem_solve(pqp_problem* P, int mode, long long num_iter, long long max_updates, float* Y, float* U,
                      long long* h_out, float* Jp_out, float* Jd_out) {
    return pqp_problem_solve_from(P, PQP_START_COLD, nullptr, mode, num_iter, max_updates, Y, U, h_out, Jp_out,
                                  Jd_out);
}

int pqp_problem_solve_from(pqp_problem* P, int start, const float* Y0, int mode, long long num_iter,
                           long long max_updates, float* Y, float* U, long long* h_out, float* Jp_out,
                           float* Jd_out) {
    if (!P || !Y) return set_error(PQP_ERR_ARG, "pqp_problem_solve: null handle or Y");
    if (mode != PQP_MODE_CONVERGE && mode != PQP_MODE_FIXED)
        return set_error(PQP_ERR_ARG, "pqp_problem_solve: unknown mode %d", mode);
    if (start != PQP_START_COLD && start != PQP_START_HOST && start != PQP_START_LAST)
        return set_error(PQP_ERR_ARG, "pqp_problem_solve_from: unknown start %d", start);
    if (start == PQP_START_HOST && !Y0) return set_error(PQP_ERR_ARG, "pqp_problem_solve_from: PQP_START_HOST needs Y0");
    std::lock_guard<std::mutex> lk(P->mu);
    if (start == PQP_START_LAST && !P->has_last)
        return set_error(PQP_ERR_ARG, "pqp_problem_solve_from: PQP_START_LAST before the handle's first solve");
    DeviceGuard on(P->dev);
    PQP_TRY(ensure_device());
    hipStream_t s = P->stream;
    // the starting iterate in a buffer of its own: the paths write P.Y
    const float* y0 = nullptr;
    if (start == PQP_START_HOST) {
        std::memcpy(P->hio.p, Y0, sizeof(float) * P->N);  // through the pinned staging buffer
        PQP_HIP(hipMemcpyAsync(P->Y0.p, P->hio.p, sizeof(float) * P->N, hipMemcpyHostToDevice, s));
        y0 = P->Y0.f();
    } else if (start == PQP_START_LAST) {
        PQP_HIP(hipMemcpyAsync(P->Y0.p, P->Y.p, sizeof(float) * P->N, hipMemcpyDeviceToDevice, s));
        y0 = P->Y0.f();
    }
    P->has_last = false;  // until this solve has left its final iterate in P.Y
    SolveOut o;
    PQP_TRY(problem_run(*P, mode == PQP_MODE_CONVERGE ? kModeConverge : kModeFixed, num_iter, max_updates, false, o,
                        s, y0));
    P->has_last = true;
    const bool want_u = U && mode == PQP_MODE_CONVERGE;
    float* hio = P->hio.f();
    if (!o.staged) {  // through the pinned staging buffer: one sync, no pageable DMA
        PQP_HIP(hipMemcpyAsync(hio, P->Y.p, sizeof(float) * P->N, hipMemcpyDeviceToHost, s));
        if (want_u) PQP_HIP(hipMemcpyAsync(hio + P->N, P->U.p, sizeof(float) * P->M, hipMemcpyDeviceToHost, s));
        PQP_HIP(hipStreamSynchronize(s));
    }
    std::memcpy(Y, hio, sizeof(float) * P->N);
    if (want_u) std::memcpy(U, hio + P->N, sizeof(float) * P->M);
    if (h_out) *h_out = o.h;
    if (Jp_out) *Jp_out = o.Jp;
    if (Jd_out) *Jd_out = o.Jd;
    if (o.status == kStatusCapped)
        return set_error(PQP_ERR_NOT_CONVERGED, "no convergence within %lld updates (h=%lld)", max_updates, o.h);
    return PQP_OK;
}

int pqp_problem_destroy(pqp_problem* P) {
    if (!P) return PQP_OK;
    {
        std::lock_guard<std::mutex> lk(P->mu);  // a solve still running on another thread ends first
        DeviceGuard on(P->dev);
        if (P->stream) (void)hipStreamSynchronize(P->stream);
    }
    DeviceGuard on(P->dev);
    delete P;
    return PQP_OK;
}

// Gp Qp_inv (convertToDual's temporary, PQP_CPU.c:491-492) in k_relin_pack's
// layout, built on the first pqp_problem_update_linear of a problem.
static int ensure_gq(pqp_problem& P, hipStream_t s) {
    if (P.d.GQ.p) return PQP_OK;
    const int N = P.N, M = P.M;
    DevBuf rowmajor, packed;
    PQP_TRY(rowmajor.floats((size_t)N * M));
    PQP_TRY(packed.floats((size_t)N * M));
    PQP_TRY(dev_matmul(rowmajor.f(), P.Gp.f(), 0, P.Qinv.f(), 0, N, M, M, s));  // Gp_Qp_inv :492
    PQP_HIP(launch_relin_pack(1, N, M, rowmajor.f(), packed.f(), s));
    PQP_HIP(hipStreamSynchronize(s));  // before the row-major copy is freed
    P.d.GQ = std::move(packed);
    return PQP_OK;
}

int pqp_problem_update_linear(pqp_problem* P, const float* Fp, const float* Mp, const float* Kp) {
    if (!P || !Fp || !Mp) return set_error(PQP_ERR_ARG, "pqp_problem_update_linear: null handle, Fp or Mp");
    std::lock_guard<std::mutex> lk(P->mu);
    DeviceGuard on(P->dev);
    PQP_TRY(ensure_device());
    hipStream_t s = P->stream;
    const int N = P->N, M = P->M;
    PQP_TRY(ensure_gq(*P, s));
    // in place: buffers of the same size keep their addresses (the captured graphs hold them)
    PQP_TRY(upload(P->Fp, Fp, M, s));
    PQP_TRY(upload(P->Mp, Mp, 1, s));
    if (Kp) PQP_TRY(upload(P->Kp, Kp, N, s));
    PQP_HIP(launch_relinearize(1, N, M, P->d.GQ.f(), P->Qinv.f(), P->Kp.f(), P->Fp.f(), P->Mp.f(), P->Fd.f(),
                               P->Md.f(), s));
    // what the solve paths derived from Fd, where it lives: the 32-lane
    // layout's {Fdn, Fdp} (persistent launches) and the relay block's, which
    // in the lean layout are the first two words of each row's aux
    RelayBlock& rb = P->d.relay.block;
    PQP_HIP(launch_relin_refresh(P->Fd.f(), N, P->d.persist.fdpn.f(), rb.lean ? nullptr : rb.fdpn.f(),
                                 rb.lean ? rb.fdpn.f() : nullptr, s));
    PQP_HIP(hipStreamSynchronize(s));
    return PQP_OK;
}

int pqp_problem_get_dual(pqp_problem* P, float* Fd, float* Md) {
    if (!P) return set_error(PQP_ERR_ARG, "pqp_problem_get_dual: null handle");
    std::lock_guard<std::mutex> lk(P->mu);
    DeviceGuard on(P->dev);
    PQP_TRY(ensure_device());
    hipStream_t s = P->stream;
    if (Fd) PQP_TRY(download(Fd, P->Fd.p, P->N, s));
    if (Md) PQP_TRY(download(Md, P->Md.p, 1, s));
    PQP_HIP(hipStreamSynchronize(s));
    return PQP_OK;
}

static std::mutex g_oneshot_mu;              // guards g_oneshot
static pqp_problem* g_oneshot[64] = {nullptr};  // per device: cached handle of pqp_solve_dual's tiny problems

int pqp_solve_dual(const float* Qd, const float* Fd, const float* Md, const float* Qp, const float* Qp_inv,
                   const float* Fp, const float* Mp, const float* Gp, const float* Kp, int N, int M, int mode,
                   long long num_iter, long long max_updates, float* Y, float* U, long long* h_out,
                   float* Jp_out, float* Jd_out) {
    if (mode != PQP_MODE_CONVERGE && mode != PQP_MODE_FIXED)
        return set_error(PQP_ERR_ARG, "pqp_solve_dual: unknown mode %d", mode);
    if (!Y) return set_error(PQP_ERR_ARG, "pqp_solve_dual: null Y");
    if (N >= 1 && M >= 1 && N <= 32 && M <= 32) {
        // the one-shot form of tiny problems (the reference's own call
        // pattern, solveQuadraticDual per solve) reuses one cached handle: its
        // buffers are re-filled in place (no allocations), and these problems
        // build no derived per-problem data a new Qd could leave stale
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64)
            return set_error(PQP_ERR_NO_DEVICE, "libpqp: cannot query the current device");
        std::lock_guard<std::mutex> lk(g_oneshot_mu);
        pqp_problem*& h = g_oneshot[dev];
        if (!h) {
            PQP_TRY(pqp_problem_create(Qd, Fd, Md, Qp, Qp_inv, Fp, Mp, Gp, Kp, N, M, &h));
        } else {
            if (!Qd || !Fd || !Md || !Qp || !Qp_inv || !Fp || !Mp || !Gp || !Kp)
                return set_error(PQP_ERR_ARG, "pqp_solve_dual: null input");
            std::lock_guard<std::mutex> lk2(h->mu);
            PQP_TRY(ensure_device());
            PQP_TRY(problem_upload(*h, Qd, Fd, Md, Qp, Qp_inv, Fp, Mp, Gp, Kp, N, M, h->stream));
        }
        return pqp_problem_solve(h, mode, num_iter, max_updates, Y, U, h_out, Jp_out, Jd_out);
    }
    pqp_problem* P = nullptr;
    PQP_TRY(pqp_problem_create(Qd, Fd, Md, Qp, Qp_inv, Fp, Mp, Gp, Kp, N, M, &P));
    const int rc = pqp_problem_solve(P, mode, num_iter, max_updates, Y, U, h_out, Jp_out, Jd_out);
    const std::string err = pqp_last_error();
    pqp_problem_destroy(P);
    restore_error(err);
    return rc;
}

int pqp_update_host(const float* Qd, const float* theta_diag, const float* Fd, const float* Y, float* Y_next,
                    int N) {
    if (N <= 0 || !Qd || !theta_diag || !Fd || !Y || !Y_next) return set_error(PQP_ERR_ARG, "pqp_update_host");
    PQP_TRY(ensure_device());
    hipStream_t s = lib_stream();
    const int ldq = round4(N);
    DevBuf dQd, dQdT, dth, dFd, dY, dYn;
    PQP_TRY(upload(dQd, Qd, (size_t)N * N, s));
    PQP_TRY(upload(dth, theta_diag, N, s));
    PQP_TRY(upload(dFd, Fd, N, s));
    PQP_TRY(upload(dY, Y, N, s));
    PQP_TRY(dYn.floats(N));
    PQP_TRY(dQdT.floats((size_t)N * ldq));
    PQP_HIP(launch_pack_colmajor(1, dQd.f(), N, (long long)N * N, dQdT.f(), ldq, (long long)N * ldq, s));
    PQP_HIP(launch_batch_update(1, dQdT.f(), (long long)N * ldq, ldq, N, dth.f(), dFd.f(), N, dY.f(), dYn.f(), s));
    PQP_TRY(download(Y_next, dYn.p, N, s));
    PQP_HIP(hipStreamSynchronize(s));
    return PQP_OK;
}

int pqp_run_example(const char* dir, void* out_file) {
    FILE* out = out_file ? static_cast<FILE*>(out_file) : stdout;
    ExampleData e;
    const int m = kRefNInput * kRefPHorizon, nd = kRefNDis * kRefPHorizon, ns = kRefNState;
    PQP_TRY(read_example(dir, m, nd, ns, e));
    const int M = m, N = 4 * m;
    PQP_TRY(ensure_device());
    hipStream_t s = lib_stream();
    DevBuf Qinv, Fp1, Fp2, Fp3, Mp1, Mp2, Mp3, Mp4, Mp5, Mp6, Gp, Kp, x, D;
    PQP_TRY(upload(Qinv, e.Qp_inv.data(), e.Qp_inv.size(), s));
    PQP_TRY(upload(Fp1, e.Fp1.data(), e.Fp1.size(), s));
    PQP_TRY(upload(Fp2, e.Fp2.data(), e.Fp2.size(), s));
    PQP_TRY(upload(Fp3, e.Fp3.data(), e.Fp3.size(), s));
    PQP_TRY(upload(Mp1, e.Mp1.data(), e.Mp1.size(), s));
    PQP_TRY(upload(Mp2, e.Mp2.data(), e.Mp2.size(), s));
    PQP_TRY(upload(Mp3, e.Mp3.data(), e.Mp3.size(), s));
    PQP_TRY(upload(Mp4, e.Mp4.data(), e.Mp4.size(), s));
    PQP_TRY(upload(Mp5, e.Mp5.data(), e.Mp5.size(), s));
    PQP_TRY(upload(Mp6, e.Mp6.data(), e.Mp6.size(), s));
    PQP_TRY(upload(Gp, e.Gp.data(), e.Gp.size(), s));
    PQP_TRY(upload(Kp, e.Kp.data(), e.Kp.size(), s));
    PQP_TRY(upload(x, e.x.data(), e.x.size(), s));
    PQP_TRY(upload(D, e.D.data(), e.D.size(), s));
    pqp_problem P;
    P.N = N;
    P.M = M;
    DevBuf Jp, Jd;
    PQP_TRY(P.Qp.floats((size_t)M * M));
    PQP_TRY(P.Fp.floats(M));
    PQP_TRY(P.Mp.floats(1));
    PQP_TRY(P.Qd.floats((size_t)N * N));
    PQP_TRY(P.Fd.floats(N));
    PQP_TRY(P.Md.floats(1));
    PQP_TRY(Jp.floats(1));
    PQP_TRY(Jd.floats(1));
    P.Qinv = std::move(Qinv);
    P.Gp = std::move(Gp);
    P.Kp = std::move(Kp);
    PQP_TRY(dev_gauss_jordan(P.Qp.f(), P.Qinv.f(), M, s));                                                // :989
    PQP_TRY(dev_compute_fp(P.Fp.f(), Fp1.f(), Fp2.f(), Fp3.f(), D.f(), x.f(), m, nd, ns, s));            // :991
    PQP_TRY(dev_compute_mp(P.Mp.f(), Mp1.f(), Mp2.f(), Mp3.f(), Mp4.f(), Mp5.f(), Mp6.f(), D.f(), x.f(), nd, ns,
                           s));                                                                         // :992
    PQP_TRY(dev_convert_to_dual(P.Qd.f(), P.Fd.f(), P.Md.f(), P.Qinv.f(), P.Gp.f(), P.Kp.f(), P.Fp.f(), P.Mp.f(), N,
                                M, s));                                                                 // :994
    PQP_TRY(problem_finish(P, s));
    SolveOut o;
    PQP_TRY(problem_run(P, kModeConverge, 0, 0, false, o, s));                                          // :996
    std::fprintf(out, "Printing number of iterations = %ld\n", (long)o.h);                              // :741
    float* U = P.U.f();
    float* Y = P.Y.f();
    PQP_TRY(dev_u_from_y(U, Y, P.Fp.f(), P.Gp.f(), P.Qinv.f(), N, M, s));                                // :999
    PQP_TRY(dev_cost(Jp.f(), U, P.Qp.f(), P.Fp.f(), P.Mp.f(), M, s));                                    // :1002
    PQP_TRY(dev_cost(Jd.f(), Y, P.Qd.f(), P.Fd.f(), P.Md.f(), N, s));                                    // :1003
    std::vector<float> hU(M);
    float jp = 0, jd = 0;
    PQP_TRY(download(hU.data(), U, M, s));
    PQP_TRY(download(&jp, Jp.p, 1, s));
    PQP_TRY(download(&jd, Jd.p, 1, s));
    PQP_HIP(hipStreamSynchronize(s));
    std::fprintf(out, "Jp = %f\n", jp);
    std::fprintf(out, "Jd = %f\n", jd);
    std::fprintf(out, "Printing U*\n");
    for (int i = 0; i < M; ++i) std::fprintf(out, "\t%f\n", hU[i]);
    std::fflush(out);
    return PQP_OK;
}

// ---------------------------------------------------------------------------
// 2b. batched device API
// ---------------------------------------------------------------------------
static int check_batch(int B, int N, const void* QdT, int ldq, long long qstride, int ldv) {
    if (B <= 0 || N <= 0) return set_error(PQP_ERR_ARG, "B and N must be positive (B=%d, N=%d)", B, N);
    if (!QdT || (reinterpret_cast<uintptr_t>(QdT) & 15))
        return set_error(PQP_ERR_ARG, "QdT must be a 16-byte aligned device pointer");
    if (ldq < N || (ldq & 3)) return set_error(PQP_ERR_ARG, "ldq (%d) must be >= N (%d) and a multiple of 4", ldq, N);
    if (qstride < (long long)N * ldq || (qstride & 3))
        return set_error(PQP_ERR_ARG, "qstride (%lld) must be >= N*ldq and a multiple of 4", qstride);
    if (ldv < N) return set_error(PQP_ERR_ARG, "ldv (%d) must be >= N (%d)", ldv, N);
    return ensure_device();
}

int pqp_batch_generate(uint32_t seed, long long inst0, int B, int N, int M, float* d_QdT, int ldq,
                       long long qstride, float* d_Fd, float* d_Md, float* d_theta, int ldv, void* stream) {
    PQP_TRY(check_batch(B, N, d_QdT, ldq, qstride, ldv));
    if (M <= 0 || !d_Fd || !d_theta) return set_error(PQP_ERR_ARG, "pqp_batch_generate: bad M or null output");
    hipStream_t s = static_cast<hipStream_t>(stream);
    PQP_HIP(launch_synth(seed, inst0, B, N, M, d_QdT, ldq, qstride, d_Fd, ldv, d_Md, s));
    PQP_HIP(launch_theta(B, d_QdT, ldq, qstride, N, d_theta, ldv, s));
    return PQP_OK;
}

int pqp_batch_synth_primal(uint32_t seed, long long inst0, int B, int N, int M, float* d_Qp_inv, float* d_Gp,
                           float* d_Kp, float* d_Fp, float* d_Mp, void* stream) {
    if (B <= 0 || N <= 0 || M <= 0 || !d_Qp_inv || !d_Gp || !d_Kp || !d_Fp || !d_Mp)
        return set_error(PQP_ERR_ARG, "pqp_batch_synth_primal: bad arguments");
    PQP_TRY(ensure_device());
    PQP_HIP(launch_synth_primal(seed, inst0, B, N, M, d_Qp_inv, d_Gp, d_Kp, d_Fp, d_Mp,
                                static_cast<hipStream_t>(stream)));
    return PQP_OK;
}

int pqp_batch_pack(int B, int N, const float* d_Qd, float* d_QdT, int ldq, long long qstride, void* stream) {
    PQP_TRY(check_batch(B, N, d_QdT, ldq, qstride, N));
    if (!d_Qd) return set_error(PQP_ERR_ARG, "pqp_batch_pack: null input");
    PQP_HIP(launch_pack_colmajor(B, d_Qd, N, (long long)N * N, d_QdT, ldq, qstride, static_cast<hipStream_t>(stream)));
    return PQP_OK;
}

int pqp_batch_theta(int B, int N, const float* d_QdT, int ldq, long long qstride, float* d_theta, int ldv,
                    void* stream) {
    PQP_TRY(check_batch(B, N, d_QdT, ldq, qstride, ldv));
    if (!d_theta) return set_error(PQP_ERR_ARG, "pqp_batch_theta: null output");
    PQP_HIP(launch_theta(B, d_QdT, ldq, qstride, N, d_theta, ldv, static_cast<hipStream_t>(stream)));
    return PQP_OK;
}

int pqp_batch_update(int B, int N, const float* d_QdT, int ldq, long long qstride, const float* d_theta,
                     const float* d_Fd, int ldv, const float* d_Y, float* d_Ynext, void* stream) {
    PQP_TRY(check_batch(B, N, d_QdT, ldq, qstride, ldv));
    if (!d_theta || !d_Fd || !d_Y || !d_Ynext) return set_error(PQP_ERR_ARG, "pqp_batch_update: null pointer");
    if (d_Y == d_Ynext) return set_error(PQP_ERR_ARG, "pqp_batch_update: d_Y and d_Ynext must not alias");
    if ((size_t)ldq * sizeof(float) > 150 * 1024) return set_error(PQP_ERR_ARG, "pqp_batch_update: N too large");
    PQP_HIP(launch_batch_update(B, d_QdT, qstride, ldq, N, d_theta, d_Fd, ldv, d_Y, d_Ynext,
                                static_cast<hipStream_t>(stream)));
    return PQP_OK;
}

int pqp_batch_iterate(int B, int N, const float* d_QdT, int ldq, long long qstride, const float* d_theta,
                      const float* d_Fd, int ldv, const float* d_Y0, float* d_Y, int updates, void* stream) {
    PQP_TRY(check_batch(B, N, d_QdT, ldq, qstride, ldv));
    if (!d_theta || !d_Fd || !d_Y || updates < 0) return set_error(PQP_ERR_ARG, "pqp_batch_iterate: bad argument");
    if ((size_t)2 * ldq * sizeof(float) > 160 * 1024)
        return set_error(PQP_ERR_ARG, "pqp_batch_iterate: ldq=%d needs more than 160 KiB of LDS", ldq);
    PQP_HIP(launch_batch_iterate(B, d_QdT, qstride, ldq, N, d_theta, d_Fd, ldv, d_Y0, d_Y, updates,
                                 static_cast<hipStream_t>(stream)));
    return PQP_OK;
}

int pqp_batch_iterate_sym(int B, int N, const float* d_QdT, int ldq, long long qstride, const float* d_theta,
                          const float* d_Fd, int ldv, const float* d_Y0, float* d_Y, int updates, void* stream) {
    PQP_TRY(check_batch(B, N, d_QdT, ldq, qstride, ldv));
    if (!d_theta || !d_Fd || !d_Y || updates < 0)
        return set_error(PQP_ERR_ARG, "pqp_batch_iterate_sym: bad argument");
    if ((size_t)2 * ldq * sizeof(float) > 160 * 1024)
        return set_error(PQP_ERR_ARG, "pqp_batch_iterate_sym: ldq=%d needs more than 160 KiB of LDS", ldq);
    PQP_HIP(launch_batch_iterate_sym(B, d_QdT, qstride, ldq, N, d_theta, d_Fd, ldv, d_Y0, d_Y, updates,
                                     static_cast<hipStream_t>(stream)));
    return PQP_OK;
}

// B states of one problem (pqp.h 2b'): k_batch_shared
int pqp_batch_shared_states(int N, int ldq) { return pqp::batch_shared_states(N, ldq); }

int pqp_batch_iterate_shared(int B, int N, const float* d_QdT, int ldq, const float* d_theta, const float* d_Fd,
                             int ldv, const float* d_Y0, float* d_Y, int updates, void* stream) {
    // check_batch's rules for one problem's QdT, and this entry point's own, before any device is looked for
    if (B <= 0 || N <= 0) return set_error(PQP_ERR_ARG, "B and N must be positive (B=%d, N=%d)", B, N);
    if (!d_QdT || (reinterpret_cast<uintptr_t>(d_QdT) & 15))
        return set_error(PQP_ERR_ARG, "QdT must be a 16-byte aligned device pointer");
    if (ldq < N || (ldq & 3)) return set_error(PQP_ERR_ARG, "ldq (%d) must be >= N (%d) and a multiple of 4", ldq, N);
    if (ldv < N) return set_error(PQP_ERR_ARG, "ldv (%d) must be >= N (%d)", ldv, N);
    if (updates < 0) return set_error(PQP_ERR_ARG, "pqp_batch_iterate_shared: updates (%d) must be >= 0", updates);
    if (!d_theta || !d_Fd || !d_Y) return set_error(PQP_ERR_ARG, "pqp_batch_iterate_shared: null pointer");
    if (pqp::batch_shared_states(N, ldq) == 0)
        return set_error(PQP_ERR_ARG, "pqp_batch_iterate_shared: ldq=%d is not supported: 8 states need 64*ldq bytes "
                                      "of LDS, the limit is 160 KiB (ldq <= 2560)", ldq);
    PQP_TRY(ensure_device());
    PQP_HIP(launch_batch_shared(B, d_QdT, ldq, N, d_theta, d_Fd, ldv, d_Y0, d_Y, updates,
                                static_cast<hipStream_t>(stream)));
    return PQP_OK;
}

int pqp_batch_symmetric(int B, int N, const float* d_QdT, int ldq, long long qstride, int* d_sym, int* all_sym_out,
                        void* stream) {
    if (all_sym_out) *all_sym_out = 0;
    PQP_TRY(check_batch(B, N, d_QdT, ldq, qstride, N));
    hipStream_t s = static_cast<hipStream_t>(stream);
    DevBuf own;  // the flags, where the caller keeps none
    int* sym = d_sym;
    if (!sym) {
        PQP_TRY(own.alloc(sizeof(int) * (size_t)B));
        sym = static_cast<int*>(own.p);
    }
    PQP_HIP(launch_check_symmetric_ld(B, d_QdT, N, ldq, qstride, sym, s));
    std::vector<int> flags((size_t)B);
    PQP_HIP(hipMemcpyAsync(flags.data(), sym, sizeof(int) * (size_t)B, hipMemcpyDeviceToHost, s));
    PQP_HIP(hipStreamSynchronize(s));
    bool all_sym = true;
    for (int v : flags) all_sym = all_sym && v != 0;
    if (all_sym_out) *all_sym_out = all_sym ? 1 : 0;
    return PQP_OK;
}

// ---------------------------------------------------------------------------
// 2d. row blocks of one large problem (row-sharded solve)
// ---------------------------------------------------------------------------
int pqp_rowblock_create(const float* d_Qd_rows, int ld, const float* d_Fd, int N, int row0, int rows, void* stream,
                        pqp_rowblock** out) {
    if (!out) return set_error(PQP_ERR_ARG, "pqp_rowblock_create: null out");
    *out = nullptr;
    if (N <= 0 || ld < N || row0 < 0 || rows < 0 || row0 + (long long)rows > N || !d_Fd || (rows > 0 && !d_Qd_rows))
        return set_error(PQP_ERR_ARG, "pqp_rowblock_create: bad arguments (N=%d ld=%d row0=%d rows=%d)", N, ld, row0,
                         rows);
    if (split_lds_bytes(N) > kLdsBudget)
        return set_error(PQP_ERR_ARG, "pqp_rowblock_create: N=%d needs more than %zu B of LDS", N, kLdsBudget);
    PQP_TRY(ensure_device());
    hipStream_t s = static_cast<hipStream_t>(stream);
    std::unique_ptr<pqp_rowblock> b(new pqp_rowblock);
    PQP_HIP(hipGetDevice(&b->dev));
    b->N = N;
    b->row0 = row0;
    b->rows = rows;
    PQP_TRY(relay_error_word(b->relay, s));  // all an empty block holds
    if (rows > 0) {
        DevBuf theta;
        PQP_TRY(theta.floats(rows));
        PQP_HIP(launch_theta_rows(d_Qd_rows, ld, N, rows, theta.f(), s));
        const int lw = use_lean(N, rows) ? lean_pick_lw(rows) : split_pick_lw(rows);
        PQP_TRY(relay_build(b->relay, d_Qd_rows, ld, theta.f(), d_Fd, N, rows, row0, lw, s));
        PQP_HIP(hipStreamSynchronize(s));  // theta is freed on return
    }
    *out = b.release();
    return PQP_OK;
}

int pqp_rowblock_update(pqp_rowblock* b, const float* d_Y, float* d_Y_rows, void* stream) {
    if (!b || !d_Y || (b->rows > 0 && !d_Y_rows)) return set_error(PQP_ERR_ARG, "pqp_rowblock_update: null argument");
    hipStream_t s = static_cast<hipStream_t>(stream);
    DeviceGuard on(b->dev);
    PQP_HIP(relay_update(b->relay, b->N, b->rows, b->row0, d_Y, d_Y_rows, s));
    return PQP_OK;
}

int pqp_rowblock_check(pqp_rowblock* b, void* stream) {
    if (!b) return set_error(PQP_ERR_ARG, "pqp_rowblock_check: null block");
    hipStream_t s = static_cast<hipStream_t>(stream);
    DeviceGuard on(b->dev);
    int herr = 0;
    PQP_HIP(hipMemcpyAsync(&herr, b->relay.err.p, sizeof herr, hipMemcpyDeviceToHost, s));
    return relay_error_check(b->relay.err, &herr, s, "pqp_rowblock_update");
}

int pqp_rowblock_destroy(pqp_rowblock* b) {
    if (!b) return PQP_OK;
    DeviceGuard on(b->dev);
    delete b;
    return PQP_OK;
}

int pqp_synth_rows(uint32_t seed, long long inst, int N, int M, int row0, int rows, float* d_Qd_rows, int ld,
                   float* d_Fd, float* d_Md, void* stream) {
    if (N <= 0 || M <= 0 || ld < N || row0 < 0 || rows < 0 || row0 + (long long)rows > N || (rows > 0 && !d_Qd_rows))
        return set_error(PQP_ERR_ARG, "pqp_synth_rows: bad arguments (N=%d M=%d ld=%d row0=%d rows=%d)", N, M, ld,
                         row0, rows);
    PQP_TRY(ensure_device());
    PQP_HIP(launch_synth_rows(seed, inst, N, M, row0, rows, d_Qd_rows, ld, d_Fd, d_Md,
                              static_cast<hipStream_t>(stream)));
    return PQP_OK;
}

// ---------------------------------------------------------------------------
// 2c. batched small problems
// ---------------------------------------------------------------------------
int pqp_batch_gauss_jordan(int B, int n, const float* d_A, float* d_res, void* stream) {
    if (B <= 0 || n <= 0 || !d_A || !d_res) return set_error(PQP_ERR_ARG, "pqp_batch_gauss_jordan: bad arguments");
    PQP_TRY(ensure_device());
    hipStream_t s = static_cast<hipStream_t>(stream);
    DevBuf aug, fac;
    PQP_TRY(aug.floats((size_t)B * gauss_jordan_aug_floats(n)));
    PQP_TRY(fac.floats((size_t)B * n));
    PQP_HIP(launch_gauss_jordan_b(B, d_A, aug.f(), fac.f(), d_res, n, s));
    PQP_HIP(hipStreamSynchronize(s));
    return PQP_OK;
}

// One grow-only device workspace per device for the batched setup calls
// (the round-5 form kept one per (thread, device), so a host that
// called from many pooled threads kept one buffer per thread it ever used).
// A call holds its device's lock from the workspace request until its stream
// has synchronised, so concurrent setup calls on one device take turns (each
// one fills the device anyway); no hipMalloc / hipFree (which synchronise the
// device) per call.  pqp_release_workspaces() frees every pool; nothing frees
// them at exit (a static destructor could run after the HIP runtime is gone).
namespace {
struct SetupPool {
    std::mutex mu;
    void* buf = nullptr;
    size_t cap = 0;
};
SetupPool g_setup_pool[64];

class SetupWorkspace {
  public:
    ~SetupWorkspace() {
        if (pool_) pool_->mu.unlock();
    }
    int acquire(size_t floats, float** out) {
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64)
            return set_error(PQP_ERR_NO_DEVICE, "libpqp: cannot query the current device");
        pool_ = &g_setup_pool[dev];
        pool_->mu.lock();
        const size_t bytes = floats * sizeof(float);
        if (pool_->cap < bytes) {
            if (pool_->buf) (void)hipFree(pool_->buf);
            pool_->buf = nullptr;
            pool_->cap = 0;
            const hipError_t e = hipMalloc(&pool_->buf, bytes);
            if (e != hipSuccess) {
                pool_->buf = nullptr;
                return set_error(PQP_ERR_ALLOC, "hipMalloc(%zu bytes): %s", bytes, hipGetErrorString(e));
            }
            pool_->cap = bytes;
        }
        *out = static_cast<float*>(pool_->buf);
        return PQP_OK;
    }

  private:
    SetupPool* pool_ = nullptr;
};
}  // namespace

int pqp_release_workspaces(void) {
    int dev0 = 0;
    const bool restore = hipGetDevice(&dev0) == hipSuccess;
    int rc = PQP_OK;
    for (int d = 0; d < 64; ++d) {
        SetupPool& p = g_setup_pool[d];
        std::lock_guard<std::mutex> g(p.mu);
        if (!p.buf) continue;
        if (hipSetDevice(d) != hipSuccess || hipFree(p.buf) != hipSuccess)
            rc = set_error(PQP_ERR_HIP, "pqp_release_workspaces: hipFree on device %d failed", d);
        p.buf = nullptr;
        p.cap = 0;
    }
    if (restore) (void)hipSetDevice(dev0);
    return rc;
}

int pqp_batch_convert_to_dual(int B, int N, int M, const float* d_Qp_inv, const float* d_Gp, const float* d_Kp,
                              const float* d_Fp, const float* d_Mp, float* d_Qd, float* d_Fd, float* d_Md,
                              void* stream) {
    if (B <= 0 || N <= 0 || M <= 0 || !d_Qp_inv || !d_Gp || !d_Kp || !d_Fp || !d_Mp || !d_Qd || !d_Fd || !d_Md)
        return set_error(PQP_ERR_ARG, "pqp_batch_convert_to_dual: bad arguments");
    PQP_TRY(ensure_device());
    hipStream_t s = static_cast<hipStream_t>(stream);
    const long long nm = (long long)N * M, mm = (long long)M * M, nn = (long long)N * N;
    // Gp Qp_inv (and Fp'Qp_inv) in the device's grow-only workspace, held
    // until this call's stream has synchronised
    SetupWorkspace wsp;
    float* ws = nullptr;
    PQP_TRY(wsp.acquire((size_t)B * nm + (size_t)B * M + 64, &ws));
    float* GQ = ws;
    float* fq = ws + (((size_t)B * nm + 63) & ~(size_t)63);
    // same sequence as dev_convert_to_dual (PQP_CPU.c:489-498), problem-strided
    PQP_HIP(launch_matmul_seq_b(B, GQ, d_Gp, 0, d_Qp_inv, 0, N, M, M, nm, mm, nm, s));
    PQP_HIP(launch_matmul_seq_b(B, d_Qd, GQ, 0, d_Gp, 1, N, M, N, nm, nm, nn, s));
    PQP_HIP(launch_matmul_seq_b(B, d_Fd, GQ, 0, d_Fp, 0, N, M, 1, nm, M, N, s));
    PQP_HIP(launch_axpy_b(B, d_Fd, d_Kp, 1.0f, N, N, N, s));
    PQP_HIP(launch_matmul_seq_b(B, fq, d_Fp, 1, d_Qp_inv, 0, 1, M, M, M, mm, M, s));
    PQP_HIP(launch_matmul_seq_b(B, d_Md, fq, 0, d_Fp, 0, 1, M, 1, M, M, 1, s));
    PQP_HIP(launch_axpy_b(B, d_Md, d_Mp, -1.0f, 1, 1, 1, s));
    PQP_HIP(hipStreamSynchronize(s));
    return PQP_OK;
}

int pqp_batch_relin_prepare(int B, int N, int M, const float* d_Gp, const float* d_Qp_inv, float* d_GQ, void* stream) {
    if (B <= 0 || N <= 0 || M <= 0 || !d_Gp || !d_Qp_inv || !d_GQ || (long long)B * N > 0x7fffffffLL)
        return set_error(PQP_ERR_ARG, "pqp_batch_relin_prepare: bad arguments");
    if (reinterpret_cast<uintptr_t>(d_GQ) & 15)
        return set_error(PQP_ERR_ARG, "pqp_batch_relin_prepare: d_GQ must be 16-byte aligned");
    PQP_TRY(ensure_device());
    hipStream_t s = static_cast<hipStream_t>(stream);
    const long long nm = (long long)N * M, mm = (long long)M * M;
    // the row-major product in the device's setup workspace (held until the
    // stream has synchronised), then its packets into d_GQ
    SetupWorkspace wsp;
    float* ws = nullptr;
    PQP_TRY(wsp.acquire((size_t)B * nm, &ws));
    PQP_HIP(launch_matmul_seq_b(B, ws, d_Gp, 0, d_Qp_inv, 0, N, M, M, nm, mm, nm, s));  // Gp_Qp_inv :492
    PQP_HIP(launch_relin_pack(B, N, M, ws, d_GQ, s));
    PQP_HIP(hipStreamSynchronize(s));
    return PQP_OK;
}

int pqp_batch_relinearize(int B, int N, int M, const float* d_GQ, const float* d_Qp_inv, const float* d_Kp,
                          const float* d_Fp, const float* d_Mp, float* d_Fd, float* d_Md, void* stream) {
    if (B <= 0 || N <= 0 || M <= 0 || !d_GQ || !d_Qp_inv || !d_Kp || !d_Fp || !d_Mp || !d_Fd || !d_Md ||
        (long long)B * N > 0x7fffffffLL)
        return set_error(PQP_ERR_ARG, "pqp_batch_relinearize: bad arguments");
    if (reinterpret_cast<uintptr_t>(d_GQ) & 15)
        return set_error(PQP_ERR_ARG, "pqp_batch_relinearize: d_GQ must be 16-byte aligned");
    PQP_TRY(ensure_device());
    PQP_HIP(launch_relinearize(B, N, M, d_GQ, d_Qp_inv, d_Kp, d_Fp, d_Mp, d_Fd, d_Md,
                               static_cast<hipStream_t>(stream)));
    return PQP_OK;
}

int pqp_batch_compute_fp(int B, int m, int nd, int ns, const float* d_Fp1, const float* d_Fp2, const float* d_Fp3,
                         const float* d_D, const float* d_x, float* d_Fp, void* stream) {
    if (B <= 0 || m <= 0 || nd <= 0 || ns <= 0 || !d_Fp1 || !d_Fp2 || !d_Fp3 || !d_D || !d_x || !d_Fp)
        return set_error(PQP_ERR_ARG, "pqp_batch_compute_fp: bad arguments");
    PQP_TRY(ensure_device());
    hipStream_t s = static_cast<hipStream_t>(stream);
    DevBuf t;
    PQP_TRY(t.floats((size_t)B * m));
    PQP_HIP(launch_matmul_seq_b(B, d_Fp, d_Fp1, 0, d_D, 0, m, nd, 1, 0, nd, m, s));      // Fp1 D
    PQP_HIP(launch_matmul_seq_b(B, t.f(), d_Fp2, 0, d_x, 0, m, ns, 1, 0, ns, m, s));     // Fp2 x
    PQP_HIP(launch_axpy_b(B, d_Fp, t.f(), 1.0f, m, m, m, s));
    PQP_HIP(launch_axpy_b(B, d_Fp, d_Fp3, -1.0f, m, m, 0, s));
    PQP_HIP(hipStreamSynchronize(s));
    return PQP_OK;
}

int pqp_batch_compute_mp(int B, int nd, int ns, const float* d_Mp1, const float* d_Mp2, const float* d_Mp3,
                         const float* d_Mp4, const float* d_Mp5, const float* d_Mp6, const float* d_D,
                         const float* d_x, float* d_Mp, void* stream) {
    if (B <= 0 || nd <= 0 || ns <= 0 || !d_Mp1 || !d_Mp2 || !d_Mp3 || !d_Mp4 || !d_Mp5 || !d_Mp6 || !d_D || !d_x ||
        !d_Mp)
        return set_error(PQP_ERR_ARG, "pqp_batch_compute_mp: bad arguments");
    PQP_TRY(ensure_device());
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int big = ns > nd ? ns : nd;
    DevBuf row, T;
    PQP_TRY(row.floats((size_t)B * big));
    PQP_TRY(T.floats((size_t)B * 5));
    float* R = row.f();
    float* t = T.f();
    // the five halved terms of PQP_CPU.c:400-423, term s of problem b at t[b*5 + s]
    PQP_HIP(launch_matmul_seq_b(B, R, d_x, 1, d_Mp1, 0, 1, ns, ns, ns, 0, big, s));       // x' Mp1
    PQP_HIP(launch_matmul_seq_b(B, t + 0, R, 0, d_x, 0, 1, ns, 1, big, ns, 5, s));        //  . x
    PQP_HIP(launch_matmul_seq_b(B, R, d_D, 1, d_Mp2, 0, 1, nd, ns, nd, 0, big, s));       // D' Mp2
    PQP_HIP(launch_matmul_seq_b(B, t + 1, R, 0, d_x, 0, 1, ns, 1, big, ns, 5, s));        //  . x
    PQP_HIP(launch_matmul_seq_b(B, t + 2, d_Mp4, 1, d_x, 0, 1, ns, 1, 0, ns, 5, s));      // Mp4' x
    PQP_HIP(launch_matmul_seq_b(B, R, d_D, 1, d_Mp3, 0, 1, nd, nd, nd, 0, big, s));       // D' Mp3
    PQP_HIP(launch_matmul_seq_b(B, t + 3, R, 0, d_D, 0, 1, nd, 1, big, nd, 5, s));        //  . D
    PQP_HIP(launch_matmul_seq_b(B, t + 4, d_Mp5, 1, d_D, 0, 1, nd, 1, 0, nd, 5, s));      // Mp5' D
    PQP_HIP(launch_mp_finish_b(B, t, d_Mp6, d_Mp, 0, s));
    PQP_HIP(hipStreamSynchronize(s));
    return PQP_OK;
}

// Which batched solver a problem size takes: 0 one wave / tiny workgroup
// (N, M <= 32), 3 every matrix once in LDS (k_solve_mid), 1 everything
// staged in LDS with the split copies (k_solve_small; mid_off), 2 one
// workgroup from global memory (k_solve_single; needs the prepared data of
// pqp_batch_prepare), -1 too large for any.
static int batch_path(int N, int M) {
    if (N <= 32 && M <= 32 && !g_tune.force_small) return 0;
    if (!g_tune.mid_off && solve_mid_lds_bytes(N, M, true) <= kLdsBudget) return 3;
    if (solve_small_lds_bytes(N, M) <= kLdsBudget) return 1;
    if (solve_single_lds_bytes(round4(N), round4(M), false) <= kLdsBudget) return 2;
    return -1;
}

int pqp_batch_solve_path(int N, int M) {
    if (N <= 0 || M <= 0) return set_error(PQP_ERR_ARG, "pqp_batch_solve_path: N and M must be positive");
    const int p = batch_path(N, M);
    return p < 0 ? set_error(PQP_ERR_ARG, "N=%d, M=%d exceeds the batched solvers' LDS budget", N, M) : p;
}

int pqp_batch_solve_kernel(int N, int M) {
    if (N <= 0 || M <= 0) return set_error(PQP_ERR_ARG, "pqp_batch_solve_kernel: N and M must be positive");
    return batch_path(N, M) == 2 && pipe_route(N, M, g_tune.pipe_variant) ? 1 : 0;
}

int pqp_batch_prepare(int B, int N, int M, const float* d_Qd, const float* d_Gp, const float* d_Qp_inv, float* d_QdT,
                      float* d_theta, int* d_sym, float* d_GpT, float* d_QinvT, int* all_sym_out, void* stream) {
    if (all_sym_out) *all_sym_out = 0;
    if (B <= 0 || N <= 0 || M <= 0 || !d_Qd || !d_theta || !d_sym)
        return set_error(PQP_ERR_ARG, "pqp_batch_prepare: bad arguments");
    if ((d_GpT && !d_Gp) || (d_QinvT && !d_Qp_inv))
        return set_error(PQP_ERR_ARG, "pqp_batch_prepare: a transposed copy needs its source");
    PQP_TRY(ensure_device());
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int ldq = round4(N);
    // Qd bit-symmetric in every problem (convertToDual's (Gp Qp_inv) Gp' is,
    // for a diagonal Qp_inv) and N % 4 == 0: the row-major Qd is its own
    // column-major copy, no packing pass.  The per-problem flags also gate the
    // fused Y'Qd pass of converge mode.
    PQP_HIP(launch_check_symmetric(B, d_Qd, N, d_sym, s));
    std::vector<int> hs((size_t)B);
    PQP_HIP(hipMemcpyAsync(hs.data(), d_sym, sizeof(int) * (size_t)B, hipMemcpyDeviceToHost, s));
    PQP_HIP(hipStreamSynchronize(s));
    bool all_sym = ldq == N;
    for (int v : hs) all_sym = all_sym && v != 0;
    if (all_sym_out) *all_sym_out = all_sym ? 1 : 0;
    const float* qdt = d_Qd;
    if (!all_sym) {
        if (!d_QdT)
            return set_error(PQP_ERR_NEEDS_QDT, "pqp_batch_prepare: some Qd is not bit-symmetric (or N %% 4 != 0): pass "
                                          "d_QdT ([B][N][round4(N)] floats) for its column-major copy");
        PQP_HIP(launch_pack_colmajor(B, d_Qd, N, (long long)N * N, d_QdT, ldq, (long long)N * ldq, s));
        qdt = d_QdT;
    }
    PQP_HIP(launch_theta(B, qdt, ldq, (long long)N * ldq, N, d_theta, N, s));  // computeTheta :503-519
    if (d_GpT) PQP_HIP(launch_transpose_b(B, d_Gp, N, M, d_GpT, s));
    if (d_QinvT) PQP_HIP(launch_transpose_b(B, d_Qp_inv, M, M, d_QinvT, s));
    return PQP_OK;
}

int pqp_batch_solve_prepared(int B, int N, int M, const float* d_Qd, const float* d_QdT, const float* d_theta,
                             const int* d_sym, const float* d_GpT, const float* d_QinvT, const float* d_Fd,
                             const float* d_Md, const float* d_Qp, const float* d_Qp_inv, const float* d_Fp,
                             const float* d_Mp, const float* d_Gp, const float* d_Kp, int mode, long long num_iter,
                             long long max_updates, float* d_Y, float* d_U, long long* d_h, int* d_status,
                             void* stream) {
    return pqp_batch_solve_from(B, N, M, d_Qd, d_QdT, d_theta, d_sym, d_GpT, d_QinvT, d_Fd, d_Md, d_Qp, d_Qp_inv, d_Fp,
                                d_Mp, d_Gp, d_Kp, mode, num_iter, max_updates, d_Y, d_U, d_h, d_status, nullptr,
                                stream);
}

int pqp_batch_solve_from(int B, int N, int M, const float* d_Qd, const float* d_QdT, const float* d_theta,
                         const int* d_sym, const float* d_GpT, const float* d_QinvT, const float* d_Fd,
                         const float* d_Md, const float* d_Qp, const float* d_Qp_inv, const float* d_Fp,
                         const float* d_Mp, const float* d_Gp, const float* d_Kp, int mode, long long num_iter,
                         long long max_updates, float* d_Y, float* d_U, long long* d_h, int* d_status,
                         const float* d_Y0, void* stream) {
    if (B <= 0 || N <= 0 || M <= 0 || !d_Qd || !d_Fd || !d_Y)
        return set_error(PQP_ERR_ARG, "pqp_batch_solve: bad arguments");
    if (mode != PQP_MODE_CONVERGE && mode != PQP_MODE_FIXED)
        return set_error(PQP_ERR_ARG, "pqp_batch_solve: unknown mode %d", mode);
    if (mode == PQP_MODE_CONVERGE && (!d_Md || !d_Qp || !d_Qp_inv || !d_Fp || !d_Mp || !d_Gp || !d_Kp || !d_U))
        return set_error(PQP_ERR_ARG, "pqp_batch_solve: converge mode needs every primal/dual array and U");
    PQP_TRY(ensure_device());
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int ldq = round4(N), ldm = round4(M);
    const int path = batch_path(N, M);
    if (path < 0) return set_error(PQP_ERR_ARG, "pqp_batch_solve: N=%d, M=%d exceeds the LDS budget", N, M);
    if (path == 2 && (!d_theta || !d_sym || (!d_QdT && ldq != N)))
        return set_error(PQP_ERR_ARG, "pqp_batch_solve_prepared: N=%d, M=%d needs pqp_batch_prepare's theta, "
                                      "symmetry flags and (unless every Qd is bit-symmetric) d_QdT", N, M);
    // the fused Y'Qd pass needs one more ldq-long LDS vector: only where it fits
    const bool fuse = path == 2 && !batch_unfused() && ldq == N && solve_single_lds_bytes(ldq, ldm, true) <= kLdsBudget;
    DevBuf state, pending, Udummy;
    if (!d_U) {
        PQP_TRY(Udummy.floats((size_t)B * M));
        d_U = Udummy.f();
    }
    PQP_TRY(state.alloc(sizeof(SolveState) * (size_t)B));
    PQP_TRY(pending.alloc(sizeof(int)));
    // a warm start enters as a chunked relaunch does: h = 1 with its iterate in d_Y
    PQP_HIP((d_Y0 ? launch_state_init_warm : launch_state_init)(B, static_cast<SolveState*>(state.p), s));
    if (d_Y0 && d_Y0 != d_Y)
        PQP_HIP(hipMemcpyAsync(d_Y, d_Y0, sizeof(float) * (size_t)B * N, hipMemcpyDeviceToDevice, s));
    SolveArgs a{};
    a.QdT = path == 2 ? (d_QdT ? d_QdT : d_Qd) : nullptr;
    a.Qd = d_Qd;
    a.theta = path == 2 ? d_theta : nullptr;
    a.Fd = d_Fd;
    a.Md = d_Md;
    a.Qp = d_Qp;
    a.Qinv = d_Qp_inv;
    a.sym = fuse ? d_sym : nullptr;
    a.GpT = path == 2 && mode == PQP_MODE_CONVERGE ? d_GpT : nullptr;
    a.QinvT = path == 2 && mode == PQP_MODE_CONVERGE ? d_QinvT : nullptr;
    a.feas_split = (g_tune.batch_opts & 16) ? 0 : 1;
    a.trace = g_tune.mid_trace;
    a.trace_n = g_tune.mid_trace_n;
    a.Fp = d_Fp;
    a.Mp = d_Mp;
    a.Gp = d_Gp;
    a.Kp = d_Kp;
    a.Y = d_Y;
    a.U = d_U;
    a.N = N;
    a.M = M;
    a.ldq = ldq;
    a.ldm = ldm;
    a.mode = (mode == PQP_MODE_CONVERGE) ? kModeConverge : kModeFixed;
    a.num_iter = num_iter;
    a.max_updates = max_updates;
    a.chunk = pqp::batch_chunk_for(N, M);
    a.pending = static_cast<int*>(pending.p);
    SolveState* st = static_cast<SolveState*>(state.p);
    for (;;) {
        int left = 0;
        PQP_HIP(hipMemsetAsync(pending.p, 0, sizeof(int), s));
        PQP_HIP(launch_solve_batch(B, path, a, st, s));
        PQP_HIP(hipMemcpyAsync(&left, pending.p, sizeof(int), hipMemcpyDeviceToHost, s));
        PQP_HIP(hipStreamSynchronize(s));
        if (left == 0) break;
    }
    PQP_HIP(launch_extract_state(B, st, d_h, d_status, s));
    PQP_HIP(hipStreamSynchronize(s));
    return PQP_OK;
}

int pqp_batch_solve(int B, int N, int M, const float* d_Qd, const float* d_Fd, const float* d_Md, const float* d_Qp,
                    const float* d_Qp_inv, const float* d_Fp, const float* d_Mp, const float* d_Gp, const float* d_Kp,
                    int mode, long long num_iter, long long max_updates, float* d_Y, float* d_U, long long* d_h,
                    int* d_status, void* stream) {
    if (B <= 0 || N <= 0 || M <= 0 || !d_Qd || !d_Fd || !d_Y)
        return set_error(PQP_ERR_ARG, "pqp_batch_solve: bad arguments");
    const int path = batch_path(N, M);
    if (path < 0) return set_error(PQP_ERR_ARG, "pqp_batch_solve: N=%d, M=%d exceeds the LDS budget", N, M);
    DevBuf QdT, theta, sym, GpT, QinvT;
    if (path == 2) {  // the per-problem setup, for this call only (pqp_batch_prepare keeps it across calls)
        PQP_TRY(ensure_device());
        PQP_TRY(theta.floats((size_t)B * N));
        PQP_TRY(sym.alloc(sizeof(int) * (size_t)B));
        if ((g_tune.batch_opts & 2) && mode == PQP_MODE_CONVERGE && d_Gp && d_Qp_inv) {
            PQP_TRY(GpT.floats((size_t)B * N * M));
            PQP_TRY(QinvT.floats((size_t)B * M * M));
        }
        int all_sym = 0;
        int* ps = static_cast<int*>(sym.p);
        const int rc = pqp_batch_prepare(B, N, M, d_Qd, d_Gp, d_Qp_inv, nullptr, theta.f(), ps, GpT.f(), QinvT.f(),
                                         &all_sym, stream);
        if (rc != PQP_OK && rc != PQP_ERR_NEEDS_QDT) return rc;
        if (rc == PQP_ERR_NEEDS_QDT) {  // some Qd not bit-symmetric: the column-major copy
            PQP_TRY(QdT.floats((size_t)B * N * round4(N)));
            PQP_TRY(pqp_batch_prepare(B, N, M, d_Qd, d_Gp, d_Qp_inv, QdT.f(), theta.f(), ps, GpT.f(), QinvT.f(),
                                      &all_sym, stream));
            restore_error("");  // the first call's "pass d_QdT" text is not this call's outcome
        }
    }
    return pqp_batch_solve_prepared(B, N, M, d_Qd, QdT.f(), theta.f(), static_cast<const int*>(sym.p), GpT.f(),
                                    QinvT.f(), d_Fd, d_Md, d_Qp, d_Qp_inv, d_Fp, d_Mp, d_Gp, d_Kp, mode, num_iter,
                                    max_updates, d_Y, d_U, d_h, d_status, stream);
}

// ---------------------------------------------------------------------------
// 2f. a resident plant and a one-launch control step
// ---------------------------------------------------------------------------
int pqp_plant_supported(int N, int M, int nd, int ns) { return plant_shape_ok(N, M, nd, ns) ? 1 : 0; }

// 2g: 0 unsupported, 1 the one-wave step (2f), 2 the one-workgroup step at horizon sizes
int pqp_plant_kind(int N, int M, int nd, int ns) {
    if (plant_shape_ok(N, M, nd, ns)) return 1;
    return plant_mid_shape_ok(N, M, nd, ns) ? 2 : 0;
}

// pqp_plant_create (kind 1 only) and pqp_plant_create_horizon (kinds 1 and 2): `fn` names the caller in messages
static int plant_create(const char* fn, bool horizon, int device, int N, int M, int nd, int ns, const float* Qp_inv,
                        const float* Gp, const float* Kp, const float* Fp1, const float* Fp2, const float* Fp3,
                        const float* Mp1, const float* Mp2, const float* Mp3, const float* Mp4, const float* Mp5,
                        const float* Mp6, pqp_plant** out) {
    if (!out) return set_error(PQP_ERR_ARG, "%s: null handle pointer", fn);
    *out = nullptr;
    const int kind = pqp_plant_kind(N, M, nd, ns);
    if (!horizon && kind != 1)
        return set_error(PQP_ERR_ARG, "pqp_plant_create: (N=%d, M=%d, nd=%d, ns=%d) is not a shape pqp_plant_step runs "
                                      "(N <= 32, M <= 32, N + M < 64, nd <= 64, ns <= 64): use ProblemBatch "
                                      "(pqp_batch_*) for it", N, M, nd, ns);
    if (kind == 0)
        return set_error(PQP_ERR_ARG, "%s: (N=%d, M=%d, nd=%d, ns=%d) is not a shape pqp_plant_step runs (one wave: "
                                      "N <= 32, M <= 32, N + M < 64; one workgroup: M < 64, N <= 192 and the plant "
                                      "within %zu bytes of LDS, which (N, M) takes %zu of; nd <= 64, ns <= 64): use "
                                      "ProblemBatch (pqp_batch_*) for it", fn, N, M, nd, ns, kLdsBudget,
                         (N > 0 && M > 0 && N < (1 << 14) && M < (1 << 14)) ? plant_mid_lds_bytes(N, M) : (size_t)0);
    if (!Qp_inv || !Gp || !Kp || !Fp1 || !Fp2 || !Fp3 || !Mp1 || !Mp2 || !Mp3 || !Mp4 || !Mp5 || !Mp6)
        return set_error(PQP_ERR_ARG, "%s: null input", fn);
    PQP_TRY(resolve_device(fn, device, &device));
    DeviceGuard on(device);
    PQP_TRY(ensure_device());
    hipStream_t s = lib_stream();
    std::unique_ptr<pqp_plant> P(new pqp_plant());
    P->N = N, P->M = M, P->nd = nd, P->ns = ns;
    P->kind = kind;
    P->dev = device;
    PQP_TRY(upload(P->Fp1, Fp1, (size_t)M * nd, s));
    PQP_TRY(upload(P->Fp2, Fp2, (size_t)M * ns, s));
    PQP_TRY(upload(P->Fp3, Fp3, M, s));
    PQP_TRY(upload(P->Mp1, Mp1, (size_t)ns * ns, s));
    PQP_TRY(upload(P->Mp2, Mp2, (size_t)nd * ns, s));
    PQP_TRY(upload(P->Mp3, Mp3, (size_t)nd * nd, s));
    PQP_TRY(upload(P->Mp4, Mp4, ns, s));
    PQP_TRY(upload(P->Mp5, Mp5, nd, s));
    PQP_TRY(upload(P->Mp6, Mp6, 1, s));
    // kind 2: with what k_solve_mid2 finds in Qd when it stages a problem, once -- its bit symmetry
    PlantCore& c = P->core;
    PQP_TRY(derive_plant_core(c, N, M, Qp_inv, Gp, Kp, kind == 2, s));  // (the host arrays are free after it)
    for (int pipe = 0; pipe < 2; ++pipe) {
        P->slots[pipe] = kind == 2 ? plant_mid_resident_wgs(N, M) : plant_resident_wgs(N, M, nd, ns, pipe != 0);
        if (P->slots[pipe] <= 0) {
            const hipError_t e = hipGetLastError();
            return set_error(PQP_ERR_HIP, "%s: no occupancy for (N=%d, M=%d, nd=%d, ns=%d): %s", fn, N, M, nd, ns,
                             hipGetErrorString(e));
        }
    }
    if (kind == 1 && plant_roll_shape_ok(N, M, nd, ns)) {  // 2j: the fused rollout's grid bound
        P->roll_slots = plant_roll_resident_wgs(N, M, nd, ns);
        if (P->roll_slots <= 0) {  // a plant that steps is made as before: its rollout is then the chain
            (void)hipGetLastError();
            P->roll_slots = 0;
        }
    }
    if (kind == 2) {  // 2l: the fused rollout's grid bound; a plant that steps is made as before
        P->roll_mid_slots = plant_mid_roll_resident_wgs(N, M);
        if (P->roll_mid_slots <= 0) {
            (void)hipGetLastError();
            P->roll_mid_slots = 0;
        }
    }
    if (kind == 2) {  // the rest of what k_solve_mid2 finds in Qd: NaN / inf, by a scan of the host copy
        std::vector<float> hq((size_t)N * N);
        PQP_TRY(download(hq.data(), c.Qd.p, hq.size(), s));
        PQP_HIP(hipStreamSynchronize(s));
        bool nan = false, inf = false;
        for (float q : hq) {
            nan = nan || q != q;
            inf = inf || std::fabs(q) == std::numeric_limits<float>::infinity();
        }
        P->mid.sym = c.sym;
        P->mid.fast = nan ? 0 : 1;
        P->mid.qfinite = (!nan && !inf) ? 1 : 0;
    }
    PlantData& d = P->data;
    d.N = N, d.M = M, d.nd = nd, d.ns = ns;
    d.Qd = c.Qd.f(), d.Gp = c.Gp.f(), d.Qp = c.Qp.f(), d.Qinv = c.Qinv.f(), d.Kp = c.Kp.f();
    d.theta = c.theta.f(), d.GQ = c.GQ.f();
    d.Fp1 = P->Fp1.f(), d.Fp2 = P->Fp2.f(), d.Fp3 = P->Fp3.f();
    d.Mp1 = P->Mp1.f(), d.Mp2 = P->Mp2.f(), d.Mp3 = P->Mp3.f();
    d.Mp4 = P->Mp4.f(), d.Mp5 = P->Mp5.f(), d.Mp6 = P->Mp6.f();
    *out = P.release();
    return PQP_OK;
}

int pqp_plant_create(int device, int N, int M, int nd, int ns, const float* Qp_inv, const float* Gp, const float* Kp,
                     const float* Fp1, const float* Fp2, const float* Fp3, const float* Mp1, const float* Mp2,
                     const float* Mp3, const float* Mp4, const float* Mp5, const float* Mp6, pqp_plant** out) {
    return plant_create("pqp_plant_create", false, device, N, M, nd, ns, Qp_inv, Gp, Kp, Fp1, Fp2, Fp3, Mp1, Mp2, Mp3,
                        Mp4, Mp5, Mp6, out);
}

int pqp_plant_create_horizon(int device, int N, int M, int nd, int ns, const float* Qp_inv, const float* Gp,
                             const float* Kp, const float* Fp1, const float* Fp2, const float* Fp3, const float* Mp1,
                             const float* Mp2, const float* Mp3, const float* Mp4, const float* Mp5, const float* Mp6,
                             pqp_plant** out) {
    return plant_create("pqp_plant_create_horizon", true, device, N, M, nd, ns, Qp_inv, Gp, Kp, Fp1, Fp2, Fp3, Mp1, Mp2,
                        Mp3, Mp4, Mp5, Mp6, out);
}

int pqp_plant_destroy(pqp_plant* p) {
    if (!p) return PQP_OK;
    DeviceGuard on(p->dev);
    delete p;
    return PQP_OK;
}

int pqp_plant_get(pqp_plant* p, float* Qd, float* Qp, float* theta) {
    if (!p) return set_error(PQP_ERR_ARG, "pqp_plant_get: null plant");
    DeviceGuard on(p->dev);
    PQP_TRY(ensure_device());
    hipStream_t s = lib_stream();
    PQP_TRY(download_plant_core(p->core, p->N, p->M, Qd, Qp, theta, s));
    PQP_HIP(hipStreamSynchronize(s));
    return PQP_OK;
}

long long pqp_plant_max_updates(const pqp_plant* p) {
    if (!p) return set_error(PQP_ERR_ARG, "pqp_plant_max_updates: null plant");
    return pqp::batch_chunk_for(p->N, p->M);
}

// A kind-2 plant's flags as a launch takes them: create's, and the tuning knob mid2_dense as it is now.
static PlantMidFlags plant_mid_flags(const pqp_plant& p) {
    PlantMidFlags F = p.mid;
    F.dense = g_tune.mid2_dense ? 1 : 0;
    return F;
}

// One step's launch on the plant's device (current): the kind's kernel, at the tuning knobs' form.
static int plant_launch_step(const pqp_plant& p, const PlantStep& S, hipStream_t s) {
    if (p.kind == 2) {  // the one-workgroup step: plant_pipe has no meaning for it
        PQP_HIP(launch_plant_step_mid(p.data, S, plant_mid_flags(p), p.slots[0], s));
        return PQP_OK;
    }
    const bool pipe = g_plant_pipe != 0;
    PQP_HIP(launch_plant_step(p.data, S, p.slots[pipe ? 1 : 0], pipe, s));
    return PQP_OK;
}

// 2k: a tolerance is a finite float >= 0 (-0.0f counts as 0); checked before anything else of a _tol call
static int check_tols(const char* fn, float abs_tol, float rel_tol) {
    if (!(abs_tol >= 0.0f) || std::isinf(abs_tol))
        return set_error(PQP_ERR_ARG, "%s: abs_tol = %g is not a finite value >= 0", fn, (double)abs_tol);
    if (!(rel_tol >= 0.0f) || std::isinf(rel_tol))
        return set_error(PQP_ERR_ARG, "%s: rel_tol = %g is not a finite value >= 0", fn, (double)rel_tol);
    return PQP_OK;
}

// What the step, solve and rollout entry points check alike, in two parts, since each has checks of its own between
// them: the handle (`what` names it) and B; then max_updates against one launch's budget (`budget_fn` reports it,
// `per` is what it bounds: a launch or a rollout's step).
static int check_states(const char* fn, const void* handle, const char* what, int B) {
    if (!handle) return set_error(PQP_ERR_ARG, "%s: null %s", fn, what);
    if (B <= 0) return set_error(PQP_ERR_ARG, "%s: B = %d states", fn, B);
    return PQP_OK;
}
static int check_budget(const char* fn, long long max_updates, int N, int M, const char* budget_fn, const char* per) {
    const long long cap = pqp::batch_chunk_for(N, M);
    if (max_updates < 1 || max_updates > cap)
        return set_error(PQP_ERR_ARG, "%s: max_updates = %lld is outside 1 .. %lld (%s: one %s's budget)", fn,
                         max_updates, cap, budget_fn, per);
    return PQP_OK;
}

// pqp_plant_step (fn names the caller in messages; tolerances 0, 0) and pqp_plant_step_tol
static int plant_step(const char* fn, pqp_plant* p, int B, const float* d_x, const float* d_D, const float* d_Kp,
                      int warm, long long max_updates, float* d_Y, float* d_U, long long* d_h, int* d_status,
                      float* d_Fp, float* d_Mp, float* d_Fd, float* d_Md, float* d_Jp, float* d_Jd, float abs_tol,
                      float rel_tol, void* stream) {
    PQP_TRY(check_tols(fn, abs_tol, rel_tol));
    PQP_TRY(check_states(fn, p, "plant", B));
    if (!d_x || !d_D || !d_Y || !d_U) return set_error(PQP_ERR_ARG, "%s: null d_x, d_D, d_Y or d_U", fn);
    PQP_TRY(check_budget(fn, max_updates, p->N, p->M, "pqp_plant_max_updates", "launch"));
    PlantStep S{};
    S.B = B;
    S.warm = warm ? 1 : 0;
    S.max_updates = max_updates;
    S.x = d_x, S.D = d_D, S.Kp = d_Kp;
    S.Y = d_Y, S.U = d_U, S.h = d_h, S.status = d_status;
    S.Fp = d_Fp, S.Mp = d_Mp, S.Fd = d_Fd, S.Md = d_Md, S.Jp = d_Jp, S.Jd = d_Jd;
    S.abs_tol = abs_tol, S.rel_tol = rel_tol;
    DeviceGuard on(p->dev);
    return plant_launch_step(*p, S, static_cast<hipStream_t>(stream));
}

int pqp_plant_step(pqp_plant* p, int B, const float* d_x, const float* d_D, const float* d_Kp, int warm,
                   long long max_updates, float* d_Y, float* d_U, long long* d_h, int* d_status, float* d_Fp,
                   float* d_Mp, float* d_Fd, float* d_Md, float* d_Jp, float* d_Jd, void* stream) {
    return plant_step("pqp_plant_step", p, B, d_x, d_D, d_Kp, warm, max_updates, d_Y, d_U, d_h, d_status, d_Fp, d_Mp,
                      d_Fd, d_Md, d_Jp, d_Jd, 0.0f, 0.0f, stream);
}

int pqp_plant_step_tol(pqp_plant* p, int B, const float* d_x, const float* d_D, const float* d_Kp, int warm,
                       long long max_updates, float* d_Y, float* d_U, long long* d_h, int* d_status, float* d_Fp,
                       float* d_Mp, float* d_Fd, float* d_Md, float* d_Jp, float* d_Jd, float abs_tol, float rel_tol,
                       void* stream) {
    return plant_step("pqp_plant_step_tol", p, B, d_x, d_D, d_Kp, warm, max_updates, d_Y, d_U, d_h, d_status, d_Fp,
                      d_Mp, d_Fd, d_Md, d_Jp, d_Jd, abs_tol, rel_tol, stream);
}

// ---------------------------------------------------------------------------
// 2j. the closed loop: the plant's dynamics, and K control steps in one call
// ---------------------------------------------------------------------------
int pqp_dynamics_create(int device, int ns, int M, int nd, const float* A, const float* Bu, const float* Bd,
                        pqp_dynamics** out) {
    if (!out) return set_error(PQP_ERR_ARG, "pqp_dynamics_create: null handle pointer");
    *out = nullptr;
    if (ns < 1 || ns > 64 || nd < 1 || nd > 64 || M < 1 || M > kDynMaxM)
        return set_error(PQP_ERR_ARG, "pqp_dynamics_create: (ns=%d, M=%d, nd=%d) is outside 1 <= ns, nd <= 64, "
                                      "1 <= M <= %d", ns, M, nd, kDynMaxM);
    if (!A || !Bu || !Bd) return set_error(PQP_ERR_ARG, "pqp_dynamics_create: null input");
    PQP_TRY(resolve_device("pqp_dynamics_create", device, &device));
    DeviceGuard on(device);
    PQP_TRY(ensure_device());
    hipStream_t s = lib_stream();
    std::unique_ptr<pqp_dynamics> D(new pqp_dynamics());
    D->ns = ns, D->M = M, D->nd = nd;
    D->dev = device;
    // k-major copies: word [k][i] is the reference's [i][k]
    auto transposed = [ns](const float* a, int cols) {
        std::vector<float> t((size_t)cols * ns);
        for (int i = 0; i < ns; ++i)
            for (int k = 0; k < cols; ++k) t[(size_t)k * ns + i] = a[(size_t)i * cols + k];
        return t;
    };
    const std::vector<float> at = transposed(A, ns), but = transposed(Bu, M), bdt = transposed(Bd, nd);
    PQP_TRY(upload(D->AT, at.data(), at.size(), s));
    PQP_TRY(upload(D->BuT, but.data(), but.size(), s));
    PQP_TRY(upload(D->BdT, bdt.data(), bdt.size(), s));
    PQP_HIP(hipStreamSynchronize(s));  // the host copies are free after it
    D->data = DynData{ns, M, nd, D->AT.f(), D->BuT.f(), D->BdT.f()};
    *out = D.release();
    return PQP_OK;
}

int pqp_dynamics_destroy(pqp_dynamics* d) {
    if (!d) return PQP_OK;
    DeviceGuard on(d->dev);
    delete d;
    return PQP_OK;
}

int pqp_dynamics_advance(const pqp_dynamics* d, int B, const float* d_x, const float* d_U, const float* d_D,
                         float* d_xnext, void* stream) {
    PQP_TRY(check_states("pqp_dynamics_advance", d, "dynamics", B));
    if (!d_x || !d_U || !d_D || !d_xnext)
        return set_error(PQP_ERR_ARG, "pqp_dynamics_advance: null d_x, d_U, d_D or d_xnext");
    if (d_xnext == d_x) return set_error(PQP_ERR_ARG, "pqp_dynamics_advance: d_xnext aliases d_x");
    const size_t words = (size_t)B * d->ns;
    if (d_xnext < d_x + words && d_x < d_xnext + words)
        return set_error(PQP_ERR_ARG, "pqp_dynamics_advance: d_xnext overlaps d_x");
    DeviceGuard on(d->dev);
    PlantAdvance a{B, 0, 0.0f, d_x, d_U, d_D, d_xnext, nullptr};
    PQP_HIP(launch_plant_advance(d->data, a, static_cast<hipStream_t>(stream)));
    return PQP_OK;
}

int pqp_plant_rollout_fused(int N, int M, int nd, int ns) { return plant_roll_shape_ok(N, M, nd, ns) ? 1 : 0; }

int pqp_plant_rollout_forms(int N, int M, int nd, int ns) {
    const int chain = 1 << PQP_ROLL_CHAIN, fused = 1 << PQP_ROLL_FUSED;
    if (plant_shape_ok(N, M, nd, ns)) return chain | (plant_roll_shape_ok(N, M, nd, ns) ? fused : 0);
    if (plant_mid_shape_ok(N, M, nd, ns)) return chain | fused;  // k_plant_roll_mid takes the step's LDS
    return 0;
}

// pqp_plant_rollout (tolerances 0, 0), pqp_plant_rollout_tol (both PQP_ROLL_DEFAULT) and pqp_plant_rollout_form
static int plant_rollout(const char* fn, pqp_plant* p, const pqp_dynamics* dyn, int B, int K, float* d_X,
                         const float* d_D, int D_steps, const float* d_Kp, int warm, float y_floor,
                         long long max_updates, float* d_Y, float* d_U, long long* d_h, int* d_status, float* d_Jp,
                         float* d_Jd, float abs_tol, float rel_tol, int form, void* stream) {
    PQP_TRY(check_tols(fn, abs_tol, rel_tol));
    if (form < PQP_ROLL_DEFAULT || form > PQP_ROLL_FUSED)
        return set_error(PQP_ERR_ARG, "%s: form = %d is none of PQP_ROLL_DEFAULT, PQP_ROLL_CHAIN, PQP_ROLL_FUSED", fn,
                         form);
    if (!p) return set_error(PQP_ERR_ARG, "%s: null plant", fn);
    PQP_TRY(check_states(fn, dyn, "dynamics", B));
    if (K <= 0) return set_error(PQP_ERR_ARG, "%s: K = %d steps", fn, K);
    if (D_steps != 1 && D_steps != K)
        return set_error(PQP_ERR_ARG, "%s: D_steps = %d is neither 1 nor K = %d", fn, D_steps, K);
    if (!d_X || !d_D || !d_Y || !d_U) return set_error(PQP_ERR_ARG, "%s: null d_X, d_D, d_Y or d_U", fn);
    PQP_TRY(check_budget(fn, max_updates, p->N, p->M, "pqp_plant_max_updates", "step"));
    if (dyn->ns != p->ns || dyn->M != p->M || dyn->nd != p->nd)
        return set_error(PQP_ERR_ARG, "%s: the dynamics' (ns=%d, M=%d, nd=%d) are not the plant's "
                                      "(ns=%d, M=%d, nd=%d)", fn, dyn->ns, dyn->M, dyn->nd, p->ns, p->M, p->nd);
    if (dyn->dev != p->dev)
        return set_error(PQP_ERR_ARG, "%s: the dynamics are on device %d, the plant on device %d", fn, dyn->dev,
                         p->dev);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t B_ = (size_t)B;
    PlantStep S{};
    S.B = B;
    S.max_updates = max_updates;
    S.Kp = d_Kp;
    S.Y = d_Y;
    S.abs_tol = abs_tol, S.rel_tol = rel_tol;
    const int fused_slots = p->kind == 1 ? p->roll_slots : p->roll_mid_slots;
    if (form == PQP_ROLL_FUSED && fused_slots <= 0)
        return set_error(PQP_ERR_ARG, "%s: PQP_ROLL_FUSED, but the fused launch of this plant (N=%d, M=%d, nd=%d, ns=%d) "
                                      "has no occupancy on device %d: use PQP_ROLL_CHAIN", fn, p->N, p->M, p->nd, p->ns,
                         p->dev);
    // the default: one launch for kind 1 (unless plant_roll_chain says otherwise), the chain for kind 2
    const bool fused = form == PQP_ROLL_FUSED ||
                       (form == PQP_ROLL_DEFAULT && p->kind == 1 && p->roll_slots > 0 && !g_plant_roll_chain);
    DeviceGuard on(p->dev);
    if (fused) {  // ONE launch: the ROLL form of k_plant_step (kind 1) or of k_plant_step_mid (kind 2, 2l)
        S.warm = warm ? 1 : 0;
        S.D = d_D;
        S.U = d_U, S.h = d_h, S.status = d_status, S.Jp = d_Jp, S.Jd = d_Jd;
        const PlantRoll R{K, D_steps, y_floor, d_X, dyn->data};
        if (p->kind == 2) {
            PQP_HIP(launch_plant_roll_mid(p->data, S, plant_mid_flags(*p), R, p->roll_mid_slots, s));
        } else {
            PQP_HIP(launch_plant_roll(p->data, S, R, p->roll_slots, s));
        }
        return PQP_OK;
    }
    // the chain: K times the step and the advance, which also floors Y for the next step
    const bool floored = y_floor > 0.0f;
    if (warm && floored) PQP_HIP(launch_plant_floor(d_Y, B_ * p->N, y_floor, s));
    for (int k = 0; k < K; ++k) {
        const size_t kb = (size_t)k * B_;
        S.warm = (k > 0 || warm) ? 1 : 0;
        S.x = d_X + kb * p->ns;
        S.D = d_D + (D_steps > 1 ? kb * p->nd : (size_t)0);
        S.U = d_U + kb * p->M;
        S.h = d_h ? d_h + kb : nullptr;
        S.status = d_status ? d_status + kb : nullptr;
        S.Jp = d_Jp ? d_Jp + kb : nullptr;
        S.Jd = d_Jd ? d_Jd + kb : nullptr;
        PQP_TRY(plant_launch_step(*p, S, s));
        const PlantAdvance a{B, p->N, y_floor, S.x, S.U, S.D, d_X + (kb + B_) * p->ns,
                             (floored && k + 1 < K) ? d_Y : nullptr};
        PQP_HIP(launch_plant_advance(dyn->data, a, s));
    }
    return PQP_OK;
}

int pqp_plant_rollout(pqp_plant* p, const pqp_dynamics* dyn, int B, int K, float* d_X, const float* d_D, int D_steps,
                      const float* d_Kp, int warm, float y_floor, long long max_updates, float* d_Y, float* d_U,
                      long long* d_h, int* d_status, float* d_Jp, float* d_Jd, void* stream) {
    return plant_rollout("pqp_plant_rollout", p, dyn, B, K, d_X, d_D, D_steps, d_Kp, warm, y_floor, max_updates, d_Y,
                         d_U, d_h, d_status, d_Jp, d_Jd, 0.0f, 0.0f, PQP_ROLL_DEFAULT, stream);
}

int pqp_plant_rollout_tol(pqp_plant* p, const pqp_dynamics* dyn, int B, int K, float* d_X, const float* d_D,
                          int D_steps, const float* d_Kp, int warm, float y_floor, long long max_updates, float* d_Y,
                          float* d_U, long long* d_h, int* d_status, float* d_Jp, float* d_Jd, float abs_tol,
                          float rel_tol, void* stream) {
    return plant_rollout("pqp_plant_rollout_tol", p, dyn, B, K, d_X, d_D, D_steps, d_Kp, warm, y_floor, max_updates,
                         d_Y, d_U, d_h, d_status, d_Jp, d_Jd, abs_tol, rel_tol, PQP_ROLL_DEFAULT, stream);
}

int pqp_plant_rollout_form(pqp_plant* p, const pqp_dynamics* dyn, int B, int K, float* d_X, const float* d_D,
                           int D_steps, const float* d_Kp, int warm, float y_floor, long long max_updates, float* d_Y,
                           float* d_U, long long* d_h, int* d_status, float* d_Jp, float* d_Jd, float abs_tol,
                           float rel_tol, int form, void* stream) {
    return plant_rollout("pqp_plant_rollout_form", p, dyn, B, K, d_X, d_D, D_steps, d_Kp, warm, y_floor, max_updates,
                         d_Y, d_U, d_h, d_status, d_Jp, d_Jd, abs_tol, rel_tol, form, stream);
}

// ---------------------------------------------------------------------------
// 2h. the shared-plant converge solve: B states of one plant on one resident Qd
// ---------------------------------------------------------------------------
int pqp_shared_states(int N, int M) { return pqp::solve_shared_states(N, M); }

// The nine linear-term matrices of a plant (pqp_shared_create_plant), host pointers in the reference layouts.
struct SharedPlantIn {
    int nd, ns;
    const float *Fp1, *Fp2, *Fp3, *Mp1, *Mp2, *Mp3, *Mp4, *Mp5, *Mp6;
};

// pqp_shared_create (lin NULL) and pqp_shared_create_plant: `fn` names the caller in messages
static int shared_create(const char* fn, int device, int N, int M, const float* Qp_inv, const float* Gp,
                         const float* Kp, const SharedPlantIn* lin, pqp_shared** out) {
    if (!out) return set_error(PQP_ERR_ARG, "%s: null handle pointer", fn);
    *out = nullptr;
    if (N <= 0 || M <= 0) return set_error(PQP_ERR_ARG, "%s: N = %d, M = %d must be positive", fn, N, M);
    if (lin && (lin->nd <= 0 || lin->ns <= 0))
        return set_error(PQP_ERR_ARG, "%s: nd = %d, ns = %d must be positive", fn, lin->nd, lin->ns);
    const int S = pqp::solve_shared_states(N, M);
    if (S == 0)
        return set_error(PQP_ERR_ARG, "%s: (N=%d, M=%d) is not a shape pqp_shared_solve runs: two states' "
                                      "vectors, 2 * 4 * (4 * round4(N) + 3 * round4(M)) bytes, must fit %zu bytes of LDS "
                                      "(160 KiB less %zu)", fn, N, M, kSolveSharedLdsBudget - kSolveSharedStaticLds,
                         kSolveSharedStaticLds);
    if (lin && pqp::step_shared_states(N, M, lin->nd, lin->ns) == 0)
        return set_error(PQP_ERR_ARG, "%s: (N=%d, M=%d, nd=%d, ns=%d) is not a shape pqp_shared_step runs: the step's "
                                      "words of %d states, %d * 4 * (3 * round4(ns) + 2 * round4(nd) + 2 * round4(M)) "
                                      "bytes, must fit %zu bytes of LDS (160 KiB less %zu)", fn, N, M, lin->nd, lin->ns,
                         S, S, kSolveSharedLdsBudget - kSolveSharedStaticLds, kSolveSharedStaticLds);
    if (!Qp_inv || !Gp || !Kp) return set_error(PQP_ERR_ARG, "%s: null input", fn);
    if (lin && (!lin->Fp1 || !lin->Fp2 || !lin->Fp3 || !lin->Mp1 || !lin->Mp2 || !lin->Mp3 || !lin->Mp4 || !lin->Mp5 ||
                !lin->Mp6))
        return set_error(PQP_ERR_ARG, "%s: null input", fn);
    PQP_TRY(resolve_device(fn, device, &device));
    DeviceGuard on(device);
    PQP_TRY(ensure_device());
    hipStream_t s = lib_stream();
    std::unique_ptr<pqp_shared> P(new pqp_shared());
    const int ldq = round4(N), ldm = round4(M);
    P->N = N, P->M = M, P->ldq = ldq, P->ldm = ldm, P->S = S, P->dev = device;
    PlantCore& c = P->core;
    PQP_TRY(derive_plant_core(c, N, M, Qp_inv, Gp, Kp, true, s));
    // the kernels' layouts: rows padded to a multiple of 4 floats (zero-filled), k-major for each product
    PQP_TRY(P->QdR.floats((size_t)N * ldq));
    PQP_TRY(P->GpP.floats((size_t)N * ldm));
    PQP_TRY(P->GpT.floats((size_t)M * ldq));
    PQP_TRY(P->QinvT.floats((size_t)M * ldm));
    PQP_TRY(P->QinvR.floats((size_t)M * ldm));
    PQP_TRY(P->QpP.floats((size_t)M * ldm));
    PQP_TRY(P->GQT.floats((size_t)M * ldq));
    PQP_HIP(launch_shared_layout(c.Qd.f(), N, N, 0, P->QdR.f(), ldq, s));
    if (!c.sym) {  // a bit-symmetric Qd is its own column-major copy
        PQP_TRY(P->QdT.floats((size_t)N * ldq));
        PQP_HIP(launch_shared_layout(c.Qd.f(), N, N, 1, P->QdT.f(), ldq, s));
    }
    PQP_HIP(launch_shared_layout(c.Gp.f(), N, M, 0, P->GpP.f(), ldm, s));
    PQP_HIP(launch_shared_layout(c.Gp.f(), M, N, 1, P->GpT.f(), ldq, s));
    PQP_HIP(launch_shared_layout(c.Qinv.f(), M, M, 1, P->QinvT.f(), ldm, s));
    PQP_HIP(launch_shared_layout(c.Qinv.f(), M, M, 0, P->QinvR.f(), ldm, s));
    PQP_HIP(launch_shared_layout(c.Qp.f(), M, M, 0, P->QpP.f(), ldm, s));
    PQP_HIP(launch_shared_layout(c.GQ.f(), M, N, 1, P->GQT.f(), ldq, s));
    DevBuf in[5];  // the uploaded Fp1, Fp2, Mp1, Mp2, Mp3, alive until their padded copies are made
    if (lin) {
        // the step's matrices: k-major for its products, rows padded like the rest
        const int nd = lin->nd, ns = lin->ns, ldd = round4(nd), ldx = round4(ns);
        P->nd = nd, P->ns = ns;
        PQP_TRY(upload(in[0], lin->Fp1, (size_t)M * nd, s));
        PQP_TRY(upload(in[1], lin->Fp2, (size_t)M * ns, s));
        PQP_TRY(upload(in[2], lin->Mp1, (size_t)ns * ns, s));
        PQP_TRY(upload(in[3], lin->Mp2, (size_t)nd * ns, s));
        PQP_TRY(upload(in[4], lin->Mp3, (size_t)nd * nd, s));
        PQP_TRY(upload(P->Fp3, lin->Fp3, M, s));
        PQP_TRY(upload(P->Mp4, lin->Mp4, ns, s));
        PQP_TRY(upload(P->Mp5, lin->Mp5, nd, s));
        PQP_TRY(upload(P->Mp6, lin->Mp6, 1, s));
        PQP_TRY(P->Fp1T.floats((size_t)nd * ldm));
        PQP_TRY(P->Fp2T.floats((size_t)ns * ldm));
        PQP_TRY(P->Mp1P.floats((size_t)ns * ldx));
        PQP_TRY(P->Mp2P.floats((size_t)nd * ldx));
        PQP_TRY(P->Mp3P.floats((size_t)nd * ldd));
        PQP_HIP(launch_shared_layout(in[0].f(), nd, M, 1, P->Fp1T.f(), ldm, s));
        PQP_HIP(launch_shared_layout(in[1].f(), ns, M, 1, P->Fp2T.f(), ldm, s));
        PQP_HIP(launch_shared_layout(in[2].f(), ns, ns, 0, P->Mp1P.f(), ldx, s));
        PQP_HIP(launch_shared_layout(in[3].f(), nd, ns, 0, P->Mp2P.f(), ldx, s));
        PQP_HIP(launch_shared_layout(in[4].f(), nd, nd, 0, P->Mp3P.f(), ldd, s));
    }
    PQP_HIP(hipStreamSynchronize(s));  // the host arrays and the uploaded copies are free after it
    *out = P.release();
    return PQP_OK;
}

int pqp_shared_create(int device, int N, int M, const float* Qp_inv, const float* Gp, const float* Kp,
                      pqp_shared** out) {
    return shared_create("pqp_shared_create", device, N, M, Qp_inv, Gp, Kp, nullptr, out);
}

int pqp_shared_destroy(pqp_shared* p) {
    if (!p) return PQP_OK;
    DeviceGuard on(p->dev);
    delete p;
    return PQP_OK;
}

int pqp_shared_get(pqp_shared* p, float* Qd, float* Qp, float* theta, float* GQ, int* sym_out) {
    if (!p) return set_error(PQP_ERR_ARG, "pqp_shared_get: null handle");
    DeviceGuard on(p->dev);
    PQP_TRY(ensure_device());
    hipStream_t s = lib_stream();
    PQP_TRY(download_plant_core(p->core, p->N, p->M, Qd, Qp, theta, s));
    if (GQ) PQP_TRY(download(GQ, p->core.GQ.p, (size_t)p->N * p->M, s));
    PQP_HIP(hipStreamSynchronize(s));
    if (sym_out) *sym_out = p->core.sym;
    return PQP_OK;
}

// The handle's part of a solve's or a step's SharedSolveCore: the plant's layouts and the shape.
static SharedSolveCore shared_core_args(const pqp_shared& p) {
    SharedSolveCore a{};
    const int sym = p.core.sym;
    a.QdR = p.QdR.f(), a.QdT = sym ? p.QdR.f() : p.QdT.f(), a.theta = p.core.theta.f();
    a.GpP = p.GpP.f(), a.GpT = p.GpT.f(), a.QinvT = p.QinvT.f(), a.QpP = p.QpP.f(), a.Kp = p.core.Kp.f();
    a.N = p.N, a.M = p.M, a.ldq = p.ldq, a.ldm = p.ldm, a.sym = sym;
    return a;
}

int pqp_shared_relinearize(pqp_shared* p, int B, const float* d_Fp, const float* d_Mp, const float* d_Kp, float* d_Fd,
                           float* d_Md, void* stream) {
    PQP_TRY(check_states("pqp_shared_relinearize", p, "handle", B));
    if (!d_Fp || !d_Mp || !d_Fd || !d_Md)
        return set_error(PQP_ERR_ARG, "pqp_shared_relinearize: null d_Fp, d_Mp, d_Fd or d_Md");
    SharedRelinArgs a{};
    a.GQT = p->GQT.f(), a.QinvR = p->QinvR.f(), a.Kp = p->core.Kp.f();
    a.Fp = d_Fp, a.Mp = d_Mp, a.KpB = d_Kp, a.Fd = d_Fd, a.Md = d_Md;
    a.N = p->N, a.M = p->M, a.ldq = p->ldq, a.ldm = p->ldm, a.B = B;
    DeviceGuard on(p->dev);
    PQP_HIP(launch_relin_shared(a, p->S, static_cast<hipStream_t>(stream)));
    return PQP_OK;
}

// pqp_shared_solve (tolerances 0, 0) and pqp_shared_solve_tol
static int shared_solve(const char* fn, pqp_shared* p, int B, const float* d_Fd, const float* d_Md, const float* d_Fp,
                        const float* d_Mp, const float* d_Kp, long long max_updates, const float* d_Y0, float* d_Y,
                        float* d_U, long long* d_h, int* d_status, float* d_Jp, float* d_Jd, float abs_tol,
                        float rel_tol, void* stream) {
    PQP_TRY(check_tols(fn, abs_tol, rel_tol));
    PQP_TRY(check_states(fn, p, "handle", B));
    if (!d_Fd || !d_Md || !d_Fp || !d_Mp || !d_Y || !d_U)
        return set_error(PQP_ERR_ARG, "%s: null d_Fd, d_Md, d_Fp, d_Mp, d_Y or d_U", fn);
    DeviceGuard on(p->dev);
    PQP_TRY(ensure_device());
    hipStream_t s = static_cast<hipStream_t>(stream);
    // per-call resume storage, as pqp_batch_solve: solves on different streams share nothing but the handle
    DevBuf state, pending;
    PQP_TRY(state.alloc(sizeof(SharedSolveState) * (size_t)B));
    PQP_TRY(pending.alloc(sizeof(int)));
    SharedSolveArgs a{shared_core_args(*p)};  // (built in place; the tolerances after it zeroed)
    a.Fd = d_Fd, a.Md = d_Md, a.Fp = d_Fp, a.Mp = d_Mp, a.KpB = d_Kp;
    a.Y = d_Y, a.U = d_U, a.h = d_h, a.status = d_status, a.Jp = d_Jp, a.Jd = d_Jd;
    a.st = static_cast<SharedSolveState*>(state.p);
    a.pending = static_cast<int*>(pending.p);
    a.B = B;
    a.max_updates = max_updates;
    a.abs_tol = abs_tol, a.rel_tol = rel_tol;
    a.chunk = pqp::batch_chunk_for(p->N, p->M);
    PQP_HIP(launch_shared_solve_init(B, p->N, a.st, d_Y0, d_Y, s));
    for (;;) {  // bounded launches that resume from the device state
        int left = 0;
        PQP_HIP(hipMemsetAsync(pending.p, 0, sizeof(int), s));
        PQP_HIP(launch_solve_shared(a, p->S, s));
        PQP_HIP(hipMemcpyAsync(&left, pending.p, sizeof(int), hipMemcpyDeviceToHost, s));
        PQP_HIP(hipStreamSynchronize(s));
        if (left == 0) break;
    }
    return PQP_OK;
}

int pqp_shared_solve(pqp_shared* p, int B, const float* d_Fd, const float* d_Md, const float* d_Fp, const float* d_Mp,
                     const float* d_Kp, long long max_updates, const float* d_Y0, float* d_Y, float* d_U,
                     long long* d_h, int* d_status, float* d_Jp, float* d_Jd, void* stream) {
    return shared_solve("pqp_shared_solve", p, B, d_Fd, d_Md, d_Fp, d_Mp, d_Kp, max_updates, d_Y0, d_Y, d_U, d_h,
                        d_status, d_Jp, d_Jd, 0.0f, 0.0f, stream);
}

int pqp_shared_solve_tol(pqp_shared* p, int B, const float* d_Fd, const float* d_Md, const float* d_Fp,
                         const float* d_Mp, const float* d_Kp, long long max_updates, const float* d_Y0, float* d_Y,
                         float* d_U, long long* d_h, int* d_status, float* d_Jp, float* d_Jd, float abs_tol,
                         float rel_tol, void* stream) {
    return shared_solve("pqp_shared_solve_tol", p, B, d_Fd, d_Md, d_Fp, d_Mp, d_Kp, max_updates, d_Y0, d_Y, d_U, d_h,
                        d_status, d_Jp, d_Jd, abs_tol, rel_tol, stream);
}

// ---------------------------------------------------------------------------
// 2i. the shared plant's control step: x, D to U for B states in one launch
// ---------------------------------------------------------------------------
int pqp_shared_step_states(int N, int M, int nd, int ns) { return pqp::step_shared_states(N, M, nd, ns); }

int pqp_shared_create_plant(int device, int N, int M, int nd, int ns, const float* Qp_inv, const float* Gp,
                            const float* Kp, const float* Fp1, const float* Fp2, const float* Fp3, const float* Mp1,
                            const float* Mp2, const float* Mp3, const float* Mp4, const float* Mp5, const float* Mp6,
                            pqp_shared** out) {
    const SharedPlantIn lin = {nd, ns, Fp1, Fp2, Fp3, Mp1, Mp2, Mp3, Mp4, Mp5, Mp6};
    return shared_create("pqp_shared_create_plant", device, N, M, Qp_inv, Gp, Kp, &lin, out);
}

long long pqp_shared_max_updates(const pqp_shared* p) {
    if (!p) return set_error(PQP_ERR_ARG, "pqp_shared_max_updates: null handle");
    return pqp::batch_chunk_for(p->N, p->M);
}

// pqp_shared_step (tolerances 0, 0) and pqp_shared_step_tol
static int shared_step(const char* fn, pqp_shared* p, int B, const float* d_x, const float* d_D, const float* d_Kp,
                       int warm, long long max_updates, float* d_Y, float* d_U, long long* d_h, int* d_status,
                       float* d_Fp, float* d_Mp, float* d_Fd, float* d_Md, float* d_Jp, float* d_Jd, float abs_tol,
                       float rel_tol, void* stream) {
    PQP_TRY(check_tols(fn, abs_tol, rel_tol));
    PQP_TRY(check_states(fn, p, "handle", B));
    if (!d_x || !d_D || !d_Y || !d_U || !d_Fp || !d_Fd)
        return set_error(PQP_ERR_ARG, "%s: null d_x, d_D, d_Y, d_U, d_Fp or d_Fd", fn);
    if (p->nd == 0)
        return set_error(PQP_ERR_ARG, "%s: the handle was made by pqp_shared_create and has no plant "
                                      "matrices (use pqp_shared_create_plant)", fn);
    PQP_TRY(check_budget(fn, max_updates, p->N, p->M, "pqp_shared_max_updates", "launch"));
    SharedStepArgs t{shared_core_args(*p)};  // (t.solve, built in place; every member after it zeroed)
    SharedSolveCore& a = t.solve;
    a.Fd = d_Fd, a.Fp = d_Fp, a.KpB = d_Kp;  // Md, Mp: the kernel's own words
    a.Y = d_Y, a.U = d_U, a.h = d_h, a.status = d_status, a.Jp = d_Jp, a.Jd = d_Jd;
    a.B = B;
    a.max_updates = max_updates;
    t.abs_tol = abs_tol, t.rel_tol = rel_tol;
    a.chunk = max_updates;  // every state finishes within it
    t.Fp1T = p->Fp1T.f(), t.Fp2T = p->Fp2T.f(), t.Fp3 = p->Fp3.f();
    t.Mp1P = p->Mp1P.f(), t.Mp2P = p->Mp2P.f(), t.Mp3P = p->Mp3P.f();
    t.Mp4 = p->Mp4.f(), t.Mp5 = p->Mp5.f(), t.Mp6 = p->Mp6.f();
    t.GQT = p->GQT.f(), t.QinvR = p->QinvR.f();
    t.x = d_x, t.D = d_D, t.Fp = d_Fp, t.Fd = d_Fd, t.Mp = d_Mp, t.Md = d_Md;
    t.nd = p->nd, t.ns = p->ns, t.warm = warm ? 1 : 0;
    DeviceGuard on(p->dev);
    PQP_HIP(launch_step_shared(t, p->S, static_cast<hipStream_t>(stream)));
    return PQP_OK;
}

int pqp_shared_step(pqp_shared* p, int B, const float* d_x, const float* d_D, const float* d_Kp, int warm,
                    long long max_updates, float* d_Y, float* d_U, long long* d_h, int* d_status, float* d_Fp,
                    float* d_Mp, float* d_Fd, float* d_Md, float* d_Jp, float* d_Jd, void* stream) {
    return shared_step("pqp_shared_step", p, B, d_x, d_D, d_Kp, warm, max_updates, d_Y, d_U, d_h, d_status, d_Fp, d_Mp,
                       d_Fd, d_Md, d_Jp, d_Jd, 0.0f, 0.0f, stream);
}

int pqp_shared_step_tol(pqp_shared* p, int B, const float* d_x, const float* d_D, const float* d_Kp, int warm,
                        long long max_updates, float* d_Y, float* d_U, long long* d_h, int* d_status, float* d_Fp,
                        float* d_Mp, float* d_Fd, float* d_Md, float* d_Jp, float* d_Jd, float abs_tol, float rel_tol,
                        void* stream) {
    return shared_step("pqp_shared_step_tol", p, B, d_x, d_D, d_Kp, warm, max_updates, d_Y, d_U, d_h, d_status, d_Fp,
                       d_Mp, d_Fd, d_Md, d_Jp, d_Jd, abs_tol, rel_tol, stream);
}

// ---------------------------------------------------------------------------
// 2k. the gap-tolerance stopping rule: the predicate itself, on the host
// ---------------------------------------------------------------------------
int pqp_stop_decide(float Jp, float Jd, float abs_tol, float rel_tol) { return pqp::stop_decide(Jp, Jd, abs_tol, rel_tol); }

// ---------------------------------------------------------------------------
// 1. drop-in entry points (reference signatures)
// ---------------------------------------------------------------------------
void solveQuadraticDual(float* Y, float* Qd, float* Fd, float* Md, float* U, float* Qp, float* Qp_inv, float* Fp,
                        float* Mp, float* Gp, float* Kp, int N, int M) {
    long long h = 0;
    long long cap = 0;  // the reference has no cap (PQP_CPU.c:718); PQP_MAX_UPDATES adds one
    if (const char* env = std::getenv("PQP_MAX_UPDATES")) cap = std::atoll(env);
    int rc = pqp_solve_dual(Qd, Fd, Md, Qp, Qp_inv, Fp, Mp, Gp, Kp, N, M, PQP_MODE_CONVERGE, 0, cap, Y, U, &h,
                            nullptr, nullptr);
    if (rc != PQP_OK && rc != PQP_ERR_NOT_CONVERGED) die("solveQuadraticDual");
    std::printf("Printing number of iterations = %ld\n", (long)h);
}

void updateY2(float* Y_next, float* Y, float* Qdp_theta, float* Qdn_theta, float* Fd, float* Fdp, float* Fdn,
              int N) {
    (void)Fd;
    auto run = [&]() -> int {
        if (N <= 0) return set_error(PQP_ERR_ARG, "updateY2: N must be positive");
        PQP_TRY(ensure_device());
        hipStream_t s = lib_stream();
        const int ldq = round4(N);
        DevBuf qp, qn, qpT, qnT, fdp, fdn, y, yn;
        PQP_TRY(upload(qp, Qdp_theta, (size_t)N * N, s));
        PQP_TRY(upload(qn, Qdn_theta, (size_t)N * N, s));
        PQP_TRY(upload(fdp, Fdp, N, s));
        PQP_TRY(upload(fdn, Fdn, N, s));
        PQP_TRY(upload(y, Y, N, s));
        PQP_TRY(yn.floats(N));
        PQP_TRY(qpT.floats((size_t)N * ldq));
        PQP_TRY(qnT.floats((size_t)N * ldq));
        PQP_HIP(launch_pack_colmajor(1, qp.f(), N, (long long)N * N, qpT.f(), ldq, (long long)N * ldq, s));
        PQP_HIP(launch_pack_colmajor(1, qn.f(), N, (long long)N * N, qnT.f(), ldq, (long long)N * ldq, s));
        PQP_HIP(launch_update_split(qpT.f(), qnT.f(), ldq, N, fdp.f(), fdn.f(), y.f(), yn.f(), s));
        PQP_TRY(download(Y_next, yn.p, N, s));
        PQP_HIP(hipStreamSynchronize(s));
        return PQP_OK;
    };
    if (run() != PQP_OK) die("updateY2");
}

int terminate(float* Y, float* Qd, float* Fd, float* Md, float* U, float* Qp, float* Qp_inv, float* Fp, float* Mp,
              float* Gp, float* Kp, int N, int M) {
    int result = 0;
    auto run = [&]() -> int {
        PQP_TRY(check_dims(N, M));
        PQP_TRY(ensure_device());
        hipStream_t s = lib_stream();
        pqp_problem P;
        PQP_TRY(problem_upload(P, Qd, Fd, Md, Qp, Qp_inv, Fp, Mp, Gp, Kp, N, M, s));
        PQP_HIP(hipMemcpyAsync(P.Y.p, Y, sizeof(float) * N, hipMemcpyHostToDevice, s));
        SolveOut o;
        PQP_TRY(problem_run(P, kModeTerminate, 0, 0, true, o, s));
        PQP_TRY(download(U, P.U.p, M, s));
        PQP_HIP(hipStreamSynchronize(s));
        result = o.last_stop;
        return PQP_OK;
    };
    if (run() != PQP_OK) die("terminate");
    return result;
}

void convertToDual(float* Qd, float* Fd, float* Md, float* Qp_inv, float* Gp, float* Kp, float* Fp, float* Mp, int N,
                   int M) {
    auto run = [&]() -> int {
        PQP_TRY(check_dims(N, M));
        PQP_TRY(ensure_device());
        hipStream_t s = lib_stream();
        DevBuf qinv, gp, kp, fp, mp, qd, fd, md;
        PQP_TRY(upload(qinv, Qp_inv, (size_t)M * M, s));
        PQP_TRY(upload(gp, Gp, (size_t)N * M, s));
        PQP_TRY(upload(kp, Kp, N, s));
        PQP_TRY(upload(fp, Fp, M, s));
        PQP_TRY(upload(mp, Mp, 1, s));
        PQP_TRY(qd.floats((size_t)N * N));
        PQP_TRY(fd.floats(N));
        PQP_TRY(md.floats(1));
        PQP_TRY(dev_convert_to_dual(qd.f(), fd.f(), md.f(), qinv.f(), gp.f(), kp.f(), fp.f(), mp.f(), N, M, s));
        PQP_TRY(download(Qd, qd.p, (size_t)N * N, s));
        PQP_TRY(download(Fd, fd.p, N, s));
        PQP_TRY(download(Md, md.p, 1, s));
        PQP_HIP(hipStreamSynchronize(s));
        return PQP_OK;
    };
    if (run() != PQP_OK) die("convertToDual");
}

void computeUfromY(float* U, float* Y, float* Fp, float* Gp, float* Qp_inv, int N, int M) {
    auto run = [&]() -> int {
        PQP_TRY(check_dims(N, M));
        PQP_TRY(ensure_device());
        hipStream_t s = lib_stream();
        DevBuf u, y, fp, gp, qinv;
        PQP_TRY(upload(y, Y, N, s));
        PQP_TRY(upload(fp, Fp, M, s));
        PQP_TRY(upload(gp, Gp, (size_t)N * M, s));
        PQP_TRY(upload(qinv, Qp_inv, (size_t)M * M, s));
        PQP_TRY(u.floats(M));
        PQP_TRY(dev_u_from_y(u.f(), y.f(), fp.f(), gp.f(), qinv.f(), N, M, s));
        PQP_TRY(download(U, u.p, M, s));
        PQP_HIP(hipStreamSynchronize(s));
        return PQP_OK;
    };
    if (run() != PQP_OK) die("computeUfromY");
}

float computeCost(float* Z, float* Q, float* F, float* Mc, int N) {
    float J = 0.0f;
    auto run = [&]() -> int {
        if (N <= 0) return set_error(PQP_ERR_ARG, "computeCost: N must be positive");
        PQP_TRY(ensure_device());
        hipStream_t s = lib_stream();
        DevBuf z, q, f, m, j;
        PQP_TRY(upload(z, Z, N, s));
        PQP_TRY(upload(q, Q, (size_t)N * N, s));
        PQP_TRY(upload(f, F, N, s));
        PQP_TRY(upload(m, Mc, 1, s));
        PQP_TRY(j.floats(1));
        PQP_TRY(dev_cost(j.f(), z.f(), q.f(), f.f(), m.f(), N, s));
        PQP_TRY(download(&J, j.p, 1, s));
        PQP_HIP(hipStreamSynchronize(s));
        return PQP_OK;
    };
    if (run() != PQP_OK) die("computeCost");
    return J;
}

int checkFeas(float* U, float* Gp, float* Kp, int N, int M) {
    int flag = 0;
    auto run = [&]() -> int {
        PQP_TRY(check_dims(N, M));
        PQP_TRY(ensure_device());
        hipStream_t s = lib_stream();
        DevBuf u, gp, kp;
        PQP_TRY(upload(u, U, M, s));
        PQP_TRY(upload(gp, Gp, (size_t)N * M, s));
        PQP_TRY(upload(kp, Kp, N, s));
        return dev_check_feas(u.f(), gp.f(), kp.f(), N, M, &flag, s);
    };
    if (run() != PQP_OK) die("checkFeas");
    return flag;
}

void computeTheta(float* theta, float* Qd, int N) {
    auto run = [&]() -> int {
        if (N <= 0) return set_error(PQP_ERR_ARG, "computeTheta: N must be positive");
        PQP_TRY(ensure_device());
        hipStream_t s = lib_stream();
        DevBuf th, qd;
        PQP_TRY(upload(th, theta, (size_t)N * N, s));
        PQP_TRY(upload(qd, Qd, (size_t)N * N, s));
        PQP_HIP(launch_theta_rowmajor(qd.f(), N, th.f(), s));
        PQP_TRY(download(theta, th.p, (size_t)N * N, s));
        PQP_HIP(hipStreamSynchronize(s));
        return PQP_OK;
    };
    if (run() != PQP_OK) die("computeTheta");
}

void matrixMultiply(float* output, float* mat1, int transpose1, float* mat2, int transpose2, int a, int b, int c) {
    auto run = [&]() -> int {
        if (a <= 0 || b < 0 || c <= 0) return set_error(PQP_ERR_ARG, "matrixMultiply: bad sizes");
        PQP_TRY(ensure_device());
        hipStream_t s = lib_stream();
        DevBuf A, B, O;
        PQP_TRY(upload(A, mat1, (size_t)a * b, s));
        PQP_TRY(upload(B, mat2, (size_t)b * c, s));
        PQP_TRY(O.floats((size_t)a * c));
        PQP_TRY(dev_matmul(O.f(), A.f(), transpose1, B.f(), transpose2, a, b, c, s));
        PQP_TRY(download(output, O.p, (size_t)a * c, s));
        PQP_HIP(hipStreamSynchronize(s));
        return PQP_OK;
    };
    if (run() != PQP_OK) die("matrixMultiply");
}

void Gauss_Jordan(float* A, float* res, int N) {
    auto run = [&]() -> int {
        if (N <= 0) return set_error(PQP_ERR_ARG, "Gauss_Jordan: N must be positive");
        PQP_TRY(ensure_device());
        hipStream_t s = lib_stream();
        DevBuf a, r;
        PQP_TRY(upload(a, A, (size_t)N * N, s));
        PQP_TRY(r.floats((size_t)N * N));
        PQP_TRY(dev_gauss_jordan(r.f(), a.f(), N, s));
        PQP_TRY(download(res, r.p, (size_t)N * N, s));
        PQP_HIP(hipStreamSynchronize(s));
        return PQP_OK;
    };
    if (run() != PQP_OK) die("Gauss_Jordan");
}

void computeFp(float* Fp, float* Fp1, float* Fp2, float* Fp3, float* D, float* x) {
    const int m = kRefNInput * kRefPHorizon, nd = kRefNDis * kRefPHorizon, ns = kRefNState;
    auto run = [&]() -> int {
        PQP_TRY(ensure_device());
        hipStream_t s = lib_stream();
        DevBuf fp, f1, f2, f3, d, xx;
        PQP_TRY(upload(f1, Fp1, (size_t)m * nd, s));
        PQP_TRY(upload(f2, Fp2, (size_t)m * ns, s));
        PQP_TRY(upload(f3, Fp3, m, s));
        PQP_TRY(upload(d, D, nd, s));
        PQP_TRY(upload(xx, x, ns, s));
        PQP_TRY(fp.floats(m));
        PQP_TRY(dev_compute_fp(fp.f(), f1.f(), f2.f(), f3.f(), d.f(), xx.f(), m, nd, ns, s));
        PQP_TRY(download(Fp, fp.p, m, s));
        PQP_HIP(hipStreamSynchronize(s));
        return PQP_OK;
    };
    if (run() != PQP_OK) die("computeFp");
}

void computeMp(float* Mp, float* Mp1, float* Mp2, float* Mp3, float* Mp4, float* Mp5, float* Mp6, float* D,
               float* x) {
    const int nd = kRefNDis * kRefPHorizon, ns = kRefNState;
    auto run = [&]() -> int {
        PQP_TRY(ensure_device());
        hipStream_t s = lib_stream();
        DevBuf mp, m1, m2, m3, m4, m5, m6, d, xx;
        PQP_TRY(upload(m1, Mp1, (size_t)ns * ns, s));
        PQP_TRY(upload(m2, Mp2, (size_t)nd * ns, s));
        PQP_TRY(upload(m3, Mp3, (size_t)nd * nd, s));
        PQP_TRY(upload(m4, Mp4, ns, s));
        PQP_TRY(upload(m5, Mp5, nd, s));
        PQP_TRY(upload(m6, Mp6, 1, s));
        PQP_TRY(upload(d, D, nd, s));
        PQP_TRY(upload(xx, x, ns, s));
        PQP_TRY(mp.floats(1));
        PQP_TRY(dev_compute_mp(mp.f(), m1.f(), m2.f(), m3.f(), m4.f(), m5.f(), m6.f(), d.f(), xx.f(), nd, ns, s));
        PQP_TRY(download(Mp, mp.p, 1, s));
        PQP_HIP(hipStreamSynchronize(s));
        return PQP_OK;
    };
    if (run() != PQP_OK) die("computeMp");
}

void input(float* qp_inv, float* Fp1, float* Fp2, float* Fp3, float* Mp1, float* Mp2, float* Mp3, float* Mp4,
           float* Mp5, float* Mp6, float* Gp, float* Kp, float* x, float* D, float* theta, float* Z) {
    const int m = kRefNInput * kRefPHorizon, nd = kRefNDis * kRefPHorizon, ns = kRefNState;
    if (pqp_read_example("./example", m, nd, ns, qp_inv, Fp1, Fp2, Fp3, Mp1, Mp2, Mp3, Mp4, Mp5, Mp6, Gp, Kp, x, D) !=
            PQP_OK ||
        read_unused_example("./example", ns, kRefNOutput * kRefPHorizon, nd, Z, theta) != PQP_OK)
        die("input");
}

}  // extern "C"

// ---------------------------------------------------------------------------
// tuning / diagnostics (include/pqp_tuning.h)
// ---------------------------------------------------------------------------
#include "../../include/pqp_tuning.h"

namespace {
// key -> knob of pqp::g_tune (pqp_tune / pqp_tune_get)
struct KnobRef {
    const char* key;
    int* i;
    bool* b;
    long long* ll;
};
const KnobRef* find_knob(const char* key) {
    using pqp::g_tune;
    static const KnobRef knobs[] = {
        {"relay_spin_max", &g_tune.relay_spin_max, nullptr, nullptr},
        {"lean_min_n", &g_tune.lean_min_n, nullptr, nullptr},
        {"split_lw", &g_tune.split_lw, nullptr, nullptr},
        {"wave_pipe_max_b", &g_tune.wave_pipe_max_b, nullptr, nullptr},
        {"fixed_rl_max_b", &g_tune.fixed_rl_max_b, nullptr, nullptr},
        {"wave_min_b", &g_tune.wave_min_b, nullptr, nullptr},
        {"matmul_tiled_off", &g_tune.matmul_tiled_off, nullptr, nullptr},
        {"gj_blocked_off", &g_tune.gj_blocked_off, nullptr, nullptr},
        {"single_scalar", &g_tune.single_scalar, nullptr, nullptr},
        {"persist_off", &g_tune.persist_off, nullptr, nullptr},
        {"persist_stall_wg", &g_tune.persist_stall_wg, nullptr, nullptr},
        {"persist_fit_cus", &g_tune.persist_fit_cus, nullptr, nullptr},
        {"converge_persist_off", &g_tune.converge_persist_off, nullptr, nullptr},
        {"force_small", nullptr, &g_tune.force_small, nullptr},
        {"force_single", nullptr, &g_tune.force_single, nullptr},
        {"wide_min_n", &g_tune.wide_min_n, nullptr, nullptr},
        {"batch_opts", &g_tune.batch_opts, nullptr, nullptr},
        {"mid_off", &g_tune.mid_off, nullptr, nullptr},
        {"pipe_off", &g_tune.pipe_off, nullptr, nullptr},
        {"mid_v1", &g_tune.mid_v1, nullptr, nullptr},
        {"mid2_pair", &g_tune.mid2_pair, nullptr, nullptr},
        {"mid2_min_n", &g_tune.mid2_min_n, nullptr, nullptr},
        {"mid2_dense", &g_tune.mid2_dense, nullptr, nullptr},
        {"single_occ", &g_tune.single_occ, nullptr, nullptr},
        {"matmul_pk_off", &g_tune.matmul_pk_off, nullptr, nullptr},
        {"pipe_variant", &g_tune.pipe_variant, nullptr, nullptr},
        {"pipe_force", &g_tune.pipe_force, nullptr, nullptr},
        {"batch_chunk", nullptr, nullptr, &g_tune.batch_chunk},
        {"converge_chunk", nullptr, nullptr, &g_tune.converge_chunk},
        {"tiny_old", &g_tune.tiny_old, nullptr, nullptr},
        {"tiny_dense", &g_tune.tiny_dense, nullptr, nullptr},
        {"tiny_stall", &g_tune.tiny_stall, nullptr, nullptr},
        {"tiny_fallback", &g_tune.tiny_fallback, nullptr, nullptr},
        {"tiny_np", &g_tune.tiny_np, nullptr, nullptr},
        {"tiny_ablk", &g_tune.tiny_ablk, nullptr, nullptr},
        {"tiny_apoll", &g_tune.tiny_apoll, nullptr, nullptr},
        {"persist_xcds", &g_tune.persist_xcds, nullptr, nullptr},
        {"converge_xcds", &g_tune.converge_xcds, nullptr, nullptr},
        {"tiny_chunk", nullptr, nullptr, &g_tune.tiny_chunk},
        {"iterate_kind", &g_tune.iterate_kind, nullptr, nullptr},
        {"iterate_half", &g_tune.iterate_half, nullptr, nullptr},
        {"plant_grid", &pqp::g_plant_grid, nullptr, nullptr},
        {"plant_pipe", &pqp::g_plant_pipe, nullptr, nullptr},
        {"plant_roll_chain", &pqp::g_plant_roll_chain, nullptr, nullptr},
    };
    for (const KnobRef& k : knobs)
        if (std::strcmp(k.key, key) == 0) return &k;
    return nullptr;
}
long long knob_value(const KnobRef& k) { return k.i ? *k.i : (k.b ? (long long)*k.b : *k.ll); }
}  // namespace

namespace pqp {
// iterates per problem per batched-solve launch: about 2^28 element updates per
// problem (56 at n_dual 1024, M 512: each launch's start -- its first Gp'Y
// pass, the state, the host's check of the pending count -- cost about a
// quarter (infeasible) to 1.4 (feasible) iterates at 2^26:
// profiles/r04/pipe/launch_amortization.json), or the batch_chunk knob
long long batch_chunk_for(int N, int M) {
    return g_tune.batch_chunk > 0 ? g_tune.batch_chunk : updates_per_launch(N, M, 1 << 28, 1);
}
}  // namespace pqp

static std::mutex g_tune_mu;  // pqp_tune / pqp_tune_trace writers

extern "C" int pqp_tune(const char* key, long long value, long long* old_value) {
    // writers are serialized; readers (the launches) take no lock: the knobs
    // are test and tuning hooks that must not change while another thread is
    // inside a solve (include/pqp_tuning.h)
    std::lock_guard<std::mutex> lk(g_tune_mu);
    const KnobRef* k = key ? find_knob(key) : nullptr;
    if (!k) return pqp::set_error(PQP_ERR_ARG, "pqp_tune: unknown key '%s'", key ? key : "(null)");
    if (old_value) *old_value = knob_value(*k);
    if (std::strcmp(key, "relay_spin_max") == 0) {
        // 0 restores the default; clamped: a budget near INT_MAX would let a
        // broken hand-off spin until its counter overflows
        value = value == 0 ? pqp::kRelaySpinMax : (value > (1 << 30) ? (1 << 30) : value);
    } else if (std::strcmp(key, "converge_chunk") == 0) {
        value = value > 0 ? value : (1 << 16);
    } else if (std::strcmp(key, "persist_stall_wg") == 0) {
        value = value >= 0 ? value : -1;
    } else if (std::strcmp(key, "iterate_half") == 0) {
        value = (value >= 0 && value <= 2) ? value : 1;  // 0 forward, 1 product-first, 2 lean only
    }
    if (k->i) *k->i = (int)value;
    else if (k->b) *k->b = value != 0;
    else *k->ll = value;
    return PQP_OK;
}

extern "C" int pqp_tune_get(const char* key, long long* value) {
    if (!key || !value) return pqp::set_error(PQP_ERR_ARG, "pqp_tune_get: null argument");
    if (std::strcmp(key, "last_path") == 0) {
        *value = pqp::g_last_path;
        return PQP_OK;
    }
    if (std::strcmp(key, "last_batch_kernel") == 0) {  // 1: k_solve_pipe, 0: k_solve_single (path 2)
        *value = pqp::g_last_batch_kernel;
        return PQP_OK;
    }
    if (std::strcmp(key, "tiny_stale") == 0) {  // tiny solves whose pinned output lacked their tag
        *value = pqp::g_tiny_stale;
        return PQP_OK;
    }
    if (std::strcmp(key, "persist_fallbacks") == 0) {
        *value = pqp::g_persist_fallbacks;
        return PQP_OK;
    }
    if (std::strcmp(key, "batch_chunk_for") == 0) {  // in: N << 32 | M; out: iterates per batched launch
        const long long v = *value;
        *value = pqp::batch_chunk_for((int)(v >> 32), (int)(v & 0xffffffff));
        return PQP_OK;
    }
    if (std::strcmp(key, "plant_slots") == 0) {  // in: N | M << 8 | nd << 16 | ns << 24 | pipe << 32
        // out: pqp_plant_step's workgroups resident at once on the current device (its default grid's bound)
        const long long v = *value;
        const int N = (int)(v & 255), M = (int)(v >> 8 & 255), nd = (int)(v >> 16 & 255), ns = (int)(v >> 24 & 255);
        if (!pqp::plant_shape_ok(N, M, nd, ns)) return pqp::set_error(PQP_ERR_ARG, "pqp_tune_get: plant_slots of an unsupported shape");
        PQP_TRY(pqp::ensure_device());
        *value = pqp::plant_resident_wgs(N, M, nd, ns, (v >> 32 & 1) != 0);
        return PQP_OK;
    }
    if (std::strcmp(key, "plant_widths") == 0) {  // in: N | M << 8; out: NMAX | MMAX << 8 of k_plant_step's instantiation (host only)
        const long long v = *value;
        const int N = (int)(v & 255), M = (int)(v >> 8 & 255);
        if ((v >> 16) != 0 || !pqp::plant_shape_ok(N, M, 1, 1))
            return pqp::set_error(PQP_ERR_ARG, "pqp_tune_get: plant_widths of N=%d, M=%d: not a one-wave plant's shape", N, M);
        *value = pqp::plant_widths(N, M);
        return PQP_OK;
    }
    if (std::strcmp(key, "plant_mid_build") == 0) {  // in: N; out: threads | pair << 16 | lean << 17 | band << 18 of k_plant_step_mid's build (host only)
        const long long v = *value;
        if (v < 1 || v > 192)  // plant_mid_shape_ok's range of N (M decides the rest, not the build)
            return pqp::set_error(PQP_ERR_ARG, "pqp_tune_get: plant_mid_build of N=%lld: not a one-workgroup plant's N", v);
        *value = pqp::plant_mid_build((int)v);
        return PQP_OK;
    }
    if (std::strcmp(key, "plant_mid_lds") == 0) {  // in: N << 32 | M; out: bytes of LDS of the one-workgroup plant step (host only)
        const long long v = *value;
        const int N = (int)(v >> 32), M = (int)(v & 0xffffffff);
        if (N < 1 || M < 1 || N > 4096 || M > 4096) return pqp::set_error(PQP_ERR_ARG, "pqp_tune_get: plant_mid_lds of N=%d, M=%d", N, M);
        *value = (long long)pqp::plant_mid_lds_bytes(N, M);
        return PQP_OK;
    }
    if (std::strcmp(key, "converge_grid") == 0) {  // in: N << 32 | M
        const long long v = *value;
        *value = pqp::converge_persist_wgs((int)(v >> 32), (int)(v & 0xffffffff), nullptr);
        return PQP_OK;
    }
    const KnobRef* k = find_knob(key);
    if (!k) return pqp::set_error(PQP_ERR_ARG, "pqp_tune_get: unknown key '%s'", key);
    *value = knob_value(*k);
    return PQP_OK;
}

extern "C" int pqp_tune_trace(const char* what, void* d_buf, int n) {
    if (!what || n < 0 || (n > 0 && !d_buf)) return pqp::set_error(PQP_ERR_ARG, "pqp_tune_trace: bad arguments");
    auto* buf = n > 0 ? static_cast<unsigned long long*>(d_buf) : nullptr;
    std::lock_guard<std::mutex> lk(g_tune_mu);
    if (std::strcmp(what, "persist") == 0) {
        pqp::g_tune.persist_trace = buf;
        pqp::g_tune.persist_trace_n = n;
    } else if (std::strcmp(what, "mid") == 0) {
        pqp::g_tune.mid_trace = buf;
        pqp::g_tune.mid_trace_n = n;
    } else if (std::strcmp(what, "tiny") == 0) {
        // k_solve_quintet<..., true> writes kTinyTraceWords words unconditionally
        if (n > 0 && n < pqp::kTinyTraceWords)
            return pqp::set_error(PQP_ERR_ARG, "pqp_tune_trace: the tiny timeline needs %d words", pqp::kTinyTraceWords);
        pqp::g_tune.tiny_trace = buf;
    } else if (std::strcmp(what, "converge") == 0) {
        pqp::g_tune.converge_trace = buf;
        pqp::g_tune.converge_trace_n = n;
    } else {
        return pqp::set_error(PQP_ERR_ARG, "pqp_tune_trace: unknown timeline '%s'", what);
    }
    return PQP_OK;
}

extern "C" int pqp_tune_poison_lds(float value) {
    PQP_TRY(pqp::ensure_device());
    hipStream_t s = pqp::lib_stream();
    int dev = 0, cus = 0;
    PQP_HIP(hipGetDevice(&dev));
    PQP_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    pqp::DevBuf seen;
    PQP_TRY(seen.alloc(sizeof(int)));
    int bits;
    std::memcpy(&bits, &value, sizeof bits);
    PQP_HIP(pqp::launch_poison_lds(bits, static_cast<int*>(seen.p), cus, s));
    PQP_HIP(hipStreamSynchronize(s));
    return PQP_OK;
}

extern "C" int pqp_tune_glibc_rand(int n, int* out) {
    if (n < 0 || (n > 0 && !out)) return pqp::set_error(PQP_ERR_ARG, "pqp_tune_glibc_rand: bad arguments");
    return pqp::glibc_rand_sequence(n, out);
}
