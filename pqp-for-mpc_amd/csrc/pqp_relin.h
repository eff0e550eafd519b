// pqp_relin.h -- internal interface of the relinearization kernels
// (pqp_relin.hip) to the host shim.  Not part of the C ABI.  (Beside
// pqp_launch.h, not in it: that header's text is part of the key of the
// kernels' recorded counter measurements, which these declarations do not
// touch.)
#pragma once
#include "pqp_launch.h"

namespace pqp {

// New Fd / Md from new Fp, Mp, Kp with GQ = Gp Qp_inv kept.  GQ (B*N*M
// floats, 16-byte aligned) is in k_relin_pack's layout: packets of 4 k per
// row, each wave's 64 rows contiguous and k-major.
hipError_t launch_relin_pack(int B, int N, int M, const float* GQ_rowmajor, float* GQ, hipStream_t s);
// one launch, nothing else: Fd [B][N], Md [B]
hipError_t launch_relinearize(int B, int N, int M, const float* GQ, const float* Qinv, const float* Kp,
                              const float* Fp, const float* Mp, float* Fd, float* Md, hipStream_t s);
// {Fdn, Fdp} into a problem's fdpn arrays (k_build_split's layout) and lean aux words (k_build_lean's); nulls skipped
hipError_t launch_relin_refresh(const float* Fd, int N, float* fdpn0, float* fdpn1, float* aux, hipStream_t s);
// launch_state_init for a warm start: h = 1 and resume = 1, every problem starts from the iterate in SolveArgs::Y
hipError_t launch_state_init_warm(int B, SolveState* st, hipStream_t s);

}  // namespace pqp
