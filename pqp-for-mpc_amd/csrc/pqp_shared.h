// pqp_shared.h -- internal interface of the shared-Qd batched update
// (pqp_shared.hip) to the host shim.  Not part of the C ABI.  (Beside
// pqp_launch.h, not in it: that header's text is part of the key of the
// kernels' recorded counter measurements, which these declarations do not
// touch.)
#pragma once
#include "pqp_launch.h"

namespace pqp {

// States per workgroup k_batch_shared uses for the shape; 0 where it is not supported.
int batch_shared_states(int N, int ldq);
// B states of ONE problem: QdT [N][ldq], theta [N]; Fd, Y0 (may be null or Y), Y [B][ldv]
hipError_t launch_batch_shared(int B, const float* QdT, int ldq, int N, const float* theta, const float* Fd, int ldv,
                               const float* Y0, float* Y, int updates, hipStream_t s);

}  // namespace pqp
