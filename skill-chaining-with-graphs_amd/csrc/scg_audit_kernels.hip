// scg_audit_kernels.hip — the audited instantiations of rollout_kernel (SPEC §15: scg_rollout_audit), one per `rules` of
// scg_rollout_select (0, INTERRUPT, BEST, BEST | INTERRUPT), all with the record argument, and their launch.
//
// A translation unit of their own, for scg_record_kernels.hip's reason: the instantiations that existed before keep the code they
// compiled to (DESIGN §3.19's resource table). The C-ABI entry point and its checks are in scg_kernels.hip.
#include "scg_device.hpp"
#include "../../include/scg_abi.h"

using namespace scg;
typedef float f4v __attribute__((ext_vector_type(4)));

#include "scg_eval.hpp"
#include "scg_rollout_kernel.hpp"

template <bool I, bool B>
static hipError_t launch(const RolloutAuditArgs<I, B> &A, int grid, hipStream_t s) {
    hipLaunchKernelGGL((rollout_kernel<true, RolloutAuditArgs<I, B>>), dim3(grid), dim3(RO_THREADS), 0, s, A);
    return hipGetLastError();
}

hipError_t launch_rollout_audit(const RolloutAuditArgs<false, false> &A, int grid, hipStream_t s) { return launch(A, grid, s); }
hipError_t launch_rollout_audit(const RolloutAuditArgs<true, false> &A, int grid, hipStream_t s) { return launch(A, grid, s); }
hipError_t launch_rollout_audit(const RolloutAuditArgs<false, true> &A, int grid, hipStream_t s) { return launch(A, grid, s); }
hipError_t launch_rollout_audit(const RolloutAuditArgs<true, true> &A, int grid, hipStream_t s) { return launch(A, grid, s); }
