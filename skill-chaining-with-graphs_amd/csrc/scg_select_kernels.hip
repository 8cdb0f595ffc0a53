// scg_select_kernels.hip — the value-ranking instantiations of rollout_kernel (SPEC §14: scg_rollout_select with SCG_SELECT_BEST),
// without and with SPEC §11's interruption, both with the record argument, and their launches.
//
// A translation unit of their own, for scg_record_kernels.hip's reason: the instantiations that existed before keep the code they
// compiled to (DESIGN §3.17's resource table). The C-ABI entry point and its checks are in scg_kernels.hip.
#include "scg_device.hpp"
#include "../../include/scg_abi.h"

using namespace scg;
typedef float f4v __attribute__((ext_vector_type(4)));

#include "scg_eval.hpp"
#include "scg_rollout_kernel.hpp"

hipError_t launch_rollout_best(const RolloutBestArgs &A, int grid, hipStream_t s) {
    hipLaunchKernelGGL((rollout_kernel<true, RolloutBestArgs>), dim3(grid), dim3(RO_THREADS), 0, s, A);
    return hipGetLastError();
}

hipError_t launch_rollout_best_interrupt(const RolloutBestIntArgs &A, int grid, hipStream_t s) {
    hipLaunchKernelGGL((rollout_kernel<true, RolloutBestIntArgs>), dim3(grid), dim3(RO_THREADS), 0, s, A);
    return hipGetLastError();
}
