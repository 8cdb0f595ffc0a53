// scg_record_kernels.hip — the recording instantiations rollout_kernel<true> and trial_kernel<true> (SPEC §10), the interrupting
// instantiations of rollout_kernel (SPEC §11), and their launches.
//
// They live in a translation unit of their own: compiled into the same module as the plain instantiations, they changed the gfx950
// code of scg_rollout's kernel (two shifts of a known non-negative value came out signed). Apart, rollout_kernel<false> and
// trial_kernel<false> compile instruction for instruction to the kernels they were before recording existed. The C-ABI entry
// points, their checks and the plain launches stay in scg_kernels.hip.
#include "scg_device.hpp"
#include "../../include/scg_abi.h"

using namespace scg;
typedef float f4v __attribute__((ext_vector_type(4)));

#include "scg_eval.hpp"
#include "scg_rollout_kernel.hpp"
#include "scg_trial_kernel.hpp"

hipError_t launch_rollout_record(const RolloutRecArgs &A, int grid, hipStream_t s) {
    hipLaunchKernelGGL((rollout_kernel<true, RolloutRecArgs>), dim3(grid), dim3(RO_THREADS), 0, s, A);
    return hipGetLastError();
}

// the interrupting instantiations (SPEC §11), without and with the record: INT comes with the argument type
hipError_t launch_rollout_interrupt(const RolloutIntArgs &A, int grid, hipStream_t s) {
    hipLaunchKernelGGL((rollout_kernel<false, RolloutIntArgs>), dim3(grid), dim3(RO_THREADS), 0, s, A);
    return hipGetLastError();
}

hipError_t launch_rollout_interrupt_record(const RolloutIntRecArgs &A, int grid, hipStream_t s) {
    hipLaunchKernelGGL((rollout_kernel<true, RolloutIntRecArgs>), dim3(grid), dim3(RO_THREADS), 0, s, A);
    return hipGetLastError();
}

hipError_t launch_trial_record(const TrialRecArgs &A, int grid, hipStream_t s) {
    hipLaunchKernelGGL((trial_kernel<true, TrialRecArgs>), dim3(grid), dim3(RO_THREADS), 0, s, A);
    return hipGetLastError();
}
