// scg_rollout_variants.hip — every instantiation of rollout_kernel but scg_rollout's plain one (the table in scg_rollout_kernel.hpp:
// SPEC §10's record, §11's interruption, §14's value-ranked choice, §15's audit with §19's forced first action), trial_kernel<true>
// (SPEC §10), and their launches.
//
// They are apart from scg_kernels.hip because what shares a module with rollout_kernel<false, RolloutArgs> and trial_kernel<false>
// changes the gfx950 code of those two (two shifts of a known non-negative value came out signed). Among themselves
// they do not: together here, each compiles to the code it had in a unit of its own. The C-ABI entry points, their
// checks and the plain launches stay in scg_kernels.hip.
#include "scg_device.hpp"
#include "../../include/scg_abi.h"

using namespace scg;
typedef float f4v __attribute__((ext_vector_type(4)));

#include "scg_eval.hpp"
#include "scg_rollout_kernel.hpp"
#include "scg_trial_kernel.hpp"

template <bool REC, typename Args>
hipError_t launch_rollout(const Args &A, int grid, hipStream_t s) {
    hipLaunchKernelGGL((rollout_kernel<REC, Args>), dim3(grid), dim3(RO_THREADS), 0, s, A);
    return hipGetLastError();
}
template hipError_t launch_rollout<false, RolloutIntArgs>(const RolloutIntArgs &, int, hipStream_t);
#define SCG_VARIANT(I, B, AU) \
    template hipError_t launch_rollout<true, RolloutVar<I, B, AU>>(const RolloutVar<I, B, AU> &, int, hipStream_t);
SCG_VARIANT(false, false, false) SCG_VARIANT(true, false, false) SCG_VARIANT(false, true, false) SCG_VARIANT(true, true, false)
SCG_VARIANT(false, false, true) SCG_VARIANT(true, false, true) SCG_VARIANT(false, true, true) SCG_VARIANT(true, true, true)
#undef SCG_VARIANT

hipError_t launch_trial_record(const TrialRecArgs &A, int grid, hipStream_t s) {
    hipLaunchKernelGGL((trial_kernel<true, TrialRecArgs>), dim3(grid), dim3(RO_THREADS), 0, s, A);
    return hipGetLastError();
}
