// scg_rollout_population.hip — the five POP instantiations of rollout_kernel (SPEC §21: RolloutPop<INT, BEST>, AUDIT throughout;
// SPEC §25.1: RolloutPopGateArgs; the table in scg_rollout_kernel.hpp) and their launch.
//
// A unit of their own, for the reason scg_rollout_variants.hip is apart from scg_kernels.hip: what shares a module with a kernel
// may change that kernel's gfx950 code, and here nothing can (every existing kernel's disassembly is the parent's).
// The entry point and its checks are in scg_kernels.hip.
#include "scg_device.hpp"
#include "../../include/scg_abi.h"

using namespace scg;
typedef float f4v __attribute__((ext_vector_type(4)));

#include "scg_eval.hpp"
#include "scg_rollout_kernel.hpp"

template <bool REC, typename Args>
hipError_t launch_rollout(const Args &A, int grid, hipStream_t s) {
    hipLaunchKernelGGL((rollout_kernel<REC, Args>), dim3(grid), dim3(RO_THREADS), 0, s, A);
    return hipGetLastError();
}
#define SCG_POP_VARIANT(I, B) template hipError_t launch_rollout<true, RolloutPop<I, B>>(const RolloutPop<I, B> &, int, hipStream_t);
SCG_POP_VARIANT(false, false) SCG_POP_VARIANT(true, false) SCG_POP_VARIANT(false, true) SCG_POP_VARIANT(true, true)
#undef SCG_POP_VARIANT
// SPEC §25.1: the one kernel with a gate table
template hipError_t launch_rollout<true, RolloutPopGateArgs>(const RolloutPopGateArgs &, int, hipStream_t);
