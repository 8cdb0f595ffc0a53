// scg_step_gate.hip — SPEC §26: step_gate_kernel (scg_step_gate_kernel.hpp), the gate table of scg_step_gated, and its launch.
//
// A unit of its own for the reason scg_rollout_population.hip gives: what shares a module with a kernel may change that kernel's
// gfx950 code, and here nothing can (every existing kernel's disassembly is the parent's). The entry point and its
// checks are in scg_kernels.hip. The step kernel's header comes in for the result line's layout (OREC, OREC_DECLINED) and the
// wave-phase header for store_z1 and list_append; neither kernel template is instantiated here.
#include "scg_device.hpp"
#include "../../include/scg_abi.h"

using namespace scg;
typedef float f4v __attribute__((ext_vector_type(4)));

#include "scg_eval.hpp"
#include "scg_step_kernel.hpp"
#include "scg_wave_phases.hpp"
#include "scg_step_gate_kernel.hpp"

template <int ENVS>
static hipError_t launch_envs(const StepGateArgs &A, hipStream_t s) {
    hipLaunchKernelGGL((step_gate_kernel<SG_WAVES, ENVS>), dim3((A.n + ENVS - 1) / ENVS), dim3(SG_WAVES * 64), 0, s, A);
    return hipGetLastError();
}
hipError_t launch_step_gate(const StepGateArgs &A, int envs, hipStream_t s) {
    return envs == 64 ? launch_envs<64>(A, s) : envs == 128 ? launch_envs<128>(A, s) : launch_envs<256>(A, s);
}
