// scg_gram.hip — gram_kernel (SPEC §16.1, scg_gram_kernel.hpp) and its launch, compiled apart from the step, rollout and reduce kernels
// for the reason scg_rollout_variants.hip gives: what shares a module with those changes their gfx950 code. The C-ABI
// entry point scg_feature_gram and its checks are in scg_kernels.hip.
#include "scg_device.hpp"
#include "../../include/scg_abi.h"

using namespace scg;
typedef float f4v __attribute__((ext_vector_type(4)));

#include "scg_eval.hpp"
#define SCG_GRAM_DEFINE_KERNEL
#include "scg_gram_kernel.hpp"

hipError_t launch_feature_gram(const GramArgs &G, int n_active, hipStream_t s) {
    if (G.yv) hipLaunchKernelGGL(gram_kernel<true>, dim3(GRAM_MACROS, n_active), dim3(GRAM_THREADS), 0, s, G);
    else hipLaunchKernelGGL(gram_kernel<false>, dim3(GRAM_MACROS, n_active), dim3(GRAM_THREADS), 0, s, G);
    return hipGetLastError();
}
