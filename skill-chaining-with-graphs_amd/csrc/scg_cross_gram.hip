// scg_cross_gram.hip — cross_gram_kernel (SPEC §17.1, scg_cross_gram_kernel.hpp) and its launch, compiled apart from every other kernel
// for the reason scg_gram.hip gives: what shares a module with the hot kernels changes their gfx950 code. It takes
// gram_kernel's operand helpers (gram_places, gram_phi) from scg_gram_kernel.hpp, so phi is the same expression in both; gram_kernel
// itself is a template that nothing here instantiates. The C-ABI entry point scg_feature_cross_gram and its checks are in scg_kernels.hip.
#include "scg_device.hpp"
#include "../../include/scg_abi.h"

using namespace scg;
typedef float f4v __attribute__((ext_vector_type(4)));

#include "scg_eval.hpp"
#define SCG_GRAM_DEFINE_KERNEL
#include "scg_gram_kernel.hpp"
#define SCG_CROSS_GRAM_DEFINE_KERNEL
#include "scg_cross_gram_kernel.hpp"

hipError_t launch_feature_cross_gram(const CrossGramArgs &G, int n_active, hipStream_t s) {
    hipLaunchKernelGGL(cross_gram_kernel, dim3(CGRAM_MACROS, n_active), dim3(CGRAM_THREADS), 0, s, G);
    return hipGetLastError();
}
