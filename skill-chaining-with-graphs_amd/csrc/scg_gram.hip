// scg_gram.hip — gram_kernel (SPEC §16.1, §17.1; scg_gram_kernel.hpp) in its three instantiations and their two launches, compiled apart
// from the step, rollout and reduce kernels for the reason scg_rollout_variants.hip gives: what shares a module with those changes
// their gfx950 code. The three do not change one another's (§3.21). The C-ABI entry points scg_feature_gram and
// scg_feature_cross_gram and their checks are in scg_kernels.hip.
#include "scg_device.hpp"
#include "../../include/scg_abi.h"

using namespace scg;
typedef float f4v __attribute__((ext_vector_type(4)));

#include "scg_eval.hpp"
#include "scg_gram_kernel.hpp"

template <class S, bool RHS>
static hipError_t launch_gram(const GramArgs &G, int n_active, hipStream_t s) {
    hipLaunchKernelGGL((gram_kernel<S, RHS>), dim3(S::MACROS, n_active), dim3(S::THREADS), 0, s, G);
    return hipGetLastError();
}
hipError_t launch_feature_gram(const GramArgs &G, int n_active, hipStream_t s) {
    return G.yv ? launch_gram<GramSym, true>(G, n_active, s) : launch_gram<GramSym, false>(G, n_active, s);
}
hipError_t launch_feature_cross_gram(const GramArgs &G, int n_active, hipStream_t s) {
    return launch_gram<GramCross, false>(G, n_active, s);
}
