// scg_gram.hip — gram_kernel (SPEC §16.1, §17.1, §20.1, §22.1; scg_gram_kernel.hpp) in its seven instantiations and their five launches,
// compiled apart from the step, rollout and reduce kernels for the reason scg_rollout_variants.hip gives: what shares a module with
// those changes their gfx950 code. The seven do not change one another's (§3.21, §3.25, §3.27, §3.28). The C-ABI entry points
// scg_feature_gram, scg_feature_gram_targets, scg_feature_gram_weighted and scg_feature_cross_gram (and scg_basis_gram_irls, whose
// order-5 launch is here) and their checks are in scg_kernels.hip.
#include "scg_device.hpp"
#include "../../include/scg_abi.h"

using namespace scg;
typedef float f4v __attribute__((ext_vector_type(4)));

#include "scg_eval.hpp"
#include "scg_gram_kernel.hpp"

template <class S, int RHS, bool WEIGHTED = false, bool IRLS = false>
static hipError_t launch_gram(const GramArgs &G, int n_active, hipStream_t s) {
    hipLaunchKernelGGL((gram_kernel<S, RHS, WEIGHTED, IRLS>), dim3(S::MACROS, n_active), dim3(S::THREADS), 0, s, G);
    return hipGetLastError();
}
hipError_t launch_feature_gram(const GramArgs &G, int n_active, hipStream_t s) {
    return G.yv ? launch_gram<GramSym, GRAM_RHS_ONE>(G, n_active, s) : launch_gram<GramSym, GRAM_RHS_NONE>(G, n_active, s);
}
hipError_t launch_feature_gram_targets(const GramArgs &G, int n_active, hipStream_t s) {
    return launch_gram<GramSym, GRAM_RHS_TARGETS>(G, n_active, s);
}
// SPEC §22.1: the two weighted shapes, A alone (n_tgt = 0) or with the targets' B
hipError_t launch_feature_gram_weighted(const GramArgs &G, int n_active, hipStream_t s) {
    return G.n_tgt ? launch_gram<GramSym, GRAM_RHS_TARGETS, true>(G, n_active, s) : launch_gram<GramSym, GRAM_RHS_NONE, true>(G, n_active, s);
}
// SPEC §23.2 at order 5: the weighted A as H, the unweighted b for yv = e as grad
hipError_t launch_feature_gram_irls(const GramArgs &G, int n_active, hipStream_t s) {
    return launch_gram<GramSym, GRAM_RHS_ONE, true, true>(G, n_active, s);
}
hipError_t launch_feature_cross_gram(const GramArgs &G, int n_active, hipStream_t s) {
    return launch_gram<GramCross, GRAM_RHS_NONE>(G, n_active, s);
}
