// scg_basis.hip — SPEC §18, the basis-order probe: gram_kernel (scg_gram_kernel.hpp) in its symmetric shape at the orders 3 and 7,
// with and without b and in §23.2's IRLS mode, and the small kernels of the probe, basis_features_kernel (phi of order p,
// materialised), basis_values_kernel (§18.3's pinned sum of up to 8 weight rows against phi) and §23.1's logistic_terms_kernel. A translation unit of its own for the reason
// scg_gram.hip gives: the order-5 kernels of scg_gram.hip and scg_kernels.hip keep their code, and at order 5
// scg_basis_gram and scg_basis_features dispatch to them (scg_kernels.hip, where the C-ABI entry points and their checks are).
#include "scg_device.hpp"
#include "../../include/scg_abi.h"

using namespace scg;
typedef float f4v __attribute__((ext_vector_type(4)));

#include "scg_eval.hpp"
#include "scg_gram_kernel.hpp"
#include "scg_basis_kernels.hpp"

template <class S>
static hipError_t launch_gram_order(const GramArgs &G, int n_active, hipStream_t s) {
    if (G.yv) hipLaunchKernelGGL((gram_kernel<S, GRAM_RHS_ONE>), dim3(S::MACROS, n_active), dim3(S::THREADS), 0, s, G);
    else hipLaunchKernelGGL((gram_kernel<S, GRAM_RHS_NONE>), dim3(S::MACROS, n_active), dim3(S::THREADS), 0, s, G);
    return hipGetLastError();
}
hipError_t launch_basis_gram_3(const GramArgs &G, int n_active, hipStream_t s) { return launch_gram_order<GramBasis<3>>(G, n_active, s); }
hipError_t launch_basis_gram_7(const GramArgs &G, int n_active, hipStream_t s) { return launch_gram_order<GramBasis<7>>(G, n_active, s); }

// SPEC §23.2 at the orders 3 and 7 (order 5: launch_feature_gram_irls of scg_gram.hip)
template <class S>
static hipError_t launch_gram_irls_order(const GramArgs &G, int n_active, hipStream_t s) {
    hipLaunchKernelGGL((gram_kernel<S, GRAM_RHS_ONE, true, true>), dim3(S::MACROS, n_active), dim3(S::THREADS), 0, s, G);
    return hipGetLastError();
}
hipError_t launch_basis_gram_irls_3(const GramArgs &G, int n_active, hipStream_t s) { return launch_gram_irls_order<GramBasis<3>>(G, n_active, s); }
hipError_t launch_basis_gram_irls_7(const GramArgs &G, int n_active, hipStream_t s) { return launch_gram_irls_order<GramBasis<7>>(G, n_active, s); }

// SPEC §23.1
hipError_t launch_logistic_terms(int64_t n, const float *z, const uint8_t *label, float *p, float *rw, float *e, hipStream_t s) {
    const int64_t blocks = (n + LOGISTIC_THREADS - 1) / LOGISTIC_THREADS;
    hipLaunchKernelGGL((logistic_terms_kernel<LOGISTIC_THREADS>), dim3((int)(blocks < 4096 ? blocks : 4096)), dim3(LOGISTIC_THREADS), 0, s, n, z, label, p, rw, e);
    return hipGetLastError();
}

template <int ORDER>
static hipError_t launch_features_order(int64_t n, const float *const *st, float *phi, hipStream_t s) {
    const int grid = (int)(n < 8192 ? n : 8192);
    hipLaunchKernelGGL((basis_features_kernel<GramOrder<ORDER>>), dim3(grid), dim3(64), 0, s, n, st[0], st[1], st[2], st[3], phi);
    return hipGetLastError();
}
hipError_t launch_basis_features(int order, int64_t n, const float *const *st, float *phi, hipStream_t s) {
    return order == 3 ? launch_features_order<3>(n, st, phi, s) : launch_features_order<7>(n, st, phi, s);
}

template <int ORDER>
static hipError_t launch_values_order(int64_t n, const float *const *st, const float *V, int m, float *out, hipStream_t s) {
    const int64_t groups = (n + BASIS_VALUES_SAMPLES - 1) / BASIS_VALUES_SAMPLES;
    const int grid = (int)(groups < 16384 ? groups : 16384);
    hipLaunchKernelGGL((basis_values_kernel<GramOrder<ORDER>>), dim3(grid), dim3(64), 0, s, n, st[0], st[1], st[2], st[3], V, m, out);
    return hipGetLastError();
}
hipError_t launch_basis_values(int order, int64_t n, const float *const *st, const float *V, int m, float *out, hipStream_t s) {
    return order == 3 ? launch_values_order<3>(n, st, V, m, out, s)
         : order == 5 ? launch_values_order<5>(n, st, V, m, out, s) : launch_values_order<7>(n, st, V, m, out, s);
}

// SPEC §24.2
hipError_t launch_classifier_logits(int n, const float *x, const float *y, const float *w8, float *z, hipStream_t s) {
    hipLaunchKernelGGL((classifier_logits_kernel<LOGISTIC_THREADS>), dim3((n + LOGISTIC_THREADS - 1) / LOGISTIC_THREADS), dim3(LOGISTIC_THREADS), 0, s, n, x, y, w8, z);
    return hipGetLastError();
}
