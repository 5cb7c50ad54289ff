// The census pair gradient shared by the 2-D (losses.hip) and 3-D (census3d.hip) backward kernels.
#pragma once
#include <hip/hip_runtime.h>

// A pixel pair (q, n = q + delta) enters the distance twice: in the term with centre q and neighbour n (u = g[n] - g[q],
// weight k[q]) and in the term with centre n and neighbour q (u' = -u, weight k[n]).  T(u) = u / sqrt(0.81 + u^2) is odd,
// D(e) = e^2 / (0.1 + e^2) even, so both terms share every transcendental: with e = T(u1) - T(u2),
//   d dist / d g1[q] = -(k[q] + k[n]) D'(e) T'(u1),   d dist / d g2[q] = +(k[q] + k[n]) D'(e) T'(u2),
//   D'(e) = 0.2 e / (0.1 + e^2)^2,  T'(u) = 0.81 / (0.81 + u^2)^1.5
// -- 49 evaluations per pixel (2 v_rsq + 1 v_rcp each) instead of the 98 of rounds 1-3 (PMC then: 3 400 VALU
// instructions per pixel, a vector instruction issuing in 70 % of the CU-busy cycles).
// Two bitwise equal images must give a distance and gradients of exactly 0, so T(u1) - T(u2) may not depend on which
// multiplications the compiler chooses to contract:
// r = 1 / sqrt(0.81 + u^2) takes its argument from one explicit fma (left to contraction, the unrolled 3-D forward fused
// it for some taps of one volume and not for the same taps of the other), and
// e = T(u1) - T(u2) = u1 r1 - u2 r2 rounds both products before the subtraction (contracted into fma(u1, r1, -(u2 r2)) it
// is the rounding error of one product where u1 == u2).
__device__ __forceinline__ float census_rnorm(float u) { return rsqrtf(__builtin_fmaf(u, u, 0.81f)); }

__device__ __forceinline__ float census_ternary_diff(float u1, float r1, float u2, float r2) {
#pragma clang fp contract(off)
  return u1 * r1 - u2 * r2;
}

__device__ __forceinline__ void census_pair_grad(float u1, float u2, float ksum, float& a1, float& a2) {
  const float r1 = census_rnorm(u1), r2 = census_rnorm(u2);
  const float e = census_ternary_diff(u1, r1, u2, r2);
  const float den = 0.1f + e * e;
  const float dD = ksum * (0.2f * 0.81f) * e * __builtin_amdgcn_rcpf(den * den);  // v_rcp: the kernel is VALU-bound
  a1 -= dD * (r1 * r1 * r1);
  a2 += dD * (r2 * r2 * r2);
}
