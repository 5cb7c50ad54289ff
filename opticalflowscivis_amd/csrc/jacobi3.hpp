// One Jacobi rotation of a symmetric 3 x 3 matrix, shared by the eigenvalue solvers of ftle.hip (largest eigenvalue of a
// positive semi-definite tensor) and velgrad.hip (all three of an indefinite one).
#pragma once
#include "common.hpp"

namespace fs {

// One Jacobi rotation in the (p, q) plane of a symmetric 3 x 3 matrix whose entries are at most 1 in magnitude; r is
// the third index.  The angle is computed in fp32 (any angle keeps the eigenvalues as long as the rotation is
// orthogonal; an angle good to 1e-7 leaves 1e-7 of a_pq behind, which the next sweep removes), c = 1 / sqrt(1 + t^2)
// in fp64 from the fp32 estimate by two Newton steps, so c^2 + s^2 = 1 to fp64 rounding.  No fp64 division or sqrt;
// |t| may exceed 1 by the estimate's rounding, which nothing below relies on.  Nothing here asks for a definite matrix.
__device__ __forceinline__ void jacobi_rotate(double& app, double& aqq, double& apq, double& arp, double& arq) {
  if (!(fabs(apq) > 0x1p-60)) return;  // nothing to remove (and o * o below stays a normal fp32 number)
  // the hardware's one-instruction sqrt / rcp / rsq (1 ulp, normal operands here): the angle needs no more
  const float o = (float)apq, d = (float)(aqq - app);
  const float h = __builtin_amdgcn_sqrtf(d * d + 4.f * (o * o));  // >= 2 |o| > 0
  const float t32 = (2.f * o) * __builtin_amdgcn_rcpf(d + copysignf(h, d));  // the smaller root of t^2 + t d / o - 1 = 0
  const double t = (double)t32;
  const double x = 1.0 + t * t;
  double c = (double)__builtin_amdgcn_rsqf((float)x);
  c = c * (1.5 - (0.5 * x) * (c * c));
  c = c * (1.5 - (0.5 * x) * (c * c));
  const double s = t * c;
  const double cc = c * c, ss = s * s, sc = s * c;
  const double npp = (cc * app - (2.0 * sc) * apq) + ss * aqq;
  const double nqq = (ss * app + (2.0 * sc) * apq) + cc * aqq;
  const double npq = (cc - ss) * apq + sc * (app - aqq);
  const double nrp = c * arp - s * arq;
  const double nrq = s * arp + c * arq;
  app = npp; aqq = nqq; apq = npq; arp = nrp; arq = nrq;
}

}  // namespace fs
