// trilinear64.hpp -- the fp64 trilinear (bilinear in 2-D) sample of a step flow and the classification of a point
// against the grid: the statement of the rule that flowconsist.hip, advect.hip and lic.hip follow and that two
// independent numpy restatements pin bit for bit (tests/flow_consistency_ref.py, tests/advect_ref.py).  lic.hip and
// streamline.hip include this header.  flowconsist.hip, where the rule was first written, and advect.hip keep their own copies of the
// same lines, because kernels of theirs measured slower on the header than the parent's spread allows
// (profiles/trilinear64.txt): a change to the rule is made here AND in those two files.  A later step-flow tool starts
// from here.
//
// A grid has S = (W, H, D) nodes per axis (D = 1 in 2-D); a point has C components (x, y[, z]).  fp64, contraction off:
//   classify(p): a non-finite p_c -> non-finite; else p_c < 0 or p_c > S_c - 1 -> outside (border inclusive); else alive
//   sample(q): a non-finite q_c -> every value NaN, no index formed (the caller's guard: finite_point); else
//     q_c = min(max(q_c, 0), S_c - 1) (clamp_to_grid; a caller that has proved the point inside skips it), then
//     i0 = floor(q_c), f = q_c - i0, g = 1 - f, i1 = min(i0 + 1, S_c - 1); corner (bz, by, bx) weighs (tz ty) tx, t = f
//     where the bit is set, else g; the sum over corners in ascending 4 bz + 2 by + bx of w * value, from 0.0, ALL
//     products formed (a non-finite corner of weight 0 gives NaN: it lies inside the support's closure)
// What a corner contributes (which planes, which element type) is the caller's: corners64 hands it the weight and the
// element offset of each corner in that order, and the caller's own contraction pragma covers its lambda.
#pragma once
#include "common.hpp"

namespace fs {

struct Extent {
  int W, H, D;
};

template <int C>
__device__ __forceinline__ bool finite_point(const double (&p)[3]) {
  bool fin = true;
#pragma unroll
  for (int c = 0; c < C; ++c) fin = fin && isfinite(p[c]);
  return fin;
}

template <int C>
__device__ __forceinline__ bool outside(const double (&p)[3], const Extent& e) {
  const int S[3] = {e.W, e.H, e.D};
  bool out = false;
#pragma unroll
  for (int c = 0; c < C; ++c) out = out || p[c] < 0.0 || p[c] > (double)(S[c] - 1);
  return out;
}

template <int C>
__device__ __forceinline__ void clamp_to_grid(double (&q)[3], const Extent& e) {
  const int S[3] = {e.W, e.H, e.D};
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const double hi = (double)(S[c] - 1);
    const double qc = q[c] < 0.0 ? 0.0 : q[c];
    q[c] = qc > hi ? hi : qc;
  }
}

// f(wt, o) for the 2^C corners of q in ascending 4 bz + 2 by + bx: wt the corner's weight, o its element offset in a
// plane.  q is finite and 0 <= q_c <= S_c - 1, so every offset lies inside the plane.
template <int C, class F>
__device__ __forceinline__ void corners64(const double (&q)[3], const Extent& e, F&& f) {
#pragma clang fp contract(off)
  const int S[3] = {e.W, e.H, e.D};
  const size_t st[3] = {(size_t)1, (size_t)e.W, (size_t)e.W * (size_t)e.H};
  double fr[3], gr[3];
  size_t o0[3], o1[3];
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const double fl = floor(q[c]);
    const int i0 = (int)fl;
    const int i1 = i0 + 1 < S[c] ? i0 + 1 : S[c] - 1;
    fr[c] = q[c] - fl;
    gr[c] = 1.0 - fr[c];
    o0[c] = (size_t)i0 * st[c];
    o1[c] = (size_t)i1 * st[c];
  }
#pragma unroll
  for (int k = 0; k < (1 << C); ++k) {
    const int bx = k & 1, by = (k >> 1) & 1, bz = (k >> 2) & 1;
    double wt;
    size_t o;
    if (C == 3) {
      wt = ((bz ? fr[2] : gr[2]) * (by ? fr[1] : gr[1])) * (bx ? fr[0] : gr[0]);
      o = (bz ? o1[2] : o0[2]) + (by ? o1[1] : o0[1]) + (bx ? o1[0] : o0[0]);
    } else {
      wt = (by ? fr[1] : gr[1]) * (bx ? fr[0] : gr[0]);
      o = (by ? o1[1] : o0[1]) + (bx ? o1[0] : o0[0]);
    }
    f(wt, o);
  }
}

}  // namespace fs
