// streamline.hip -- streamlines of K steady fields as geometry (fs_streamlines2d / fs_streamlines3d): each of S lines starts
// at its seed and follows the NORMALISED field of one step flow, with it or against it, for up to M steps of arc length
// h; every vertex is kept.  What the separatrices of a vector-field topology are drawn with (skeleton.py).
//
// Per line s (fp64 on the widened fp32 values, contraction off, correctly rounded sqrt and division, positions fp64 for
// the whole line: a numpy fp64 restatement with the same operations in the same order reproduces every output bit --
// tests/streamline_ref.py; include/flowsci_hip.h "Streamlines" states the rule):
//   sample / classify: trilinear64.hpp's (a non-finite q samples NaN, another is clamped)
//   dir(k, q): lic.hip's: v = sample(k, q); a non-finite v_c -> NONFINITE; n = sqrt((v0 v0 + v1 v1) + v2 v2);
//     !(n > vmin) -> STAGNANT; d_c = v_c / n
//   slot 0 = (float)seed, hit = -1, length = 0, left = (home == NULL or home[s] < 0); k = step[s] outside 0..K-1 ends the
//   line INVALID, classify(seed) not ALIVE ends it OUT / NONFINITE (neither samples); hs = +-h, hh = +-0.5 h, h6 = +-h / 6
//   (formed on the host, negated here where sign[s] < 0); p = seed; for i = 1..M:
//     d1 = dir(p); Euler p' = p + hs d1; RK2 d = dir(p + hh d1), p' = p + hs d; RK4 d2 = dir(p + hh d1),
//     d3 = dir(p + hh d2), d4 = dir(p + hs d3), p' = p + h6 (((d1 + 2 d2) + 2 d3) + d4); a code at any stage ends the line
//     classify(p') not ALIVE ends the line OUT (the exit point is not stored); else p = p', slot i = (float)p, length = i
//     cell_a = min((int)floor(p_a), S_a - 2), c = (cz H + cy) W + cx; c != home[s] sets left; capture != NULL and left and
//     capture[k][c] != 0 ends the line CAPTURED with hit = c
//   M steps done: FULL.  Slots beyond length are not written.
//
// One launch, one lane per line, sampling through trilinear64.hpp straight from the C planes: a skeleton has a few
// thousand lines, and lic.hip's packed image is a pre-pass over the whole field of every step, which costs more than
// they do.  A lane whose line has ended idles until its wave is done, so a workgroup is ONE wave (64 lanes): a wave's
// registers and slot are free as soon as its own longest line ends, not when the longest of 256 does, and 4096 lines
// spread over 64 CUs instead of 16.  The loop is a chain of dependent fp64 gathers (each stage's point comes from the one
// before), so the latency is hidden by other waves only: nothing is staged in LDS, nothing goes through scratch (every
// array below is indexed by unrolled constants), and the 55 (2-D Euler) to 106 (3-D RK4) registers leave room for 8 to 4
// waves per SIMD (tests/test_streamline_build.py prints the counts).  Stores of a slot
// are coalesced across the lines of a wave (slot-major layout).  Every index is formed from a finite value clamped to the
// grid, `step` is checked before it selects a field, and a slot index never exceeds M: no input makes the kernel read or
// write outside its operands.
#include "common.hpp"
#include "trilinear64.hpp"

#include <climits>

namespace {

constexpr int NT = 64;

struct SLP {
  long long fss, css;   // step strides of flows and capture
  long long plane;      // D*H*W
  long long scs;        // component stride of seeds
  long long vss, vcs;   // slot and component strides of verts
  long long S;
  int K, D, H, W, M;
  double h, hh, h6, vmin;  // step length, 0.5 h, h / 6.0 (formed on the host)
};

// d = sample(k, q) / |sample(k, q)|, or the code that ends the line.  Every index comes from a finite value clamped to
// [0, S_c - 1].
template <int C>
__device__ __forceinline__ int dir(const float* __restrict__ fk, const SLP& a, const double (&q)[3], double (&d)[3]) {
#pragma clang fp contract(off)
  if (!fs::finite_point<C>(q)) return FS_SL_NONFINITE;  // (sample gives NaN)
  const fs::Extent e{a.W, a.H, a.D};
  double qc[3] = {0.0, 0.0, 0.0}, v[3] = {0.0, 0.0, 0.0};
#pragma unroll
  for (int c = 0; c < C; ++c) qc[c] = q[c];
  fs::clamp_to_grid<C>(qc, e);
  const size_t plane = (size_t)a.plane;
  fs::corners64<C>(qc, e, [&](double wt, size_t o) {
#pragma unroll
    for (int c = 0; c < C; ++c) v[c] = v[c] + wt * (double)fk[(size_t)c * plane + o];
  });
  bool fin = true;
#pragma unroll
  for (int c = 0; c < C; ++c) fin = fin && isfinite(v[c]);
  if (!fin) return FS_SL_NONFINITE;
  double n2 = v[0] * v[0] + v[1] * v[1];
  if (C == 3) n2 = n2 + v[2] * v[2];
  const double n = sqrt(n2);
  if (!(n > a.vmin)) return FS_SL_STAGNANT;
#pragma unroll
  for (int c = 0; c < C; ++c) d[c] = v[c] / n;
  return FS_SL_FULL;
}

template <int C, int METHOD>
__global__ __launch_bounds__(NT) void streamline_kernel(const float* __restrict__ flows, const double* __restrict__ seeds,
                                                        const int* __restrict__ step,
                                                        const signed char* __restrict__ sign,
                                                        const int* __restrict__ home,
                                                        const unsigned char* __restrict__ capture,
                                                        float* __restrict__ verts, int* __restrict__ length,
                                                        unsigned char* __restrict__ end, int* __restrict__ hit, SLP a) {
#pragma clang fp contract(off)
  const long long s = (long long)blockIdx.x * NT + threadIdx.x;
  if (s >= a.S) return;
  double p[3] = {0.0, 0.0, 0.0};
#pragma unroll
  for (int c = 0; c < C; ++c) {
    p[c] = seeds[(size_t)c * a.scs + s];
    verts[(size_t)c * a.vcs + s] = (float)p[c];
  }
  const int k = step[s];
  const int hm = home ? home[s] : -1;
  const fs::Extent e{a.W, a.H, a.D};
  int code = FS_SL_FULL, len = 0, captured = -1;
  if (k < 0 || k >= a.K) code = FS_SL_INVALID;
  else if (!fs::finite_point<C>(p)) code = FS_SL_NONFINITE;
  else if (fs::outside<C>(p, e)) code = FS_SL_OUT;
  if (code == FS_SL_FULL) {
    const bool back = sign[s] < 0;
    const double hs = back ? -a.h : a.h, hh = back ? -a.hh : a.hh, h6 = back ? -a.h6 : a.h6;
    const float* fk = flows + (size_t)k * a.fss;
    const unsigned char* ck = capture ? capture + (size_t)k * a.css : nullptr;
    bool left = hm < 0;
    for (int i = 1; i <= a.M; ++i) {
      double d1[3] = {0.0, 0.0, 0.0}, q[3] = {0.0, 0.0, 0.0};
      code = dir<C>(fk, a, p, d1);
      if (code != FS_SL_FULL) break;
      if (METHOD == FS_ADV_EULER) {
#pragma unroll
        for (int c = 0; c < C; ++c) q[c] = p[c] + hs * d1[c];
      } else if (METHOD == FS_ADV_RK2) {
        double d[3] = {0.0, 0.0, 0.0};
#pragma unroll
        for (int c = 0; c < C; ++c) q[c] = p[c] + hh * d1[c];
        code = dir<C>(fk, a, q, d);
        if (code != FS_SL_FULL) break;
#pragma unroll
        for (int c = 0; c < C; ++c) q[c] = p[c] + hs * d[c];
      } else {
        double d2[3] = {0.0, 0.0, 0.0}, d3[3] = {0.0, 0.0, 0.0}, d4[3] = {0.0, 0.0, 0.0};
#pragma unroll
        for (int c = 0; c < C; ++c) q[c] = p[c] + hh * d1[c];
        code = dir<C>(fk, a, q, d2);
        if (code != FS_SL_FULL) break;
#pragma unroll
        for (int c = 0; c < C; ++c) q[c] = p[c] + hh * d2[c];
        code = dir<C>(fk, a, q, d3);
        if (code != FS_SL_FULL) break;
#pragma unroll
        for (int c = 0; c < C; ++c) q[c] = p[c] + hs * d3[c];
        code = dir<C>(fk, a, q, d4);
        if (code != FS_SL_FULL) break;
#pragma unroll
        for (int c = 0; c < C; ++c) q[c] = p[c] + h6 * (((d1[c] + 2.0 * d2[c]) + 2.0 * d3[c]) + d4[c]);
      }
      if (!fs::finite_point<C>(q) || fs::outside<C>(q, e)) {
        code = FS_SL_OUT;
        break;
      }
      const size_t slot = (size_t)i * a.vss + s;
#pragma unroll
      for (int c = 0; c < C; ++c) {
        p[c] = q[c];
        verts[slot + (size_t)c * a.vcs] = (float)p[c];
      }
      len = i;
      // p is on the grid: 0 <= floor(p_a) <= S_a - 1, and every extent is >= 2
      const int ext[3] = {a.W, a.H, a.D};
      int cell[3] = {0, 0, 0};
#pragma unroll
      for (int c = 0; c < C; ++c) {
        const int f = (int)floor(p[c]);
        cell[c] = f < ext[c] - 2 ? f : ext[c] - 2;
      }
      const int ci = (cell[2] * a.H + cell[1]) * a.W + cell[0];
      if (ci != hm) left = true;
      if (ck && left && ck[ci] != 0) {
        code = FS_SL_CAPTURED;
        captured = ci;
        break;
      }
    }
  }
  length[s] = len;
  end[s] = (unsigned char)code;
  hit[s] = captured;
}

int launch(bool is3d, const float* flows, int K, int C, int D, int H, int W, long long fss, const double* seeds,
           long long scs, long long S, const int* step, const signed char* sign, const int* home,
           const unsigned char* capture, long long css, int M, double h, double vmin, int method, float* verts,
           long long vss, long long vcs, int* length, unsigned char* end, int* hit, fs_stream_t stream) {
  FS_ENTER();
  FS_REQUIRE_PTR(flows); FS_REQUIRE_PTR(seeds); FS_REQUIRE_PTR(step); FS_REQUIRE_PTR(sign);
  FS_REQUIRE_PTR(verts); FS_REQUIRE_PTR(length); FS_REQUIRE_PTR(end); FS_REQUIRE_PTR(hit);
  if (K < 1 || S < 1 || C != (is3d ? 3 : 2) || (is3d && D < 2) || H < 2 || W < 2) return FS_ERR_SHAPE;
  const long long plane = (long long)D * H * W;
  if (plane > INT_MAX) return FS_ERR_SHAPE;  // a cell index is an int32
  if (K > 1 && fss < C * plane) return FS_ERR_SHAPE;
  if (capture && K > 1 && css < plane) return FS_ERR_SHAPE;
  if (scs < S || vcs < S || vss < C * vcs) return FS_ERR_SHAPE;
  const long long blocks = (S + NT - 1) / NT;
  if (blocks > 0x7fffffffLL) return FS_ERR_SHAPE;
  if (M < 1) return FS_ERR_ARG;
  if (!(h > 0.0 && h < HUGE_VAL) || !(vmin >= 0.0 && vmin < HUGE_VAL)) return FS_ERR_ARG;
  if (method != FS_ADV_EULER && method != FS_ADV_RK2 && method != FS_ADV_RK4) return FS_ERR_ARG;
  SLP a;
  a.fss = fss; a.css = css; a.plane = plane; a.scs = scs; a.vss = vss; a.vcs = vcs; a.S = S;
  a.K = K; a.D = D; a.H = H; a.W = W; a.M = M;
  a.h = h; a.hh = 0.5 * h; a.h6 = h / 6.0; a.vmin = vmin;
  const hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)blocks), blk(NT);
#define FS_SL_LAUNCH(CC)                                                                                             \
  do {                                                                                                               \
    if (method == FS_ADV_EULER)                                                                                      \
      hipLaunchKernelGGL((streamline_kernel<CC, FS_ADV_EULER>), grid, blk, 0, st, flows, seeds, step, sign, home,    \
                         capture, verts, length, end, hit, a);                                                       \
    else if (method == FS_ADV_RK2)                                                                                   \
      hipLaunchKernelGGL((streamline_kernel<CC, FS_ADV_RK2>), grid, blk, 0, st, flows, seeds, step, sign, home,      \
                         capture, verts, length, end, hit, a);                                                       \
    else                                                                                                             \
      hipLaunchKernelGGL((streamline_kernel<CC, FS_ADV_RK4>), grid, blk, 0, st, flows, seeds, step, sign, home,      \
                         capture, verts, length, end, hit, a);                                                       \
  } while (0)
  if (is3d) FS_SL_LAUNCH(3);
  else FS_SL_LAUNCH(2);
#undef FS_SL_LAUNCH
  FS_LAUNCH_CHECK();
  return FS_OK;
}

}  // namespace

extern "C" int fs_streamlines2d(const float* flows, int K, int C, int H, int W, long long flow_sstride,
                                const double* seeds, long long seed_cstride, long long S, const int* step,
                                const signed char* sign, const int* home, const unsigned char* capture,
                                long long capture_sstride, int M, double h, double vmin, int method, float* verts,
                                long long vert_sstride, long long vert_cstride, int* length, unsigned char* end, int* hit,
                                fs_stream_t stream) {
  return launch(false, flows, K, C, 1, H, W, flow_sstride, seeds, seed_cstride, S, step, sign, home, capture,
                capture_sstride, M, h, vmin, method, verts, vert_sstride, vert_cstride, length, end, hit, stream);
}

extern "C" int fs_streamlines3d(const float* flows, int K, int C, int D, int H, int W, long long flow_sstride,
                                const double* seeds, long long seed_cstride, long long S, const int* step,
                                const signed char* sign, const int* home, const unsigned char* capture,
                                long long capture_sstride, int M, double h, double vmin, int method, float* verts,
                                long long vert_sstride, long long vert_cstride, int* length, unsigned char* end, int* hit,
                                fs_stream_t stream) {
  return launch(true, flows, K, C, D, H, W, flow_sstride, seeds, seed_cstride, S, step, sign, home, capture,
                capture_sstride, M, h, vmin, method, verts, vert_sstride, vert_cstride, length, end, hit, stream);
}
