// lic.hip -- line integral convolution of K steady fields in one call (fs_lic2d / fs_lic3d): every node's value is a
// texture averaged along the streamline of the NORMALISED field through that node, L steps of length h each way.
//
// Per node (fp64, contraction off, correctly rounded sqrt and division, positions fp64 for the whole line: a numpy fp64
// restatement with the same operations in the same order reproduces every output bit, end code and count --
// tests/lic_ref.py; include/flowsci_hip.h "Line integral convolution" states the rule):
//   sample / classify: trilinear64.hpp's, the rule advect.hip restates (a non-finite q samples NaN, another is clamped)
//   dir(k, q): v = sample(k, q); a non-finite v_c -> NONFINITE; n = sqrt((v0 v0 + v1 v1) + v2 v2); !(n > vmin) ->
//     STAGNANT; d_c = v_c / n
//   tsample(k, q): sample's clamp, corners and weights on the step's one texture plane
//   one side (s = +1, then -1; hs = s h, hh = 0.5 hs): p = node, A = Wt = 0, n = 0, end = FULL; for i = 1..L:
//     d = dir(p) [RK2: d = dir(p + hh d)], a code ends the side; p' = p + hs d; classify(p') not ALIVE ends the side
//     with OUT (the exit point is not sampled); else p = p', A += w[i] tsample(p), Wt += w[i], n += 1
//   out = (float)(((w[0] tsample(node) + A+) + A-) / ((w[0] + Wt+) + Wt-)), ends = end+ | end- << 2, count = 1 + n+ + n-
//
// Two launches.  A streaming pre-pass packs (v_x, v_y[, v_z], tex[, 0]) of every node and step into one 16-byte
// element of the caller's workspace; the line kernel then pays ONE 16-byte load per corner instead of C + 1 dword loads
// (the period of the plane form was set by the number of gather instructions: profiles/lic.txt, 1.7 - 2.9 x in 3-D with
// the pre-pass included).  One thread per node walks both sides.  A line point is sampled ONCE for the texture and the
// next step's direction: tsample(p) and sample(p) share p, so one set of clamped indices and corner weights serves the
// C + 1 values (the same products in the same order as two separate samplers).  Nothing goes through global memory
// between the steps.  Lane-to-node mapping: in 3-D a wave owns a compact 4 x 4 x 4 tile (its corner loads share cache
// lines in all three directions), in 2-D 64 consecutive x of a row; the ablation build keeps the other mapping and the
// plane form (FLOWSCI_LIC_VARIANT), and scripts/licbench.py --variants checks that all four give the same bits.  Every
// index is formed from a finite value clamped to the grid: no input makes the kernels read outside their operands, and
// the pre-pass writes exactly the K * D*H*W elements the size query counts.
#include "common.hpp"
#include "trilinear64.hpp"

namespace {

constexpr int NT = 256;

struct LP {
  long long fss, tss;  // step strides of flows and tex (tss = 0: one texture for every step)
  long long plane;     // D*H*W
  long long total;     // threads that own a node or a tile slot
  int K, D, H, W, L;
  int tw, th, td;      // tiles per axis (tile mapping only)
  double h, hh, vmin;  // step length, 0.5 h (formed on the host)
};

// what a line point is sampled from: one 16-byte element (v_x, v_y[, v_z], tex) per node, or (ablation build) the C
// field planes and the texture plane as they are
#ifdef FS_ABLATION
struct PlaneSrc {
  const float* fk;
  const float* tk;
  long long plane;
  template <int C, bool WV, bool WT>
  __device__ __forceinline__ void corner(size_t o, double (&v)[3], double& t) const {
    if (WV) {
#pragma unroll
      for (int c = 0; c < C; ++c) v[c] = (double)fk[(size_t)c * plane + o];
    }
    if (WT) t = (double)tk[o];
  }
};
#endif

struct PackedSrc {
  const float4* img;
  template <int C, bool WV, bool WT>
  __device__ __forceinline__ void corner(size_t o, double (&v)[3], double& t) const {
    const float4 e = img[o];
    v[0] = (double)e.x;
    v[1] = (double)e.y;
    if (C == 3) v[2] = (double)e.z;
    t = (double)(C == 3 ? e.w : e.z);
  }
};

template <int C>
__device__ __forceinline__ bool alive(const double (&p)[3], const LP& a) {
  return fs::finite_point<C>(p) && !fs::outside<C>(p, fs::Extent{a.W, a.H, a.D});
}

// v = the field (WV) and t = the texture (WT) sampled at q.  Every index comes from a finite value clamped to
// [0, S_c - 1].
template <int C, bool WV, bool WT, class Src>
__device__ __forceinline__ void gather(const Src& src, const LP& a, const double (&q)[3], double (&v)[3], double& t) {
#pragma clang fp contract(off)
  if (!fs::finite_point<C>(q)) {
#pragma unroll
    for (int c = 0; c < C; ++c) v[c] = __builtin_nan("");
    t = __builtin_nan("");
    return;
  }
  const fs::Extent e{a.W, a.H, a.D};
  double qc[3] = {0.0, 0.0, 0.0}, s[3] = {0.0, 0.0, 0.0}, ts = 0.0;
#pragma unroll
  for (int c = 0; c < C; ++c) qc[c] = q[c];  // (a 2-D caller's q[2] is not set: it is not read)
  fs::clamp_to_grid<C>(qc, e);
  fs::corners64<C>(qc, e, [&](double wt, size_t o) {
    double cv[3] = {0.0, 0.0, 0.0}, ct = 0.0;
    src.template corner<C, WV, WT>(o, cv, ct);
    if (WV) {
#pragma unroll
      for (int c = 0; c < C; ++c) s[c] = s[c] + wt * cv[c];
    }
    if (WT) ts = ts + wt * ct;
  });
#pragma unroll
  for (int c = 0; c < C; ++c) v[c] = s[c];
  t = ts;
}

// d = v / |v|, or the code that ends the side
template <int C>
__device__ __forceinline__ int direction(const double (&v)[3], double vmin, double (&d)[3]) {
#pragma clang fp contract(off)
  bool fin = true;
#pragma unroll
  for (int c = 0; c < C; ++c) fin = fin && isfinite(v[c]);
  if (!fin) return FS_LIC_NONFINITE;
  double n2 = v[0] * v[0] + v[1] * v[1];
  if (C == 3) n2 = n2 + v[2] * v[2];
  const double n = sqrt(n2);
  if (!(n > vmin)) return FS_LIC_STAGNANT;
#pragma unroll
  for (int c = 0; c < C; ++c) d[c] = v[c] / n;
  return FS_LIC_FULL;
}

// TILE: a wave owns a compact 4 x 4 x 4 (8 x 8) tile instead of 64 consecutive x of a row
template <int C, bool TILE>
__device__ __forceinline__ bool node_of(const LP& a, long long gid, int& k, int& x, int& y, int& z) {
  if (!TILE) {
    k = (int)(gid / a.plane);
    const long long r = gid - (long long)k * a.plane;
    const long long row = r / a.W;
    x = (int)(r - row * a.W);
    y = (int)(row % a.H);
    z = (int)(row / a.H);
    return true;
  }
  const int lane = (int)(gid & 63);
  long long tile = gid >> 6;
  const int tx = (int)(tile % a.tw);
  tile /= a.tw;
  const int ty = (int)(tile % a.th);
  tile /= a.th;
  const int tz = (int)(tile % a.td);
  k = (int)(tile / a.td);
  if (C == 3) {
    x = tx * 4 + (lane & 3);
    y = ty * 4 + ((lane >> 2) & 3);
    z = tz * 4 + (lane >> 4);
  } else {
    x = tx * 8 + (lane & 7);
    y = ty * 8 + (lane >> 3);
    z = 0;
  }
  return x < a.W && y < a.H && z < a.D;
}

template <int C, int M, class Src>
__device__ __forceinline__ void lic_node(const Src& src, const double* __restrict__ w, float* __restrict__ out,
                                         unsigned char* __restrict__ ends, int* __restrict__ count, const LP& a,
                                         int k, int x, int y, int z) {
#pragma clang fp contract(off)
  const double p0[3] = {(double)x, (double)y, (double)z};
  double v0[3], t0;
  gather<C, true, true>(src, a, p0, v0, t0);
  const double w0 = w[0];
  double acc = w0 * t0, wsum = w0;
  int cnt = 1, code = 0;
#pragma unroll 1
  for (int side = 0; side < 2; ++side) {
    const double hs = side ? -a.h : a.h, hh = side ? -a.hh : a.hh;
    double p[3] = {p0[0], p0[1], p0[2]}, v[3] = {v0[0], v0[1], v0[2]};
    double A = 0.0, Wt = 0.0;
    int n = 0, end = FS_LIC_FULL;
    for (int i = 1; i <= a.L; ++i) {
      double d[3] = {0.0, 0.0, 0.0}, q[3] = {0.0, 0.0, 0.0}, t;
      end = direction<C>(v, a.vmin, d);
      if (end != FS_LIC_FULL) break;
      if (M == FS_ADV_RK2) {
        double vm[3];
#pragma unroll
        for (int c = 0; c < C; ++c) q[c] = p[c] + hh * d[c];
        gather<C, true, false>(src, a, q, vm, t);
        end = direction<C>(vm, a.vmin, d);
        if (end != FS_LIC_FULL) break;
      }
#pragma unroll
      for (int c = 0; c < C; ++c) q[c] = p[c] + hs * d[c];
      if (!alive<C>(q, a)) {
        end = FS_LIC_OUT;
        break;
      }
#pragma unroll
      for (int c = 0; c < C; ++c) p[c] = q[c];
      gather<C, true, true>(src, a, p, v, t);
      const double wi = w[i];
      A = A + wi * t;
      Wt = Wt + wi;
      n += 1;
    }
    acc = acc + A;
    wsum = wsum + Wt;
    cnt += n;
    code |= end << (2 * side);
  }
  const size_t o = (size_t)k * (size_t)a.plane + ((size_t)z * a.H + (size_t)y) * a.W + (size_t)x;
  out[o] = (float)(acc / wsum);
  if (ends) ends[o] = (unsigned char)code;
  if (count) count[o] = cnt;
}

// the packed image: img[k][node] = (v_x, v_y[, v_z], tex[, 0])
template <int C>
__global__ __launch_bounds__(NT) void lic_pack_kernel(const float* __restrict__ flows, const float* __restrict__ tex,
                                                      float4* __restrict__ img, LP a) {
  const long long gid = (long long)blockIdx.x * NT + threadIdx.x;
  if (gid >= (long long)a.K * a.plane) return;
  const long long k = gid / a.plane, r = gid - k * a.plane;
  const float* fk = flows + (size_t)k * a.fss;
  const float t = tex[(size_t)k * a.tss + r];
  img[gid] = C == 3 ? make_float4(fk[r], fk[a.plane + r], fk[2 * a.plane + r], t)
                    : make_float4(fk[r], fk[a.plane + r], t, 0.f);
}

template <int C, int M, bool TILE>
__global__ __launch_bounds__(NT) void lic_kernel(const float4* __restrict__ img, const double* __restrict__ w,
                                                 float* __restrict__ out, unsigned char* __restrict__ ends,
                                                 int* __restrict__ count, LP a) {
  const long long gid = (long long)blockIdx.x * NT + threadIdx.x;
  if (gid >= a.total) return;
  int k, x, y, z;
  if (!node_of<C, TILE>(a, gid, k, x, y, z)) return;
  const PackedSrc src{img + (size_t)k * a.plane};
  lic_node<C, M>(src, w, out, ends, count, a, k, x, y, z);
}

#ifdef FS_ABLATION
template <int C, int M, bool TILE>
__global__ __launch_bounds__(NT) void lic_planes_kernel(const float* __restrict__ flows, const float* __restrict__ tex,
                                                        const double* __restrict__ w, float* __restrict__ out,
                                                        unsigned char* __restrict__ ends, int* __restrict__ count,
                                                        LP a) {
  const long long gid = (long long)blockIdx.x * NT + threadIdx.x;
  if (gid >= a.total) return;
  int k, x, y, z;
  if (!node_of<C, TILE>(a, gid, k, x, y, z)) return;
  const PlaneSrc src{flows + (size_t)k * a.fss, tex + (size_t)k * a.tss, a.plane};
  lic_node<C, M>(src, w, out, ends, count, a, k, x, y, z);
}
#endif

long long ws_bytes(int K, int D, int H, int W) {
  if (K < 1 || D < 1 || H < 1 || W < 1) return -(long long)FS_ERR_SHAPE;
  const long long plane = (long long)D * H * W;
  if (plane > (1LL << 40) / 3 || plane > (1LL << 58) / K) return -(long long)FS_ERR_SHAPE;
  return 16 * (long long)K * plane;
}

int launch(bool is3d, const float* flows, int K, int C, int D, int H, int W, long long fss, const float* tex,
           long long tss, const double* weights, int L, double h, double vmin, int method, float* out,
           unsigned char* ends, int* count, void* ws, fs_stream_t stream) {
  FS_ENTER();
  FS_REQUIRE_PTR(flows); FS_REQUIRE_PTR(tex); FS_REQUIRE_PTR(weights); FS_REQUIRE_PTR(out); FS_REQUIRE_PTR(ws);
  if (K < 1 || C != (is3d ? 3 : 2) || D < 1 || H < 1 || W < 1) return FS_ERR_SHAPE;
  if (ws_bytes(K, D, H, W) < 0) return FS_ERR_SHAPE;
  const long long plane = (long long)D * H * W;
  if (K > 1 && fss < C * plane) return FS_ERR_SHAPE;
  if (tss < 0 || (K > 1 && tss != 0 && tss < plane)) return FS_ERR_SHAPE;
  LP a;
  a.fss = fss; a.tss = tss; a.plane = plane; a.K = K; a.D = D; a.H = H; a.W = W; a.L = L;
  bool tile = is3d;
#ifdef FS_ABLATION
  bool packed = true;
  // read per call: 1 rows + planes, 2 tiles + planes, 3 rows + packed, 4 tiles + packed (unset or 0: the product's form)
  const long long variant = FS_AB_ENV_LL("FLOWSCI_LIC_VARIANT", 0);
  if (variant >= 1 && variant <= 4) {
    tile = ((variant - 1) & 1) != 0;
    packed = variant >= 3;
  }
#endif
  const int tx = is3d ? 4 : 8;
  a.tw = (W + tx - 1) / tx; a.th = (H + tx - 1) / tx; a.td = is3d ? (D + 3) / 4 : 1;
  a.total = tile ? (long long)K * a.td * a.th * a.tw * 64 : (long long)K * plane;
  const long long blocks = (a.total + NT - 1) / NT, pblocks = ((long long)K * plane + NT - 1) / NT;
  if (blocks > 0x7fffffffLL || pblocks > 0x7fffffffLL) return FS_ERR_SHAPE;
  if (L < 0 || L > FS_LIC_MAX_L) return FS_ERR_ARG;
  if (!(h > 0.0 && h < HUGE_VAL) || !(vmin >= 0.0 && vmin < HUGE_VAL)) return FS_ERR_ARG;
  if (method != FS_ADV_EULER && method != FS_ADV_RK2) return FS_ERR_ARG;
  if (((uintptr_t)ws & 15) != 0) return FS_ERR_ARG;
  a.h = h; a.hh = 0.5 * h; a.vmin = vmin;
  const hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)blocks), pgrid((unsigned)pblocks), blk(NT);
  float4* img = (float4*)ws;
#define FS_LIC_LAUNCH(KERNEL, CC, TT, ...)                                                                      \
  do {                                                                                                          \
    if (method == FS_ADV_EULER) hipLaunchKernelGGL((KERNEL<CC, FS_ADV_EULER, TT>), grid, blk, 0, s, __VA_ARGS__); \
    else hipLaunchKernelGGL((KERNEL<CC, FS_ADV_RK2, TT>), grid, blk, 0, s, __VA_ARGS__);                         \
  } while (0)
#ifdef FS_ABLATION
  if (!packed) {
    if (is3d && tile) FS_LIC_LAUNCH(lic_planes_kernel, 3, true, flows, tex, weights, out, ends, count, a);
    else if (is3d) FS_LIC_LAUNCH(lic_planes_kernel, 3, false, flows, tex, weights, out, ends, count, a);
    else if (tile) FS_LIC_LAUNCH(lic_planes_kernel, 2, true, flows, tex, weights, out, ends, count, a);
    else FS_LIC_LAUNCH(lic_planes_kernel, 2, false, flows, tex, weights, out, ends, count, a);
    FS_LAUNCH_CHECK();
    return FS_OK;
  }
  if (tile != is3d) {
    if (is3d) {
      hipLaunchKernelGGL((lic_pack_kernel<3>), pgrid, blk, 0, s, flows, tex, img, a);
      FS_LIC_LAUNCH(lic_kernel, 3, false, img, weights, out, ends, count, a);
    } else {
      hipLaunchKernelGGL((lic_pack_kernel<2>), pgrid, blk, 0, s, flows, tex, img, a);
      FS_LIC_LAUNCH(lic_kernel, 2, true, img, weights, out, ends, count, a);
    }
    FS_LAUNCH_CHECK();
    return FS_OK;
  }
#endif
  if (is3d) {
    hipLaunchKernelGGL((lic_pack_kernel<3>), pgrid, blk, 0, s, flows, tex, img, a);
    FS_LIC_LAUNCH(lic_kernel, 3, true, img, weights, out, ends, count, a);
  } else {
    hipLaunchKernelGGL((lic_pack_kernel<2>), pgrid, blk, 0, s, flows, tex, img, a);
    FS_LIC_LAUNCH(lic_kernel, 2, false, img, weights, out, ends, count, a);
  }
#undef FS_LIC_LAUNCH
  FS_LAUNCH_CHECK();
  return FS_OK;
}

}  // namespace

extern "C" long long fs_lic2d_ws_bytes(int K, int H, int W) { return ws_bytes(K, 1, H, W); }

extern "C" long long fs_lic3d_ws_bytes(int K, int D, int H, int W) { return ws_bytes(K, D, H, W); }

extern "C" int fs_lic2d(const float* flows, int K, int C, int H, int W, long long flow_sstride, const float* tex,
                        long long tex_sstride, const double* weights, int L, double h, double vmin, int method,
                        float* out, unsigned char* ends, int* count, void* ws, fs_stream_t stream) {
  return launch(false, flows, K, C, 1, H, W, flow_sstride, tex, tex_sstride, weights, L, h, vmin, method, out, ends,
                count, ws, stream);
}

extern "C" int fs_lic3d(const float* flows, int K, int C, int D, int H, int W, long long flow_sstride, const float* tex,
                        long long tex_sstride, const double* weights, int L, double h, double vmin, int method,
                        float* out, unsigned char* ends, int* count, void* ws, fs_stream_t stream) {
  return launch(true, flows, K, C, D, H, W, flow_sstride, tex, tex_sstride, weights, L, h, vmin, method, out, ends,
                count, ws, stream);
}
