// flowmetrics.hip -- optical-flow accuracy of N predicted flows against N ground-truth displacements in one launch:
// end-point error (EPE), RMSE, Barron's angular error, the KITTI outlier rate Fl and the largest EPE, over a `valid`
// mask and split by a `noc` (not occluded) mask.  The reference only prints or plots flows (UPFlow/test.py:167-176 has
// its KITTI "EPE All / F1 / EPE Noc / EPE Occ" commented out); these are the numbers users of flow methods expect.
//
// Per element (pred p, gt g, both C-vectors; p first converted to a displacement under the rife3d convention):
//   e2  = sum_c (p_c - g_c)^2                          fp64 (the differences of fp32 values are exact in fp64)
//   epe = sqrt(e2)                                      fp64; the map stores it rounded to fp32
//   ae  = atan2(sqrt(sum_{i<j} (a_i b_j - a_j b_i)^2), a.b),  a = (p, 1), b = (g, 1): the two arguments in fp64, the
//         atan2 in fp32 (acos(a.b / |a||b|) is ill-conditioned at small angles)
//   outlier: e2 > tau_abs^2 && e2 > tau_rel^2 |g|^2    fp64, contraction off: a restatement with the same operations
//         in numpy fp64 reproduces every count exactly
// rife3d (Flow-3D's warp rotates axes, oracle warp3d_closed): out[d,h,w] samples the input at
//   ix = (h + F0)(W-1)/(H-1), iy = (d + F1)(H-1)/(D-1), iz = (w + F2)(D-1)/(W-1)
// so the displacement is x = ix - w, y = iy - h, z = iz - d (not clamped), evaluated in fp64.
//
// Layout: streaming, HBM-bound.  A flow's D*H*W elements are cut into groups of V = 4 consecutive elements of the
// flattened plane (16-byte loads of every channel plane, 4-byte mask loads, 16-byte map stores; a group may straddle
// rows) when the plane size, strides and pointers allow it, else V = 1.  Workgroup b of flow n takes groups b*256 + tid, stepping by G*256; under rife3d the thread
// decodes (d, h, w) of its first group once and then advances them by carries (no division per element).  Each
// thread accumulates in fp64 (counts as integers), each workgroup writes its K partials to `ws` ([N][K][G]) and a second
// launch, one workgroup per (flow, statistic), adds the G partials in a fixed order: no atomics, bitwise reproducible.
#include "common.hpp"

namespace {

constexpr int NT = 256;
constexpr int K = FS_FLOW_METRICS_K;
constexpr long long kTargetBlocks = 1024;  // 4 workgroups (16 waves) per CU, all resident at once (<= 128 VGPRs)
constexpr long long kMaxBlocks = 1LL << 24;

struct FP {
  long long Q;             // groups of V elements per flow = D*H*W / V
  long long P;             // elements per channel plane = D*H*W
  long long pbs, gbs;      // batch strides (elements) of pred and gt
  int G;                   // workgroups per flow
  int D, H, W;
  double rx, ry, rz;       // rife3d: (W-1)/(H-1), (H-1)/(D-1), (D-1)/(W-1)
  double ta2, tr2;         // tau_abs^2, tau_rel^2
};

struct Acc {
  unsigned n, nout, nn, nnout, nf, nfn;
  double se, se2, sae, mx, sen, se2n, saen;
};

template <int C, bool RIFE>
__device__ __forceinline__ void element(const float (&p)[3], const float (&g)[3], int d, int h, int w, bool vld,
                                        bool nc, const FP& f, Acc& a, float& map) {
#pragma clang fp contract(off)
  bool fin = true;
#pragma unroll
  for (int c = 0; c < C; ++c) fin = fin && isfinite(p[c]) && isfinite(g[c]);
  double pd[3], gd[3];
#pragma unroll
  for (int c = 0; c < C; ++c) { pd[c] = (double)p[c]; gd[c] = (double)g[c]; }
  if (RIFE) {
    pd[0] = ((double)h + pd[0]) * f.rx - (double)w;
    pd[1] = ((double)d + pd[1]) * f.ry - (double)h;
    pd[2] = ((double)w + pd[2]) * f.rz - (double)d;
  }
  double e2 = 0.0, g2 = 0.0, dot = 1.0;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const double dc = pd[c] - gd[c];
    e2 = e2 + dc * dc;
    g2 = g2 + gd[c] * gd[c];
    dot = dot + pd[c] * gd[c];
  }
  // |a x b|^2 of a = (p, 1), b = (g, 1): the pairs (i, j) among the C components, then (i, last) = p_i - g_i
  double c2 = e2;
#pragma unroll
  for (int i = 0; i < C; ++i) {
#pragma unroll
    for (int j = i + 1; j < C; ++j) {
      const double t = pd[i] * gd[j] - pd[j] * gd[i];
      c2 = c2 + t * t;
    }
  }
  const double epe = sqrt(e2);
  map = fin ? (float)epe : __builtin_nanf("");
  if (!vld) return;
  const bool out = !fin || (e2 > f.ta2 && e2 > f.tr2 * g2);
  a.n += 1;
  a.nout += out;
  a.nf += !fin;
  if (nc) { a.nn += 1; a.nnout += out; a.nfn += !fin; }
  if (!fin) return;
  const double ae = (double)atan2f((float)sqrt(c2), (float)dot);
  a.se += epe; a.se2 += e2; a.sae += ae; a.mx = fmax(a.mx, epe);
  if (nc) { a.sen += epe; a.se2n += e2; a.saen += ae; }
}

template <int C, int V, bool RIFE>
__global__ __launch_bounds__(NT) void flow_metrics_kernel(const float* __restrict__ pred, const float* __restrict__ gt,
                                                          const unsigned char* __restrict__ valid,
                                                          const unsigned char* __restrict__ noc,
                                                          float* __restrict__ emap, double* __restrict__ ws, FP f) {
  const int n = blockIdx.x / f.G, b = blockIdx.x - n * f.G;
  const float* pp = pred + (size_t)n * f.pbs;
  const float* gp = gt + (size_t)n * f.gbs;
  const unsigned char* vp = valid ? valid + (size_t)n * f.P : nullptr;
  const unsigned char* np = noc ? noc + (size_t)n * f.P : nullptr;
  float* mp = emap ? emap + (size_t)n * f.P : nullptr;
  Acc a = {0u, 0u, 0u, 0u, 0u, 0u, 0.0, 0.0, 0.0, -HUGE_VAL, 0.0, 0.0, 0.0};
  const long long S = (long long)f.G * NT;
  long long q = (long long)b * NT + threadIdx.x;
  // rife3d: (d, h, w) of the group's first element, decoded once, then advanced by S*V elements per step with carries
  // (a group of V consecutive elements of the plane may straddle rows: its elements step by one, also with carries)
  int w = 0, h = 0, d = 0, sw = 0, sh = 0, sd = 0;
  if (RIFE) {
    const long long e0 = q * V, r = e0 / f.W;
    w = (int)(e0 - r * f.W); h = (int)(r % f.H); d = (int)(r / f.H);
    const long long E = S * V, sr = E / f.W;
    sw = (int)(E - sr * f.W); sh = (int)(sr % f.H); sd = (int)(sr / f.H);
  }
  for (; q < f.Q; q += S) {
    const size_t e = (size_t)q * V;
    float pv[3][V], gv[3][V];
#pragma unroll
    for (int c = 0; c < C; ++c) {
      if (V == 4) {
        const float4 x = *reinterpret_cast<const float4*>(pp + c * f.P + e);
        const float4 y = *reinterpret_cast<const float4*>(gp + c * f.P + e);
        pv[c][0] = x.x; pv[c][1] = x.y; pv[c][2] = x.z; pv[c][3] = x.w;
        gv[c][0] = y.x; gv[c][1] = y.y; gv[c][2] = y.z; gv[c][3] = y.w;
      } else {
        pv[c][0] = pp[c * f.P + e];
        gv[c][0] = gp[c * f.P + e];
      }
    }
    unsigned vm = 0x01010101u, nm = 0u;
    if (V == 4) {
      if (vp) vm = *reinterpret_cast<const unsigned*>(vp + e);
      if (np) nm = *reinterpret_cast<const unsigned*>(np + e);
    } else {
      if (vp) vm = vp[e];
      if (np) nm = np[e];
    }
    float m[V];
    int wi = w, hi = h, di = d;
#pragma unroll
    for (int i = 0; i < V; ++i) {
      float p3[3] = {0.f, 0.f, 0.f}, g3[3] = {0.f, 0.f, 0.f};
#pragma unroll
      for (int c = 0; c < C; ++c) { p3[c] = pv[c][i]; g3[c] = gv[c][i]; }
      const bool vi = ((vm >> (8 * i)) & 0xffu) != 0u;
      const bool ni = vi && ((nm >> (8 * i)) & 0xffu) != 0u;
      element<C, RIFE>(p3, g3, di, hi, wi, vi, ni, f, a, m[i]);
      if (RIFE && i + 1 < V && ++wi == f.W) {
        wi = 0;
        if (++hi == f.H) { hi = 0; ++di; }
      }
    }
    if (mp) {
      if (V == 4)
        *reinterpret_cast<float4*>(mp + e) = make_float4(m[0], m[V > 1 ? 1 : 0], m[V > 2 ? 2 : 0], m[V > 3 ? 3 : 0]);
      else
        mp[e] = m[0];
    }
    if (RIFE) {
      w += sw;
      const int cw = w >= f.W;
      w -= cw ? f.W : 0;
      h += sh + cw;
      const int ch = h >= f.H;
      h -= ch ? f.H : 0;
      d += sd + ch;
    }
  }
  // workgroup reduction: wave butterflies, then the four waves in a fixed order
  double v[K] = {(double)a.n, a.se, a.se2, a.sae, (double)a.nout, a.mx,
                 (double)a.nn, a.sen, a.se2n, a.saen, (double)a.nnout, (double)a.nf, (double)a.nfn};
#pragma unroll
  for (int k = 0; k < K; ++k) v[k] = (k == FS_FM_MAX_EPE) ? fs::wave_max(v[k]) : fs::wave_sum(v[k]);
  __shared__ double red[NT / 64][K];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < K; ++k) red[wv][k] = v[k];
  }
  __syncthreads();
  if (threadIdx.x < K) {
    const int k = threadIdx.x;
    const double r = (k == FS_FM_MAX_EPE) ? fmax(fmax(red[0][k], red[1][k]), fmax(red[2][k], red[3][k]))
                                          : (red[0][k] + red[1][k]) + (red[2][k] + red[3][k]);
    ws[((size_t)n * K + k) * f.G + b] = r;  // [N][K][G]: the second stage reads each statistic contiguously
  }
}

// Second stage: one workgroup per (flow n, statistic k) adds the G partials ws[n][k][0..G) in a fixed order -> out[n][k].
__global__ __launch_bounds__(NT) void flow_metrics_final_kernel(const double* __restrict__ ws, int G,
                                                                double* __restrict__ out) {
  __shared__ double red[NT];
  const int k = blockIdx.x % K;
  const bool mx = k == FS_FM_MAX_EPE;
  const double* w = ws + (size_t)blockIdx.x * G;
  double s = mx ? -HUGE_VAL : 0.0;
  for (int i = threadIdx.x; i < G; i += NT) s = mx ? fmax(s, w[i]) : s + w[i];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int t = NT / 2; t > 0; t >>= 1) {
    if ((int)threadIdx.x < t)
      red[threadIdx.x] = mx ? fmax(red[threadIdx.x], red[threadIdx.x + t]) : red[threadIdx.x] + red[threadIdx.x + t];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[blockIdx.x] = red[0];
}

inline bool aligned(const void* p, size_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

// Geometry of a call: FS_OK and f filled, or FS_ERR_*.  Pointers are only looked at for the vector width.
int plan(bool is3d, int N, int C, int D, int H, int W, long long pbs, long long gbs, int convention, FP& f,
         long long& blocks) {
  if (N < 1 || C != (is3d ? 3 : 2) || D < 1 || H < 1 || W < 1) return FS_ERR_SHAPE;
  if (convention != FS_FLOW_DISP && !(is3d && convention == FS_FLOW_RIFE3D)) return FS_ERR_ARG;
  if (convention == FS_FLOW_RIFE3D && (D < 2 || H < 2 || W < 2)) return FS_ERR_SHAPE;
  const long long P = (long long)D * H * W;
  if (P > (1LL << 40) / C) return FS_ERR_SHAPE;
  if (N > 1 && (pbs < C * P || gbs < C * P)) return FS_ERR_SHAPE;
  f.P = P; f.pbs = pbs; f.gbs = gbs;
  f.D = D; f.H = H; f.W = W;
  f.rx = (double)(W - 1) / (double)(H - 1 > 0 ? H - 1 : 1);
  f.ry = (double)(H - 1) / (double)(D - 1 > 0 ? D - 1 : 1);
  f.rz = (double)(D - 1) / (double)(W - 1 > 0 ? W - 1 : 1);
  const long long Q1 = P;  // groups at V = 1 (the workspace is sized for the larger grid)
  long long G = (kTargetBlocks + N - 1) / N;
  const long long gmax = (Q1 + NT - 1) / NT;
  if (G > gmax) G = gmax;
  if (G < 1) G = 1;
  f.G = (int)G;
  blocks = (long long)N * G;
  if (blocks > kMaxBlocks) return FS_ERR_SHAPE;
  return FS_OK;
}

int launch(bool is3d, const float* pred, const float* gt, int N, int C, int D, int H, int W, long long pbs,
           long long gbs, const unsigned char* valid, const unsigned char* noc, int convention, float tau_abs,
           float tau_rel, float* emap, double* ws, double* out, fs_stream_t stream) {
  FS_ENTER();
  FS_REQUIRE_PTR(pred); FS_REQUIRE_PTR(gt); FS_REQUIRE_PTR(ws); FS_REQUIRE_PTR(out);
  FP f;
  long long blocks = 0;
  const int rc = plan(is3d, N, C, D, H, W, pbs, gbs, convention, f, blocks);
  if (rc != FS_OK) return rc;
  if (!(tau_abs >= 0.f && tau_abs < HUGE_VALF && tau_rel >= 0.f && tau_rel < HUGE_VALF)) return FS_ERR_ARG;
  f.ta2 = (double)tau_abs * (double)tau_abs;
  f.tr2 = (double)tau_rel * (double)tau_rel;
  // a flow's C planes are contiguous: groups of 4 run along the flattened plane (rows of any length), so the
  // 16-byte path needs the plane size, not W, to be a multiple of 4 -- else planes c > 0 start misaligned
  const bool v4 = f.P % 4 == 0 && pbs % 4 == 0 && gbs % 4 == 0 && aligned(pred, 16) && aligned(gt, 16) &&
                  aligned(valid, 4) && aligned(noc, 4) && aligned(emap, 16);
  const int V = v4 ? 4 : 1;
  f.Q = f.P / V;
  const bool rife = convention == FS_FLOW_RIFE3D;
  const hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)blocks), blk(NT);
#define FS_FM_LAUNCH(CC, VV, RR) \
  hipLaunchKernelGGL((flow_metrics_kernel<CC, VV, RR>), grid, blk, 0, s, pred, gt, valid, noc, emap, ws, f)
  if (!is3d) {
    if (v4) FS_FM_LAUNCH(2, 4, false); else FS_FM_LAUNCH(2, 1, false);
  } else if (rife) {
    if (v4) FS_FM_LAUNCH(3, 4, true); else FS_FM_LAUNCH(3, 1, true);
  } else {
    if (v4) FS_FM_LAUNCH(3, 4, false); else FS_FM_LAUNCH(3, 1, false);
  }
#undef FS_FM_LAUNCH
  hipLaunchKernelGGL(flow_metrics_final_kernel, dim3((unsigned)(N * K)), dim3(NT), 0, s, ws, f.G, out);
  FS_LAUNCH_CHECK();
  return FS_OK;
}

long long ws_bytes(bool is3d, int N, int C, int D, int H, int W, int convention) {
  FP f;
  long long blocks = 0;
  const long long P = (long long)D * H * W;
  const int rc = plan(is3d, N, C, D, H, W, (long long)C * P, (long long)C * P, convention, f, blocks);
  if (rc != FS_OK) return -rc;
  return blocks * K * (long long)sizeof(double);
}

}  // namespace

extern "C" long long fs_flow_metrics2d_ws_bytes(int N, int C, int H, int W) {
  return ws_bytes(false, N, C, 1, H, W, FS_FLOW_DISP);
}

extern "C" long long fs_flow_metrics3d_ws_bytes(int N, int C, int D, int H, int W, int convention) {
  return ws_bytes(true, N, C, D, H, W, convention);
}

extern "C" int fs_flow_metrics2d(const float* pred, const float* gt, int N, int C, int H, int W, long long pred_bstride,
                                 long long gt_bstride, const unsigned char* valid, const unsigned char* noc,
                                 float tau_abs, float tau_rel, float* epe_map, double* ws, double* out,
                                 fs_stream_t stream) {
  return launch(false, pred, gt, N, C, 1, H, W, pred_bstride, gt_bstride, valid, noc, FS_FLOW_DISP, tau_abs, tau_rel,
                epe_map, ws, out, stream);
}

extern "C" int fs_flow_metrics3d(const float* pred, const float* gt, int N, int C, int D, int H, int W,
                                 long long pred_bstride, long long gt_bstride, const unsigned char* valid,
                                 const unsigned char* noc, int convention, float tau_abs, float tau_rel,
                                 float* epe_map, double* ws, double* out, fs_stream_t stream) {
  return launch(true, pred, gt, N, C, D, H, W, pred_bstride, gt_bstride, valid, noc, convention, tau_abs, tau_rel,
                epe_map, ws, out, stream);
}
