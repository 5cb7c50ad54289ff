// flowconsist.hip -- label-free flow quality: the forward-backward consistency of N pairs of displacements (flow_f maps
// frame a to frame b on a's grid, flow_b maps b to a on b's grid) and the photometric error of the flow-warped frame,
// in one launch.  UnFlow's occlusion test (Meister et al. 2018, eq. 1): an element is occluded when
//   |F_f(x) + F_b(x + F_f(x))|^2 > alpha1 (|F_f(x)|^2 + |F_b(x + F_f(x))|^2) + alpha2.
// fs_occ_check2d is UPFlow's training-side form of it (zero-padded align_corners=False warp, L1 magnitudes, 2-D, masks
// only); this one is a measurement: 2-D and 3-D, displacements in elements, numbers out.
//
// Per element x (fp64, contraction off: a numpy fp64 restatement with the same operations in the same order reproduces
// every count exactly -- tests/flow_consistency_ref.py):
//   p_c = x_c + F_f,c(x); a non-finite F_f,c -> NONFINITE; else p_c < 0 or p_c > S_c - 1 -> OUTGOING (border inclusive)
//   Fbw_c and I1w = flow_b's C planes and img1 sampled at p by the rule trilinear64.hpp states (p lies inside: nothing
//   to clamp).  element() keeps its OWN copy of those lines and does not include the header: on corners64 the 3-D
//   kernels measured 2 - 3 % slower on white-noise flows, outside the parent's spread, with equal instruction counts
//   (profiles/trilinear64.txt) -- a change to the rule is made there and here
//   r2 = sum_c (F_f,c + Fbw_c)^2, m2 = sum_c F_f,c^2 + sum_c Fbw_c^2, r = sqrt(r2), e = I1w - I0(x)
//   Fbw (or, with images, I0(x) or I1w) not finite -> NONFINITE; else r2 > alpha1 m2 + alpha2 -> OCCLUDED, else CONSISTENT
//
// Layout: flow_f, img0, valid and the maps stream as flowmetrics.hip's operands do (groups of V = 4 consecutive
// elements of the flattened plane when the plane size is a multiple of 4, moved by 16-byte loads and stores when
// strides and pointers allow and element by element otherwise; V = 1 for other plane sizes); the 2^C x (C + 1) corner
// reads of flow_b / img1 are plain global gathers: neighbouring lanes sample neighbouring points of a smooth flow, so a
// wave's corner reads fall into a few cache lines that the x / x+1 and y / y+1 corners share.  (d, h, w) of a thread's first element are decoded once and advanced by carries.  Each thread
// accumulates in fp64 (counts as integers), each workgroup writes its K partials to `ws` ([N][K][G]) and a second
// launch adds the G partials in a fixed order: no atomics, bitwise reproducible.
#include "common.hpp"

namespace {

constexpr int NT = 256;
constexpr int K = FS_FLOW_CONSISTENCY_K;
constexpr long long kTargetBlocks = 1024;  // as flowmetrics.hip: 4 workgroups per CU
constexpr long long kMaxBlocks = 1LL << 24;

struct CP {
  long long Q;         // groups of V elements per flow
  long long P;         // elements per plane = D*H*W
  long long fbs, bbs;  // batch strides (elements) of flow_f and flow_b
  int G;               // workgroups per flow
  int D, H, W;
  double a1, a2;
};

struct Acc {
  unsigned n, nnf, nout, nocc, nnoc;
  double sr, sr2, mx, srn, sa, se2, san, se2n;
};

// One element.  fb / i1p: flow n of flow_b and of img1.  Returns the class as if the element were valid.
template <int C, bool IMG>
__device__ __forceinline__ int element(const float (&ff)[3], float i0v, int d, int h, int w, bool vld,
                                       const float* __restrict__ fb, const float* __restrict__ i1p, const CP& f,
                                       Acc& a, float& res) {
#pragma clang fp contract(off)
  const float nanf_ = __builtin_nanf("");
  res = nanf_;
  bool fin = true;
#pragma unroll
  for (int c = 0; c < C; ++c) fin = fin && isfinite(ff[c]);
  if (!fin) {
    if (vld) { a.n += 1; a.nnf += 1; }
    return FS_FC_NONFINITE;
  }
  const int x[3] = {w, h, d}, S[3] = {f.W, f.H, f.D};
  double fd[3], p[3];
  bool out = false;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    fd[c] = (double)ff[c];
    p[c] = (double)x[c] + fd[c];
    out = out || p[c] < 0.0 || p[c] > (double)(S[c] - 1);
  }
  if (out) {
    if (vld) { a.n += 1; a.nout += 1; }
    return FS_FC_OUTGOING;
  }
  // 0 <= p_c <= S_c - 1 from here on: every corner index below lies inside the plane
  double fr[3], gr[3];
  size_t o0[3], o1[3];
  const size_t st[3] = {(size_t)1, (size_t)f.W, (size_t)f.W * (size_t)f.H};
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const double fl = floor(p[c]);
    const int i0 = (int)fl;
    const int i1 = i0 + 1 < S[c] ? i0 + 1 : S[c] - 1;
    fr[c] = p[c] - fl;
    gr[c] = 1.0 - fr[c];
    o0[c] = (size_t)i0 * st[c];
    o1[c] = (size_t)i1 * st[c];
  }
  double Fbw[3] = {0.0, 0.0, 0.0}, I1w = 0.0;
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
#pragma unroll
    for (int c = 0; c < C; ++c) Fbw[c] = Fbw[c] + wt * (double)fb[(size_t)c * f.P + o];
    if (IMG) I1w = I1w + wt * (double)i1p[o];
  }
  double r2 = 0.0, sa = 0.0, sb = 0.0;
  bool sfin = true;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const double s = fd[c] + Fbw[c];
    r2 = r2 + s * s;
    sa = sa + fd[c] * fd[c];
    sb = sb + Fbw[c] * Fbw[c];
    sfin = sfin && isfinite(Fbw[c]);
  }
  const double m2 = sa + sb;
  const double r = sqrt(r2);
  if (IMG) sfin = sfin && isfinite(i0v) && isfinite(I1w);
  if (!sfin) {
    if (vld) { a.n += 1; a.nnf += 1; }
    return FS_FC_NONFINITE;
  }
  res = (float)r;
  const bool occ = r2 > f.a1 * m2 + f.a2;
  if (vld) {
    a.n += 1;
    a.sr += r; a.sr2 += r2; a.mx = fmax(a.mx, r);
    double ae = 0.0, e2 = 0.0;
    if (IMG) {
      const double e = I1w - (double)i0v;
      ae = fabs(e); e2 = e * e;
      a.sa += ae; a.se2 += e2;
    }
    if (occ) {
      a.nocc += 1;
    } else {
      a.nnoc += 1;
      a.srn += r;
      if (IMG) { a.san += ae; a.se2n += e2; }
    }
  }
  return occ ? FS_FC_OCCLUDED : FS_FC_CONSISTENT;
}

// V: elements per thread and step (4 when the plane size is a multiple of 4, else 1); VEC: they move as one 16-byte
// (maps and mask: 4-byte) access, which needs aligned pointers and strides.  Which elements a thread takes depends on V
// only, so a misaligned copy of the same operands gives the same sums bit for bit.
template <int C, int V, bool VEC, bool IMG>
__global__ __launch_bounds__(NT) void flow_consistency_kernel(const float* __restrict__ flow_f,
                                                              const float* __restrict__ flow_b,
                                                              const float* __restrict__ img0,
                                                              const float* __restrict__ img1,
                                                              const unsigned char* __restrict__ valid,
                                                              unsigned char* __restrict__ cmap,
                                                              float* __restrict__ rmap, double* __restrict__ ws, CP f) {
  const int n = blockIdx.x / f.G, b = blockIdx.x - n * f.G;
  const float* fp = flow_f + (size_t)n * f.fbs;
  const float* bp = flow_b + (size_t)n * f.bbs;
  const float* i0p = IMG ? img0 + (size_t)n * f.P : nullptr;
  const float* i1p = IMG ? img1 + (size_t)n * f.P : nullptr;
  const unsigned char* vp = valid ? valid + (size_t)n * f.P : nullptr;
  unsigned char* cp = cmap ? cmap + (size_t)n * f.P : nullptr;
  float* rp = rmap ? rmap + (size_t)n * f.P : nullptr;
  Acc a = {0u, 0u, 0u, 0u, 0u, 0.0, 0.0, -HUGE_VAL, 0.0, 0.0, 0.0, 0.0, 0.0};
  const long long S = (long long)f.G * NT;
  long long q = (long long)b * NT + threadIdx.x;
  // (d, h, w) of the group's first element, decoded once, then advanced by S*V elements per step with carries (a
  // group of V consecutive elements of the plane may straddle rows: its elements step by one, also with carries)
  int w, h, d, sw, sh, sd;
  {
    const long long e0 = q * V, r = e0 / f.W;
    w = (int)(e0 - r * f.W); h = (int)(r % f.H); d = (int)(r / f.H);
    const long long E = S * V, sr = E / f.W;
    sw = (int)(E - sr * f.W); sh = (int)(sr % f.H); sd = (int)(sr / f.H);
  }
  for (; q < f.Q; q += S) {
    const size_t e = (size_t)q * V;
    float fv[3][V], iv[V];
#pragma unroll
    for (int c = 0; c < C; ++c) {
      if (VEC) {
        const float4 t = *reinterpret_cast<const float4*>(fp + (size_t)c * f.P + e);
        fv[c][0] = t.x; fv[c][V > 1 ? 1 : 0] = t.y; fv[c][V > 2 ? 2 : 0] = t.z; fv[c][V > 3 ? 3 : 0] = t.w;
      } else {
#pragma unroll
        for (int i = 0; i < V; ++i) fv[c][i] = fp[(size_t)c * f.P + e + i];
      }
    }
#pragma unroll
    for (int i = 0; i < V; ++i) iv[i] = 0.f;
    if (IMG) {
      if (VEC) {
        const float4 t = *reinterpret_cast<const float4*>(i0p + e);
        iv[0] = t.x; iv[V > 1 ? 1 : 0] = t.y; iv[V > 2 ? 2 : 0] = t.z; iv[V > 3 ? 3 : 0] = t.w;
      } else {
#pragma unroll
        for (int i = 0; i < V; ++i) iv[i] = i0p[e + i];
      }
    }
    unsigned vm = 0x01010101u;
    if (vp) {
      if (VEC) {
        vm = *reinterpret_cast<const unsigned*>(vp + e);
      } else {
        vm = 0u;
#pragma unroll
        for (int i = 0; i < V; ++i) vm |= (unsigned)vp[e + i] << (8 * i);
      }
    }
    float m[V];
    unsigned cls = 0u;
    int wi = w, hi = h, di = d;
#pragma unroll
    for (int i = 0; i < V; ++i) {
      float f3[3] = {0.f, 0.f, 0.f};
#pragma unroll
      for (int c = 0; c < C; ++c) f3[c] = fv[c][i];
      const bool vi = ((vm >> (8 * i)) & 0xffu) != 0u;
      const int k = element<C, IMG>(f3, iv[i], di, hi, wi, vi, bp, i1p, f, a, m[i]);
      cls |= (vi ? (unsigned)k : 0u) << (8 * i);
      if (i + 1 < V && ++wi == f.W) {
        wi = 0;
        if (++hi == f.H) { hi = 0; ++di; }
      }
    }
    if (rp) {
      if (VEC) {
        *reinterpret_cast<float4*>(rp + e) = make_float4(m[0], m[V > 1 ? 1 : 0], m[V > 2 ? 2 : 0], m[V > 3 ? 3 : 0]);
      } else {
#pragma unroll
        for (int i = 0; i < V; ++i) rp[e + i] = m[i];
      }
    }
    if (cp) {
      if (VEC) {
        *reinterpret_cast<unsigned*>(cp + e) = cls;
      } else {
#pragma unroll
        for (int i = 0; i < V; ++i) cp[e + i] = (unsigned char)(cls >> (8 * i));
      }
    }
    w += sw;
    const int cw = w >= f.W;
    w -= cw ? f.W : 0;
    h += sh + cw;
    const int ch = h >= f.H;
    h -= ch ? f.H : 0;
    d += sd + ch;
  }
  // workgroup reduction: wave butterflies, then the four waves in a fixed order
  double v[K] = {(double)a.n, (double)a.nnf, (double)a.nout, (double)a.nocc, (double)a.nnoc, a.sr, a.sr2, a.mx,
                 a.srn, a.sa, a.se2, a.san, a.se2n};
#pragma unroll
  for (int k = 0; k < K; ++k) v[k] = (k == FS_FC_MAX_R) ? fs::wave_max(v[k]) : fs::wave_sum(v[k]);
  __shared__ double red[NT / 64][K];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < K; ++k) red[wv][k] = v[k];
  }
  __syncthreads();
  if (threadIdx.x < K) {
    const int k = threadIdx.x;
    const double r = (k == FS_FC_MAX_R) ? fmax(fmax(red[0][k], red[1][k]), fmax(red[2][k], red[3][k]))
                                        : (red[0][k] + red[1][k]) + (red[2][k] + red[3][k]);
    ws[((size_t)n * K + k) * f.G + b] = r;  // [N][K][G]: the second stage reads each statistic contiguously
  }
}

// Second stage: one workgroup per (pair n, statistic k) adds the G partials ws[n][k][0..G) in a fixed order -> out[n][k].
__global__ __launch_bounds__(NT) void flow_consistency_final_kernel(const double* __restrict__ ws, int G,
                                                                    double* __restrict__ out) {
  __shared__ double red[NT];
  const int k = blockIdx.x % K;
  const bool mx = k == FS_FC_MAX_R;
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

// Geometry of a call: FS_OK and f filled, or FS_ERR_*.
int plan(bool is3d, int N, int C, int D, int H, int W, long long fbs, long long bbs, CP& f, long long& blocks) {
  if (N < 1 || C != (is3d ? 3 : 2) || D < 1 || H < 1 || W < 1) return FS_ERR_SHAPE;
  const long long P = (long long)D * H * W;
  if (P > (1LL << 40) / C) return FS_ERR_SHAPE;
  if (N > 1 && (fbs < C * P || bbs < C * P)) return FS_ERR_SHAPE;
  f.P = P; f.fbs = fbs; f.bbs = bbs;
  f.D = D; f.H = H; f.W = W;
  long long G = (kTargetBlocks + N - 1) / N;
  const long long gmax = (P + NT - 1) / NT;  // groups at V = 1 (the workspace is sized for the larger grid)
  if (G > gmax) G = gmax;
  if (G < 1) G = 1;
  f.G = (int)G;
  blocks = (long long)N * G;
  if (blocks > kMaxBlocks) return FS_ERR_SHAPE;
  return FS_OK;
}

int launch(bool is3d, const float* flow_f, const float* flow_b, int N, int C, int D, int H, int W, long long fbs,
           long long bbs, const float* img0, const float* img1, const unsigned char* valid, double alpha1,
           double alpha2, unsigned char* cmap, float* rmap, double* ws, double* out, fs_stream_t stream) {
  FS_ENTER();
  FS_REQUIRE_PTR(flow_f); FS_REQUIRE_PTR(flow_b); FS_REQUIRE_PTR(ws); FS_REQUIRE_PTR(out);
  CP f;
  long long blocks = 0;
  const int rc = plan(is3d, N, C, D, H, W, fbs, bbs, f, blocks);
  if (rc != FS_OK) return rc;
  if (!(alpha1 >= 0.0 && alpha1 < HUGE_VAL && alpha2 >= 0.0 && alpha2 < HUGE_VAL)) return FS_ERR_ARG;
  if ((img0 == nullptr) != (img1 == nullptr)) return FS_ERR_ARG;
  f.a1 = alpha1; f.a2 = alpha2;
  // groups of 4 run along the flattened plane, so the plane size, not W, has to be a multiple of 4; the streamed
  // operands decide whether a group moves in one access (flow_b and img1 are gathered element by element)
  const bool g4 = f.P % 4 == 0;
  const bool vec = g4 && fbs % 4 == 0 && aligned(flow_f, 16) && aligned(img0, 16) && aligned(valid, 4) &&
                   aligned(cmap, 4) && aligned(rmap, 16);
  f.Q = f.P / (g4 ? 4 : 1);
  const bool img = img0 != nullptr;
  const hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)blocks), blk(NT);
#define FS_FC_LAUNCH(CC, VV, VE, II)                                                                              \
  hipLaunchKernelGGL((flow_consistency_kernel<CC, VV, VE, II>), grid, blk, 0, s, flow_f, flow_b, img0, img1, valid, \
                     cmap, rmap, ws, f)
#define FS_FC_LAUNCH_C(CC)                                                               \
  do {                                                                                   \
    if (vec) {                                                                           \
      if (img) FS_FC_LAUNCH(CC, 4, true, true); else FS_FC_LAUNCH(CC, 4, true, false);   \
    } else if (g4) {                                                                     \
      if (img) FS_FC_LAUNCH(CC, 4, false, true); else FS_FC_LAUNCH(CC, 4, false, false); \
    } else {                                                                             \
      if (img) FS_FC_LAUNCH(CC, 1, false, true); else FS_FC_LAUNCH(CC, 1, false, false); \
    }                                                                                    \
  } while (0)
  if (is3d) FS_FC_LAUNCH_C(3); else FS_FC_LAUNCH_C(2);
#undef FS_FC_LAUNCH_C
#undef FS_FC_LAUNCH
  hipLaunchKernelGGL(flow_consistency_final_kernel, dim3((unsigned)(N * K)), dim3(NT), 0, s, ws, f.G, out);
  FS_LAUNCH_CHECK();
  return FS_OK;
}

long long ws_bytes(bool is3d, int N, int C, int D, int H, int W) {
  CP f;
  long long blocks = 0;
  const long long P = (long long)D * H * W;
  const int rc = plan(is3d, N, C, D, H, W, (long long)C * P, (long long)C * P, f, blocks);
  if (rc != FS_OK) return -rc;
  return blocks * K * (long long)sizeof(double);
}

}  // namespace

extern "C" long long fs_flow_consistency2d_ws_bytes(int N, int C, int H, int W) {
  return ws_bytes(false, N, C, 1, H, W);
}

extern "C" long long fs_flow_consistency3d_ws_bytes(int N, int C, int D, int H, int W) {
  return ws_bytes(true, N, C, D, H, W);
}

extern "C" int fs_flow_consistency2d(const float* flow_f, const float* flow_b, int N, int C, int H, int W,
                                     long long f_bstride, long long b_bstride, const float* img0, const float* img1,
                                     const unsigned char* valid, double alpha1, double alpha2,
                                     unsigned char* class_map, float* res_map, double* ws, double* out,
                                     fs_stream_t stream) {
  return launch(false, flow_f, flow_b, N, C, 1, H, W, f_bstride, b_bstride, img0, img1, valid, alpha1, alpha2,
                class_map, res_map, ws, out, stream);
}

extern "C" int fs_flow_consistency3d(const float* flow_f, const float* flow_b, int N, int C, int D, int H, int W,
                                     long long f_bstride, long long b_bstride, const float* img0, const float* img1,
                                     const unsigned char* valid, double alpha1, double alpha2,
                                     unsigned char* class_map, float* res_map, double* ws, double* out,
                                     fs_stream_t stream) {
  return launch(true, flow_f, flow_b, N, C, D, H, W, f_bstride, b_bstride, img0, img1, valid, alpha1, alpha2,
                class_map, res_map, ws, out, stream);
}
