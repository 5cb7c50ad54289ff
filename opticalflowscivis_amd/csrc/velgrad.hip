// velgrad.hip -- the Eulerian quantities of K step flows (fs_velgrad2d / fs_velgrad3d): the velocity gradient J by
// central or one-sided differences, and from it divergence, vorticity and its magnitude, the Q criterion and lambda2
// (the median eigenvalue of S^2 + Omega^2), any subset, as fp32 planes with a flag map and a per-step summary.
// include/flowsci_hip.h states the arithmetic; everything up to and including M is fp64 with contraction off, so
// tests/velgrad_ref.py reproduces div, vort, q and J bit for bit.
//
// One thread per node, x fastest: a wave reads and writes contiguous runs; the x neighbours are the wave's own lines and
// the y / z neighbours are rows the neighbouring waves stream, so they come from the cache (no LDS brick).  blockIdx.y
// is the step: its scale is read from the launch's arguments by a uniform index.  Nodes are taken in a grid-stride loop
// so that the workgroup reduction of the summary is paid once per thread; each workgroup writes its FS_VG_K partials to
// `ws` ([K][FS_VG_K][G]) and a second launch combines the G partials in a fixed order: no atomics, bitwise
// reproducible, and step k's summary does not depend on K.  lambda2 is a template parameter: the kernels without it
// do not carry the Jacobi's registers.
#include "common.hpp"
#include "jacobi3.hpp"

namespace {

constexpr int NT = 256;
constexpr int NS = FS_VG_K;
constexpr int kSteps = FS_VG_STEPS_PER_LAUNCH;
constexpr long long kTargetBlocks = 2048;  // workgroups per step: 8 per CU

struct VP {
  long long sstride;   // step stride of flows (elements)
  unsigned P;          // nodes
  unsigned W, H, D;
  unsigned WH;
  int G;               // workgroups per step
  unsigned fields;
  int NP;              // planes per step
  int p_div, p_vort, p_vmag, p_q, p_l2, p_j;  // first plane of each field (unused when not selected)
  double ih[3], i2h[3];
  double scale[kSteps];
};

__device__ __forceinline__ double med3(double a, double b, double c) {
  return fmax(fmin(a, b), fmin(fmax(a, b), c));
}

// The median eigenvalue of the symmetric (indefinite) m = (00, 01, 11, 02, 12, 22): cyclic Jacobi on the matrix scaled
// by a power of two (exact) taken from its largest entry magnitude -- the trace can be zero or negative here -- at most
// kSweeps sweeps, ended when the off-diagonal entries sum to at most 2^-45 of that scale.  A diagonal matrix returns
// the median of its entries untouched; a zero matrix 0; a matrix with an entry that is not finite NaN.
constexpr int kSweeps = 10;
__device__ __forceinline__ double lmed3(const double (&m)[6]) {
  double mx = fmax(fmax(fabs(m[0]), fabs(m[1])), fmax(fabs(m[2]), fabs(m[3])));
  mx = fmax(mx, fmax(fabs(m[4]), fabs(m[5])));
  const bool fin = ((m[0] - m[0]) + (m[1] - m[1])) + ((m[2] - m[2]) + (m[3] - m[3])) + ((m[4] - m[4]) + (m[5] - m[5])) == 0.0;
  if (!fin) return __builtin_nan("");  // (fmax drops a NaN operand: the differences do not)
  if (mx == 0.0) return 0.0;
  int e;
  (void)frexp(mx, &e);
  e = e < -1000 ? -1000 : e;
  const double dn = ldexp(1.0, -e);
  double a00 = m[0] * dn, a01 = m[1] * dn, a11 = m[2] * dn, a02 = m[3] * dn, a12 = m[4] * dn, a22 = m[5] * dn;
  for (int sw = 0; sw < kSweeps; ++sw) {
    if (!((fabs(a01) + fabs(a02)) + fabs(a12) > 0x1p-45)) break;
    fs::jacobi_rotate(a00, a11, a01, a02, a12);
    fs::jacobi_rotate(a00, a22, a02, a01, a12);
    fs::jacobi_rotate(a11, a22, a12, a01, a02);
  }
  return ldexp(med3(a00, a11, a22), e);
}

// how statistic n of the summary combines: 0 sum, 1 minimum, 2 maximum
__host__ __device__ constexpr int stat_op(int n) { return n < 4 ? 0 : (n - 4) % 4 == 2 ? 1 : (n - 4) % 4 == 3 ? 2 : 0; }

// the fields statistic n depends on
__host__ __device__ constexpr unsigned stat_needs(int n) {
  return n == 0 ? 0u : n == 1 ? (unsigned)FS_VG_Q : n == 2 ? (unsigned)FS_VG_L2 : n == 3 ? (unsigned)(FS_VG_Q | FS_VG_L2)
       : (n - 4) / 4 == 0 ? (unsigned)FS_VG_DIV : (n - 4) / 4 == 1 ? (unsigned)FS_VG_VMAG
       : (n - 4) / 4 == 2 ? (unsigned)FS_VG_Q : (unsigned)FS_VG_L2;
}

struct Stat {
  double s1 = 0.0, s2 = 0.0, mn = HUGE_VAL, mx = -HUGE_VAL;
  __device__ __forceinline__ void add(float x) {
    const double v = (double)x;
    s1 += v; s2 += v * v; mn = fmin(mn, v); mx = fmax(mx, v);
  }
};

template <int C, bool L2>
__global__ __launch_bounds__(NT) void velgrad_kernel(const float* __restrict__ flows, float* __restrict__ out,
                                                     unsigned char* __restrict__ flags, double* __restrict__ ws,
                                                     const VP f) {
#pragma clang fp contract(off)
  const unsigned k = blockIdx.y;
  const float* __restrict__ u = flows + (size_t)k * f.sstride;
  float* __restrict__ o = out + (size_t)k * f.NP * f.P;
  unsigned char* __restrict__ fl = flags ? flags + (size_t)k * f.P : nullptr;
  const double sc = f.scale[k];
  const float nanf_ = __builtin_nanf("");
  const bool wdiv = f.fields & FS_VG_DIV, wvort = f.fields & FS_VG_VORT, wvmag = f.fields & FS_VG_VMAG;
  const bool wq = f.fields & FS_VG_Q, wj = f.fields & FS_VG_J;
  const unsigned S[3] = {f.W, f.H, f.D}, step[3] = {1u, f.W, f.WH};
  unsigned cnt[4] = {0u, 0u, 0u, 0u};
  Stat st[4];
  const unsigned stride = (unsigned)f.G * NT;  // P < 2^31 and stride <= 2^19: q + stride does not wrap
  for (unsigned q = blockIdx.x * NT + threadIdx.x; q < f.P; q += stride) {
    const unsigned row = q / f.W, z = row / f.H;
    const unsigned x[3] = {q - row * f.W, row - z * f.H, z};
    double J[3][3];
    bool fin = true;
#pragma unroll
    for (int c = 0; c < C; ++c) {
      // q - step and q + step are formed only where they exist: every index below is a node of the grid
      const bool hm = x[c] > 0u, hp = x[c] + 1u < S[c];
      const size_t lo = hm ? (size_t)q - step[c] : q, hi = hp ? (size_t)q + step[c] : q;
      const double w = hm && hp ? f.i2h[c] : f.ih[c];
#pragma unroll
      for (int r = 0; r < C; ++r) {
        const float* __restrict__ m = u + (size_t)r * f.P;
        J[r][c] = (((double)m[hi] - (double)m[lo]) * w) * sc;
        fin = fin && isfinite(J[r][c]);
      }
    }
    float vdiv = 0.f, vw[3] = {0.f, 0.f, 0.f}, vmag = 0.f, vq = 0.f, vl2 = 0.f;
    if (wdiv) {
      const double d = C == 3 ? (J[0][0] + J[1][1]) + J[2][2] : J[0][0] + J[1][1];
      vdiv = (float)d;
      fin = fin && isfinite(vdiv);
    }
    if (wvort || wvmag) {
      if (C == 3) {
        const double w0 = J[2][1] - J[1][2], w1 = J[0][2] - J[2][0], w2 = J[1][0] - J[0][1];
        vw[0] = (float)w0; vw[1] = (float)w1; vw[2] = (float)w2;
        vmag = (float)sqrt((w0 * w0 + w1 * w1) + w2 * w2);
        if (wvort) fin = fin && isfinite(vw[0]) && isfinite(vw[1]) && isfinite(vw[2]);
      } else {
        const double w0 = J[1][0] - J[0][1];
        vw[0] = (float)w0;
        vmag = (float)fabs(w0);
        if (wvort) fin = fin && isfinite(vw[0]);
      }
      if (wvmag) fin = fin && isfinite(vmag);
    }
    if (wq || L2) {
      if (C == 3) {
        const double s00 = J[0][0], s11 = J[1][1], s22 = J[2][2];
        const double s01 = 0.5 * (J[0][1] + J[1][0]), s02 = 0.5 * (J[0][2] + J[2][0]), s12 = 0.5 * (J[1][2] + J[2][1]);
        const double o01 = 0.5 * (J[0][1] - J[1][0]), o02 = 0.5 * (J[0][2] - J[2][0]), o12 = 0.5 * (J[1][2] - J[2][1]);
        if (wq) {
          const double nS = ((s00 * s00 + s11 * s11) + s22 * s22) + 2.0 * ((s01 * s01 + s02 * s02) + s12 * s12);
          const double nO = 2.0 * ((o01 * o01 + o02 * o02) + o12 * o12);
          vq = (float)(0.5 * (nO - nS));
          fin = fin && isfinite(vq);
        }
        if (L2) {
          const double m[6] = {((s00 * s00 + s01 * s01) + s02 * s02) - (o01 * o01 + o02 * o02),
                               ((s00 * s01 + s01 * s11) + s02 * s12) - o02 * o12,
                               ((s01 * s01 + s11 * s11) + s12 * s12) - (o01 * o01 + o12 * o12),
                               ((s00 * s02 + s01 * s12) + s02 * s22) + o01 * o12,
                               ((s01 * s02 + s11 * s12) + s12 * s22) - o01 * o02,
                               ((s02 * s02 + s12 * s12) + s22 * s22) - (o02 * o02 + o12 * o12)};
          vl2 = (float)lmed3(m);
          fin = fin && isfinite(vl2);
        }
      } else {
        const double s00 = J[0][0], s11 = J[1][1];
        const double s01 = 0.5 * (J[0][1] + J[1][0]), o01 = 0.5 * (J[0][1] - J[1][0]);
        if (wq) {
          const double nS = (s00 * s00 + s11 * s11) + 2.0 * (s01 * s01);
          const double nO = 2.0 * (o01 * o01);
          vq = (float)(0.5 * (nO - nS));
          fin = fin && isfinite(vq);
        }
        if (L2) {
          const double m00 = (s00 * s00 + s01 * s01) - o01 * o01, m11 = (s01 * s01 + s11 * s11) - o01 * o01;
          const double m01 = s00 * s01 + s01 * s11;
          const double hm = 0.5 * (m00 + m11), hd = 0.5 * (m00 - m11);
          const double rad = sqrt(hd * hd + m01 * m01);
          vl2 = (float)med3(hm - rad, hm + rad, 0.0);
          fin = fin && isfinite(vl2);
        }
      }
    }
    if (wj) {
#pragma unroll
      for (int r = 0; r < C; ++r)
#pragma unroll
        for (int c = 0; c < C; ++c) fin = fin && isfinite((float)J[r][c]);
    }
    // stores: plane p of this step at o + p * P
    if (wdiv) o[(size_t)f.p_div * f.P + q] = fin ? vdiv : nanf_;
    if (wvort) {
#pragma unroll
      for (int n = 0; n < (C == 3 ? 3 : 1); ++n) o[(size_t)(f.p_vort + n) * f.P + q] = fin ? vw[n] : nanf_;
    }
    if (wvmag) o[(size_t)f.p_vmag * f.P + q] = fin ? vmag : nanf_;
    if (wq) o[(size_t)f.p_q * f.P + q] = fin ? vq : nanf_;
    if (L2) o[(size_t)f.p_l2 * f.P + q] = fin ? vl2 : nanf_;
    if (wj) {
#pragma unroll
      for (int r = 0; r < C; ++r)
#pragma unroll
        for (int c = 0; c < C; ++c) o[(size_t)(f.p_j + r * C + c) * f.P + q] = fin ? (float)J[r][c] : nanf_;
    }
    const bool bq = fin && wq && vq > 0.f, bl = fin && L2 && vl2 < 0.f;
    if (fl) fl[q] = (unsigned char)(fin ? (bq ? FS_VG_FLAG_Q : 0) | (bl ? FS_VG_FLAG_L2 : 0) : FS_VG_FLAG_NONFINITE);
    if (ws) {  // uniform
      cnt[0] += fin ? 0u : 1u; cnt[1] += bq ? 1u : 0u; cnt[2] += bl ? 1u : 0u; cnt[3] += bq && bl ? 1u : 0u;
      if (fin) {
        if (wdiv) st[0].add(vdiv);
        if (wvmag) st[1].add(vmag);
        if (wq) st[2].add(vq);
        if (L2) st[3].add(vl2);
      }
    }
  }
  if (!ws) return;  // uniform: no summary asked for
  // workgroup reduction: wave butterflies, then the four waves in a fixed order
  double v[NS];
#pragma unroll
  for (int n = 0; n < 4; ++n) {
    v[n] = (double)cnt[n];
    v[4 + 4 * n] = st[n].s1; v[5 + 4 * n] = st[n].s2; v[6 + 4 * n] = st[n].mn; v[7 + 4 * n] = st[n].mx;
  }
#pragma unroll
  for (int n = 0; n < NS; ++n)
    v[n] = stat_op(n) == 1 ? fs::wave_min(v[n]) : stat_op(n) == 2 ? fs::wave_max(v[n]) : fs::wave_sum(v[n]);
  __shared__ double red[NT / 64][NS];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if (lane == 0) {
#pragma unroll
    for (int n = 0; n < NS; ++n) red[wv][n] = v[n];
  }
  __syncthreads();
  if (threadIdx.x < NS) {
    const int n = threadIdx.x;
    const int op = stat_op(n);
    const double r = op == 1   ? fmin(fmin(red[0][n], red[1][n]), fmin(red[2][n], red[3][n]))
                     : op == 2 ? fmax(fmax(red[0][n], red[1][n]), fmax(red[2][n], red[3][n]))
                               : (red[0][n] + red[1][n]) + (red[2][n] + red[3][n]);
    ws[((size_t)k * NS + n) * f.G + blockIdx.x] = r;  // [K][NS][G]: the second stage reads each statistic contiguously
  }
}

// Second stage: workgroup (n, k) combines the G partials ws[k][n][0..G) in a fixed order -> summary[k][n]; NaN where
// the statistic depends on a field that was not selected.
__global__ __launch_bounds__(NT) void velgrad_final_kernel(const double* __restrict__ ws, int G, unsigned fields,
                                                           double* __restrict__ summary) {
  __shared__ double red[NT];
  const int n = blockIdx.x;
  const size_t kn = (size_t)blockIdx.y * NS + n;
  const int op = stat_op(n);
  const double* w = ws + kn * G;
  double s = op == 1 ? HUGE_VAL : op == 2 ? -HUGE_VAL : 0.0;
  for (int i = threadIdx.x; i < G; i += NT) s = op == 1 ? fmin(s, w[i]) : op == 2 ? fmax(s, w[i]) : s + w[i];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int t = NT / 2; t > 0; t >>= 1) {
    if ((int)threadIdx.x < t) {
      const double a = red[threadIdx.x], b = red[threadIdx.x + t];
      red[threadIdx.x] = op == 1 ? fmin(a, b) : op == 2 ? fmax(a, b) : a + b;
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) summary[kn] = (fields & stat_needs(n)) == stat_needs(n) ? red[0] : __builtin_nan("");
}

// Geometry of a call: FS_OK and f's extents and grid filled, or FS_ERR_SHAPE.
int plan(bool is3d, int C, int D, int H, int W, VP& f) {
  if (C != (is3d ? 3 : 2) || W < 2 || H < 2 || D < (is3d ? 2 : 1)) return FS_ERR_SHAPE;
  const long long P = (long long)D * H * W;
  if (P > 0x7fffffffLL) return FS_ERR_SHAPE;
  f.P = (unsigned)P;
  f.W = (unsigned)W; f.H = (unsigned)H; f.D = (unsigned)D;
  f.WH = (unsigned)((long long)W * H);
  const long long blocks = (P + NT - 1) / NT;
  f.G = (int)(blocks < kTargetBlocks ? blocks : kTargetBlocks);
  return FS_OK;
}

template <int C>
void launch_main(bool l2, dim3 grid, hipStream_t s, const float* flows, float* out, unsigned char* flags, double* ws,
                 const VP& f) {
  if (l2)
    hipLaunchKernelGGL((velgrad_kernel<C, true>), grid, dim3(NT), 0, s, flows, out, flags, ws, f);
  else
    hipLaunchKernelGGL((velgrad_kernel<C, false>), grid, dim3(NT), 0, s, flows, out, flags, ws, f);
}

int launch(bool is3d, const float* flows, int K, int C, int D, int H, int W, long long sstride, const double* inv_h,
           const double* inv_2h, const double* scale, unsigned fields, float* out, unsigned char* flags, double* ws,
           double* summary, fs_stream_t stream) {
  FS_ENTER();
  FS_REQUIRE_PTR(flows); FS_REQUIRE_PTR(inv_h); FS_REQUIRE_PTR(inv_2h); FS_REQUIRE_PTR(scale); FS_REQUIRE_PTR(out);
  if (summary) FS_REQUIRE_PTR(ws);
  VP f;
  const int rc = plan(is3d, C, D, H, W, f);
  if (rc != FS_OK) return rc;
  if (sstride < (long long)C * f.P) return FS_ERR_SHAPE;
  if (fields == 0u || (fields & ~(unsigned)FS_VG_ALL) != 0u || K < 1) return FS_ERR_ARG;
  for (int c = 0; c < 3; ++c) {
    f.ih[c] = c < C ? inv_h[c] : 0.0;
    f.i2h[c] = c < C ? inv_2h[c] : 0.0;
    if (c < C && !(fs::pos_finite(f.ih[c]) && fs::pos_finite(f.i2h[c]))) return FS_ERR_ARG;
  }
  for (int k = 0; k < K; ++k)
    if (!fs::pos_finite(scale[k])) return FS_ERR_ARG;
  f.sstride = sstride;
  f.fields = fields;
  int np = 0;
  f.p_div = np; np += fields & FS_VG_DIV ? 1 : 0;
  f.p_vort = np; np += fields & FS_VG_VORT ? (is3d ? 3 : 1) : 0;
  f.p_vmag = np; np += fields & FS_VG_VMAG ? 1 : 0;
  f.p_q = np; np += fields & FS_VG_Q ? 1 : 0;
  f.p_l2 = np; np += fields & FS_VG_L2 ? 1 : 0;
  f.p_j = np; np += fields & FS_VG_J ? C * C : 0;
  f.NP = np;
  const hipStream_t s = (hipStream_t)stream;
  const bool l2 = (fields & FS_VG_L2) != 0u;
  double* part = summary ? ws : nullptr;
  for (int k0 = 0; k0 < K; k0 += kSteps) {
    const int kc = K - k0 < kSteps ? K - k0 : kSteps;
    for (int k = 0; k < kSteps; ++k) f.scale[k] = k < kc ? scale[k0 + k] : 0.0;
    const dim3 grid((unsigned)f.G, (unsigned)kc);
    const float* fk = flows + (size_t)k0 * sstride;
    float* ok = out + (size_t)k0 * np * f.P;
    unsigned char* gk = flags ? flags + (size_t)k0 * f.P : nullptr;
    double* wk = part ? part + (size_t)k0 * NS * f.G : nullptr;
    if (is3d)
      launch_main<3>(l2, grid, s, fk, ok, gk, wk, f);
    else
      launch_main<2>(l2, grid, s, fk, ok, gk, wk, f);
    if (summary)
      hipLaunchKernelGGL(velgrad_final_kernel, dim3(NS, (unsigned)kc), dim3(NT), 0, s, wk, f.G, fields,
                         summary + (size_t)k0 * NS);
  }
  FS_LAUNCH_CHECK();
  return FS_OK;
}

long long ws_bytes(bool is3d, int K, int C, int D, int H, int W) {
  VP f;
  const int rc = plan(is3d, C, D, H, W, f);
  if (rc != FS_OK) return -rc;
  if (K < 1) return -FS_ERR_ARG;
  return (long long)K * NS * f.G * (long long)sizeof(double);
}

}  // namespace

extern "C" long long fs_velgrad2d_ws_bytes(int K, int C, int H, int W) { return ws_bytes(false, K, C, 1, H, W); }

extern "C" long long fs_velgrad3d_ws_bytes(int K, int C, int D, int H, int W) { return ws_bytes(true, K, C, D, H, W); }

extern "C" int fs_velgrad2d(const float* flows, int K, int C, int H, int W, long long flow_sstride, const double* inv_h,
                            const double* inv_2h, const double* scale, unsigned fields, float* out,
                            unsigned char* flags, double* ws, double* summary, fs_stream_t stream) {
  return launch(false, flows, K, C, 1, H, W, flow_sstride, inv_h, inv_2h, scale, fields, out, flags, ws, summary, stream);
}

extern "C" int fs_velgrad3d(const float* flows, int K, int C, int D, int H, int W, long long flow_sstride,
                            const double* inv_h, const double* inv_2h, const double* scale, unsigned fields, float* out,
                            unsigned char* flags, double* ws, double* summary, fs_stream_t stream) {
  return launch(true, flows, K, C, D, H, W, flow_sstride, inv_h, inv_2h, scale, fields, out, flags, ws, summary, stream);
}
