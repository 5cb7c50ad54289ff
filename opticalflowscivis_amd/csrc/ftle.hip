// ftle.hip -- finite-time Lyapunov exponents of a flow map sampled on a lattice (fs_ftle2d / fs_ftle3d): the map is
// differentiated by central or one-sided differences, the Cauchy-Green tensor G = J^T J is formed and reduced to
// ftle = ln(sqrt(lambda_max(G))) / |T|.  The map is what fs_advect* returns for lattice seeds, `status` its FS_ADV_*.
//
// Per node (fp64, contraction off up to and including G: a numpy fp64 restatement with the same operations in the same
// order reproduces every class and every bit of cg -- tests/ftle_ref.py):
//   usable(j): status[j] == ALIVE, or OUT when accept_out is set (the exit point stands for the end position)
//   axis c at index i, the first that applies: central, i-1 and i+1 exist and are usable (the node's own state does not
//     matter): (phi(i+1) - phi(i-1)) * inv_2h[c]; forward, i and i+1 usable: (phi(i+1) - phi(i)) * inv_h[c]; backward,
//     i and i-1 usable: (phi(i) - phi(i-1)) * inv_h[c]; none: the node is ENDED (axes are looked at in ascending c)
//     every map value is widened to fp64 before the subtraction; nothing is read from a node that is not usable
//   J[r][c] = the difference of component r along axis c; any J[r][c] not finite -> NONFINITE
//   G[a][b] = (J[0][a] J[0][b] + J[1][a] J[1][b]) + J[2][a] J[2][b]   (2-D: the first two terms)
//   lambda = the largest eigenvalue of G: 2-D 0.5 (a + c) + sqrt((0.5 (a - c))^2 + b^2); 3-D cyclic Jacobi (lmax3)
//   lambda == 0 -> COLLAPSED; e = (float)((0.5 * log(lambda)) * inv_T); e not finite -> NONFINITE; else OK
//
// One thread per node, x fastest: a wave reads and writes contiguous runs; the x neighbours are the wave's own lines and
// the y / z neighbours are rows the neighbouring waves stream, so they come from the cache (no LDS brick).  Nodes are
// taken in a grid-stride loop so that the workgroup reduction of the summary is paid once per thread, not per node:
// each workgroup writes its FS_FTLE_K partials to `ws` ([K][G]) and a second launch combines the G partials in a fixed
// order: no atomics, bitwise reproducible.
#include "common.hpp"
#include "jacobi3.hpp"

namespace {

constexpr int NT = 256;
constexpr int K = FS_FTLE_K;
constexpr long long kTargetBlocks = 2048;  // 8 workgroups per CU: the fp64 tail wants every wave slot

struct FP {
  long long mcs;       // component stride of map (elements)
  unsigned P;          // nodes
  unsigned W, H, D;    // lattice extents
  unsigned WH;
  int G;               // workgroups
  int accept_out;
  double ih[3], i2h[3], inv_T;
};

__device__ __forceinline__ bool usable(const unsigned char* __restrict__ st, size_t j, int accept_out) {
  const int s = st[j];
  return s == FS_ADV_ALIVE || (accept_out && s == FS_ADV_OUT);
}

// Largest eigenvalue of the symmetric positive semi-definite g = (xx, xy, yy, xz, yz, zz): cyclic Jacobi on the matrix
// scaled by a power of two (exact) to a trace in [0.5, 1), at most kSweeps sweeps, ended when the off-diagonal entries
// sum to less than 2^-45 (every eigenvalue then lies within that of a diagonal entry, and lambda_max >= trace / 3: a
// relative error below 2e-13).  A diagonal matrix returns its largest entry untouched; a zero matrix returns 0; a trace
// that is not finite comes back as it is.
constexpr int kSweeps = 10;
__device__ __forceinline__ double lmax3(const double (&g)[6]) {
  const double tr = (g[0] + g[2]) + g[5];
  if (!(tr > 0.0 && tr < HUGE_VAL)) return tr;
  int e;
  (void)frexp(tr, &e);
  e = e < -1000 ? -1000 : e;
  const double dn = ldexp(1.0, -e);
  double a00 = g[0] * dn, a01 = g[1] * dn, a11 = g[2] * dn, a02 = g[3] * dn, a12 = g[4] * dn, a22 = g[5] * dn;
  for (int sw = 0; sw < kSweeps; ++sw) {
    if (!((fabs(a01) + fabs(a02)) + fabs(a12) > 0x1p-45)) break;
    fs::jacobi_rotate(a00, a11, a01, a02, a12);
    fs::jacobi_rotate(a00, a22, a02, a01, a12);
    fs::jacobi_rotate(a11, a22, a12, a01, a02);
  }
  return ldexp(fmax(fmax(a00, a11), a22), e);
}

// One node: its class, G (defined for OK and COLLAPSED) and the fp32 exponent (defined for OK).
template <int C>
__device__ __forceinline__ int node(const float* __restrict__ map, const unsigned char* __restrict__ st, const FP& f,
                                    unsigned i, const unsigned (&x)[3], double (&g)[6], float& res) {
#pragma clang fp contract(off)
  const unsigned S[3] = {f.W, f.H, f.D}, step[3] = {1u, f.W, f.WH};
  const bool u0 = usable(st, i, f.accept_out);
  double J[3][3];
  bool fin = true;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    // i - step and i + step are formed only where they exist: every index below is a node of the lattice
    const bool um = x[c] > 0u && usable(st, (size_t)i - step[c], f.accept_out);
    const bool up = x[c] + 1u < S[c] && usable(st, (size_t)i + step[c], f.accept_out);
    size_t lo, hi;
    double w;
    if (um && up) {
      lo = (size_t)i - step[c]; hi = (size_t)i + step[c]; w = f.i2h[c];
    } else if (u0 && up) {
      lo = i; hi = (size_t)i + step[c]; w = f.ih[c];
    } else if (u0 && um) {
      lo = (size_t)i - step[c]; hi = i; w = f.ih[c];
    } else {
      return FS_FTLE_ENDED;
    }
#pragma unroll
    for (int r = 0; r < C; ++r) {
      const float* m = map + (size_t)r * f.mcs;
      J[r][c] = ((double)m[hi] - (double)m[lo]) * w;
      fin = fin && isfinite(J[r][c]);
    }
  }
  if (!fin) return FS_FTLE_NONFINITE;
  // plane order xx, xy, yy, xz, yz, zz
  const int A[6] = {0, 0, 1, 0, 1, 2}, B[6] = {0, 1, 1, 2, 2, 2};
#pragma unroll
  for (int n = 0; n < C * (C + 1) / 2; ++n) {
    const double s2 = J[0][A[n]] * J[0][B[n]] + J[1][A[n]] * J[1][B[n]];
    g[n] = C == 3 ? s2 + J[2][A[n]] * J[2][B[n]] : s2;
  }
  double lam;
  if (C == 3) {
    lam = lmax3(g);
  } else {
    const double hd = 0.5 * (g[0] - g[2]);
    lam = 0.5 * (g[0] + g[2]) + sqrt(hd * hd + g[1] * g[1]);
  }
  if (lam == 0.0) return FS_FTLE_COLLAPSED;
  res = (float)((0.5 * log(lam)) * f.inv_T);
  return isfinite(res) ? FS_FTLE_OK : FS_FTLE_NONFINITE;
}

template <int C>
__global__ __launch_bounds__(NT) void ftle_kernel(const float* __restrict__ map,
                                                  const unsigned char* __restrict__ status,
                                                  const unsigned char* __restrict__ valid, float* __restrict__ ftle,
                                                  unsigned char* __restrict__ cls, float* __restrict__ cg,
                                                  double* __restrict__ ws, FP f) {
  constexpr int NG = C * (C + 1) / 2;
  const float nanf_ = __builtin_nanf("");
  unsigned cnt[5] = {0u, 0u, 0u, 0u, 0u};
  double s1 = 0.0, s2 = 0.0, mn = HUGE_VAL, mx = -HUGE_VAL;
  const unsigned stride = (unsigned)f.G * NT;  // P < 2^31 and stride <= 2^19: q + stride does not wrap
  for (unsigned q = blockIdx.x * NT + threadIdx.x; q < f.P; q += stride) {
    const unsigned row = q / f.W, z = row / f.H;
    const unsigned x[3] = {q - row * f.W, row - z * f.H, z};
    int k = FS_FTLE_NOT_VALID;
    float res = nanf_;
    double g[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (!valid || valid[q] != 0) k = node<C>(map, status, f, q, x, g, res);
    const bool ok = k == FS_FTLE_OK;
    if (!ok) res = nanf_;
    ftle[q] = res;
    cls[q] = (unsigned char)k;
    if (cg) {
      const bool has = ok || k == FS_FTLE_COLLAPSED;
#pragma unroll
      for (int n = 0; n < NG; ++n) cg[(size_t)n * f.P + q] = has ? (float)g[n] : nanf_;
    }
#pragma unroll
    for (int j = 0; j < 5; ++j) cnt[j] += k == j ? 1u : 0u;
    if (ok) {
      const double v = (double)res;
      s1 += v; s2 += v * v; mn = fmin(mn, v); mx = fmax(mx, v);
    }
  }
  if (!ws) return;  // uniform: no summary asked for
  // workgroup reduction: wave butterflies, then the four waves in a fixed order
  double v[K] = {(double)cnt[0], (double)cnt[1], (double)cnt[2], (double)cnt[3], (double)cnt[4], s1, s2, mn, mx};
#pragma unroll
  for (int k = 0; k < K; ++k)
    v[k] = k == FS_FTLE_MIN ? fs::wave_min(v[k]) : k == FS_FTLE_MAX ? fs::wave_max(v[k]) : fs::wave_sum(v[k]);
  __shared__ double red[NT / 64][K];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < K; ++k) red[wv][k] = v[k];
  }
  __syncthreads();
  if (threadIdx.x < K) {
    const int k = threadIdx.x;
    const double r = k == FS_FTLE_MIN   ? fmin(fmin(red[0][k], red[1][k]), fmin(red[2][k], red[3][k]))
                     : k == FS_FTLE_MAX ? fmax(fmax(red[0][k], red[1][k]), fmax(red[2][k], red[3][k]))
                                        : (red[0][k] + red[1][k]) + (red[2][k] + red[3][k]);
    ws[(size_t)k * f.G + blockIdx.x] = r;  // [K][G]: the second stage reads each statistic contiguously
  }
}

// Second stage: one workgroup per statistic k combines the G partials ws[k][0..G) in a fixed order -> out[k].
__global__ __launch_bounds__(NT) void ftle_final_kernel(const double* __restrict__ ws, int G, double* __restrict__ out) {
  __shared__ double red[NT];
  const int k = blockIdx.x;
  const int op = k == FS_FTLE_MIN ? 1 : k == FS_FTLE_MAX ? 2 : 0;
  const double* w = ws + (size_t)k * G;
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
  if (threadIdx.x == 0) out[k] = red[0];
}

// Geometry of a call: FS_OK and f's extents and grid filled, or FS_ERR_SHAPE.
int plan(bool is3d, int C, int Gd, int Gh, int Gw, FP& f) {
  if (C != (is3d ? 3 : 2) || Gw < 2 || Gh < 2 || Gd < (is3d ? 2 : 1)) return FS_ERR_SHAPE;
  const long long P = (long long)Gd * Gh * Gw;
  if (P > 0x7fffffffLL) return FS_ERR_SHAPE;
  f.P = (unsigned)P;
  f.W = (unsigned)Gw; f.H = (unsigned)Gh; f.D = (unsigned)Gd;
  f.WH = (unsigned)((long long)Gw * Gh);
  const long long blocks = (P + NT - 1) / NT;
  f.G = (int)(blocks < kTargetBlocks ? blocks : kTargetBlocks);
  return FS_OK;
}

int launch(bool is3d, const float* map, long long mcs, const unsigned char* status, const unsigned char* valid, int C,
           int Gd, int Gh, int Gw, const double* inv_h, const double* inv_2h, double inv_T, int accept_out,
           float* ftle, unsigned char* cls, float* cg, double* ws, double* out, fs_stream_t stream) {
  FS_ENTER();
  FS_REQUIRE_PTR(map); FS_REQUIRE_PTR(status); FS_REQUIRE_PTR(inv_h); FS_REQUIRE_PTR(inv_2h);
  FS_REQUIRE_PTR(ftle); FS_REQUIRE_PTR(cls);
  if (out) FS_REQUIRE_PTR(ws);
  FP f;
  const int rc = plan(is3d, C, Gd, Gh, Gw, f);
  if (rc != FS_OK) return rc;
  if (mcs < (long long)f.P) return FS_ERR_SHAPE;
  if (!fs::pos_finite(inv_T)) return FS_ERR_ARG;
  for (int c = 0; c < 3; ++c) {
    f.ih[c] = c < C ? inv_h[c] : 0.0;
    f.i2h[c] = c < C ? inv_2h[c] : 0.0;
    if (c < C && !(fs::pos_finite(f.ih[c]) && fs::pos_finite(f.i2h[c]))) return FS_ERR_ARG;
  }
  f.mcs = mcs; f.inv_T = inv_T; f.accept_out = accept_out != 0;
  const hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)f.G), blk(NT);
  double* part = out ? ws : nullptr;
  if (is3d)
    hipLaunchKernelGGL((ftle_kernel<3>), grid, blk, 0, s, map, status, valid, ftle, cls, cg, part, f);
  else
    hipLaunchKernelGGL((ftle_kernel<2>), grid, blk, 0, s, map, status, valid, ftle, cls, cg, part, f);
  if (out) hipLaunchKernelGGL(ftle_final_kernel, dim3(K), dim3(NT), 0, s, ws, f.G, out);
  FS_LAUNCH_CHECK();
  return FS_OK;
}

long long ws_bytes(bool is3d, int C, int Gd, int Gh, int Gw) {
  FP f;
  const int rc = plan(is3d, C, Gd, Gh, Gw, f);
  if (rc != FS_OK) return -rc;
  return (long long)f.G * K * (long long)sizeof(double);
}

}  // namespace

extern "C" long long fs_ftle2d_ws_bytes(int C, int Gh, int Gw) { return ws_bytes(false, C, 1, Gh, Gw); }

extern "C" long long fs_ftle3d_ws_bytes(int C, int Gd, int Gh, int Gw) { return ws_bytes(true, C, Gd, Gh, Gw); }

extern "C" int fs_ftle2d(const float* map, long long map_cstride, const unsigned char* status,
                         const unsigned char* valid, int C, int Gh, int Gw, const double* inv_h, const double* inv_2h,
                         double inv_T, int accept_out, float* ftle, unsigned char* cls, float* cg, double* ws,
                         double* out, fs_stream_t stream) {
  return launch(false, map, map_cstride, status, valid, C, 1, Gh, Gw, inv_h, inv_2h, inv_T, accept_out, ftle, cls, cg,
                ws, out, stream);
}

extern "C" int fs_ftle3d(const float* map, long long map_cstride, const unsigned char* status,
                         const unsigned char* valid, int C, int Gd, int Gh, int Gw, const double* inv_h,
                         const double* inv_2h, double inv_T, int accept_out, float* ftle, unsigned char* cls, float* cg,
                         double* ws, double* out, fs_stream_t stream) {
  return launch(true, map, map_cstride, status, valid, C, Gd, Gh, Gw, inv_h, inv_2h, inv_T, accept_out, ftle, cls, cg,
                ws, out, stream);
}
