// raycast.hip -- K volumes through K cameras and one transfer function to K RGBA images (fs_raycast3d: emission /
// absorption or maximum intensity), and the per-brick value ranges (fs_brick_range3d) that let a ray jump over bricks
// which cannot contribute.  include/flowsci_hip.h states the arithmetic; tests/raycast_ref.py restates it.
//
// One pixel per lane, 8 x 8 pixel tiles per wave, 2 x 2 tiles per workgroup, blockIdx.z the frame: the rays of a wave
// stay within a few cells of each other, so each of the eight corner gathers of a step lands in a handful of
// neighbouring lines.  The table and the frame's camera are staged in LDS once per workgroup.  A ray's samples lie at
// (k + 1/2) dt from its origin whatever the box: the slab test only bounds k, and a sample outside the box weighs
// exactly 0 (coverage), so neither the bound nor a jump changes a bit of the image.  Sample positions are formed without
// fused multiply-adds: the cell a sample falls in is the restatement's, bit for bit.  No atomics, no scratch.
#include "common.hpp"

namespace {

constexpr int NT = 256;
constexpr int kTile = 16;           // a workgroup's pixels: 2 x 2 wave tiles of 8 x 8
constexpr int kBrick = FS_RC_BRICK;  // cells per brick and axis
constexpr float kMaxK = 16777215.f;  // sample indices stay exact in fp32

struct RP {
  const float* vol;
  long long sstride;
  const float* cams;
  const float* tf;
  const unsigned char* skip;  // [K][nbz][nby][nbx]: 1 = nothing in this brick can contribute
  float* img;
  int* counts;
  int N[3];   // W, H, D
  int nb[3];  // bricks along x, y, z
  int Hi, Wi, n;
  float ih[3];  // 1 / spacing along x, y, z
  float lo, inv_range, dt, inv_dt, t_min;
};

struct Ray {
  float o[3], d[3];
};

// origin and unit direction of pixel (i, j) of camera c = (o, ou, ov, d, du, dv)
__device__ __forceinline__ Ray make_ray(const float* c, float fi, float fj) {
#pragma clang fp contract(off)
  Ray r;
  float g[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    r.o[a] = (c[a] + fi * c[3 + a]) + fj * c[6 + a];
    g[a] = (c[9 + a] + fi * c[12 + a]) + fj * c[15 + a];
  }
  const float len = sqrtf((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]);
#pragma unroll
  for (int a = 0; a < 3; ++a) r.d[a] = g[a] / len;
  return r;
}

// index position of sample k
__device__ __forceinline__ void sample_q(const Ray& r, const float (&ih)[3], float dt, int k, float (&q)[3]) {
#pragma clang fp contract(off)
  const float t = ((float)k + 0.5f) * dt;
#pragma unroll
  for (int a = 0; a < 3; ++a) q[a] = (r.o[a] + t * r.d[a]) * ih[a];
}

// The row of the table at u in [0, 1].  Here and in the kernel the compiler fuses nothing on its own: the fused
// multiply-adds are written out, so that every instantiation of the kernel rounds alike (the image with the brick map
// must equal the image without it bit for bit).
__device__ __forceinline__ float4 table_at(const float4* tf, int n, float u) {
#pragma clang fp contract(off)
  const float s = u * (float)(n - 1);
  int j = (int)s;
  j = j < n - 2 ? j : n - 2;
  const float ft = s - (float)j;
  const float4 a = tf[j], b = tf[j + 1];
  return make_float4(fmaf(ft, b.x - a.x, a.x), fmaf(ft, b.y - a.y, a.y), fmaf(ft, b.z - a.z, a.z), fmaf(ft, b.w - a.w, a.w));
}

template <int MODE, bool SKIP>
__global__ __launch_bounds__(NT) void raycast_kernel(const RP f) {
#pragma clang fp contract(off)
  __shared__ float4 s_tf[FS_RC_MAX_TF];
  __shared__ float s_cam[18];
  const unsigned frame = blockIdx.z;
  for (int i = threadIdx.x; i < f.n; i += NT) s_tf[i] = reinterpret_cast<const float4*>(f.tf)[i];
  if (threadIdx.x < 18) s_cam[threadIdx.x] = f.cams[(size_t)frame * 18 + threadIdx.x];
  __syncthreads();
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int px = (int)blockIdx.x * kTile + (wv & 1) * 8 + (lane & 7);
  const int py = (int)blockIdx.y * kTile + (wv >> 1) * 8 + (lane >> 3);
  if (px >= f.Wi || py >= f.Hi) return;
  const float* __restrict__ vol = f.vol + (size_t)frame * f.sstride;
  const unsigned char* __restrict__ skip = SKIP ? f.skip + (size_t)frame * f.nb[0] * f.nb[1] * f.nb[2] : nullptr;
  const Ray r = make_ray(s_cam, (float)px, (float)py);

  // The k range: a sample weighs more than 0 only inside (-1, N) per axis in index units; the slab is widened by del,
  // far more than the sample positions' rounding, and by one sample at either end.
  float q0[3], dq[3], rdq[3], del[3];
  float tn = 0.f, tfar = kMaxK * f.dt;
  bool hit = true;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    q0[a] = r.o[a] * f.ih[a];
    dq[a] = r.d[a] * f.ih[a];
    hit = hit && isfinite(q0[a]) && isfinite(dq[a]);
    del[a] = 0x1p-15f * (fabsf(q0[a]) + (float)(f.N[a] + 1));
    const float lo_a = -1.f - del[a], hi_a = (float)f.N[a] + del[a];
    if (dq[a] != 0.f) {
      rdq[a] = 1.f / dq[a];
      const float t1 = (lo_a - q0[a]) * rdq[a], t2 = (hi_a - q0[a]) * rdq[a];
      tn = fmaxf(tn, fminf(t1, t2));
      tfar = fminf(tfar, fmaxf(t1, t2));
    } else {
      rdq[a] = 0.f;
      hit = hit && q0[a] > lo_a && q0[a] < hi_a;
    }
  }
  hit = hit && tn <= tfar;
  int k = 0, k1 = -1;
  if (hit) {
    k = (int)fminf(fmaxf(floorf(tn * f.inv_dt - 0.5f) - 1.f, 0.f), kMaxK);
    k1 = (int)fminf(fmaxf(ceilf(tfar * f.inv_dt - 0.5f) + 1.f, -1.f), kMaxK);
  }

  float cr = 0.f, cg = 0.f, cb = 0.f, T = 1.f, m = 0.f;
  int cnt = 0;
  int kchk = k;  // the next sample at which the brick is looked up
  const float N1[3] = {(float)(f.N[0] - 1), (float)(f.N[1] - 1), (float)(f.N[2] - 1)};
  while (k <= k1) {
    float q[3];
    sample_q(r, f.ih, f.dt, k, q);
    int i0[3];
    float fr[3], c = 1.f;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const float out = fmaxf(0.f, fmaxf(-q[a], q[a] - N1[a]));
      c *= fmaxf(0.f, 1.f - out);
      const float qc = fminf(fmaxf(q[a], 0.f), N1[a]);  // in [0, N - 1] whatever q is
      const int i = (int)qc;
      i0[a] = i < f.N[a] - 2 ? i : f.N[a] - 2;
      fr[a] = qc - (float)i0[a];
    }
    if (SKIP && k >= kchk) {
      // The brick of this sample's cell, and the last sample the ray provably spends in it: the faces it leaves through
      // are pulled in by del, a jump lands on that sample (early, never late).  The first and last brick of an axis
      // also own everything the clamp sends there.
      float te = kMaxK * f.dt;
      int b[3];
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        b[a] = i0[a] / kBrick;
        if (dq[a] > 0.f && b[a] < f.nb[a] - 1) te = fminf(te, ((float)(kBrick * (b[a] + 1)) - del[a] - q0[a]) * rdq[a]);
        if (dq[a] < 0.f && b[a] > 0) te = fminf(te, ((float)(kBrick * b[a]) + del[a] - q0[a]) * rdq[a]);
      }
      const int ke = (int)fminf(fmaxf(floorf(te * f.inv_dt - 0.5f), 0.f), kMaxK);
      const int kn = ke > k + 1 ? ke : k + 1;
      if (skip[((size_t)b[2] * f.nb[1] + b[1]) * f.nb[0] + b[0]]) {
        k = kn;
        continue;
      }
      kchk = kn;
    }
    // i0 <= N - 2 on every axis: all eight corners are nodes of the volume
    const float* __restrict__ p = vol + ((size_t)i0[2] * f.N[1] + i0[1]) * f.N[0] + i0[0];
    const size_t sy = (size_t)f.N[0], sz = (size_t)f.N[0] * f.N[1];
    const float a000 = p[0], a001 = p[1], a010 = p[sy], a011 = p[sy + 1];
    const float a100 = p[sz], a101 = p[sz + 1], a110 = p[sz + sy], a111 = p[sz + sy + 1];
    const float v00 = fmaf(fr[0], a001 - a000, a000), v01 = fmaf(fr[0], a011 - a010, a010);
    const float v10 = fmaf(fr[0], a101 - a100, a100), v11 = fmaf(fr[0], a111 - a110, a110);
    const float v0 = fmaf(fr[1], v01 - v00, v00), v1 = fmaf(fr[1], v11 - v10, v10);
    const float v = fmaf(fr[2], v1 - v0, v0);
    ++cnt;
    ++k;
    if (!isfinite(v)) continue;
    const float u = fminf(fmaxf((v - f.lo) * f.inv_range, 0.f), 1.f);
    if (MODE == FS_RC_MIP) {
      m = fmaxf(m, c * u);
    } else {
      const float4 s = table_at(s_tf, f.n, u);
      const float e = expf(-((s.w * c) * f.dt));
      const float w = T * (1.f - e);
      cr = fmaf(w, s.x, cr);
      cg = fmaf(w, s.y, cg);
      cb = fmaf(w, s.z, cb);
      T *= e;
      if (T < f.t_min) break;
    }
  }
  const size_t pix = ((size_t)frame * f.Hi + py) * f.Wi + px;
  reinterpret_cast<float4*>(f.img)[pix] = MODE == FS_RC_MIP ? table_at(s_tf, f.n, m) : make_float4(cr, cg, cb, 1.f - T);
  if (f.counts) f.counts[pix] = cnt;
}

// One wave per brick: minimum and maximum over the finite ones of its up to 9^3 nodes, and whether any is not finite.
__global__ __launch_bounds__(64) void brick_range_kernel(const float* __restrict__ vols, long long sstride, int W, int H,
                                                         int D, int nbx, int nby, int nbz, float* __restrict__ range,
                                                         unsigned char* __restrict__ nonfinite) {
  const unsigned brick = blockIdx.x, frame = blockIdx.y;
  const int bx = brick % nbx, by = (brick / nbx) % nby, bz = brick / (nbx * nby);
  const float* __restrict__ vol = vols + (size_t)frame * sstride;
  const int x0 = bx * kBrick, y0 = by * kBrick, z0 = bz * kBrick;
  const int ex = min(kBrick + 1, W - x0), ey = min(kBrick + 1, H - y0), ez = min(kBrick + 1, D - z0);
  float mn = HUGE_VALF, mx = -HUGE_VALF;
  int bad = 0;
  for (int i = threadIdx.x; i < ex * ey * ez; i += 64) {
    const int x = i % ex, y = (i / ex) % ey, z = i / (ex * ey);
    const float v = vol[((size_t)(z0 + z) * H + (y0 + y)) * W + (x0 + x)];
    if (isfinite(v)) {
      mn = fminf(mn, v);
      mx = fmaxf(mx, v);
    } else {
      bad = 1;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    mn = fminf(mn, __shfl_xor(mn, o, 64));
    mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    bad |= __shfl_xor(bad, o, 64);
  }
  if (threadIdx.x == 0) {
    const size_t at = (size_t)frame * nbx * nby * nbz + brick;
    range[2 * at] = mn;
    range[2 * at + 1] = mx;
    nonfinite[at] = (unsigned char)bad;
  }
}

// One thread per brick: may a ray jump over it?  Three nested fp32 interpolations of values in [mn, mx] stay within
// 2^-20 of the larger magnitude of that range (each adds at most a few 2^-24 of it): the test is made on the range
// widened by that much, and in dvr on one table entry more at either end than the widened range touches.
__global__ __launch_bounds__(NT) void brick_skip_kernel(const float* __restrict__ range,
                                                        const unsigned char* __restrict__ nonfinite, size_t total,
                                                        const float* __restrict__ tf, int n, float lo, float inv_range,
                                                        int mode, unsigned char* __restrict__ skip) {
  const size_t at = (size_t)blockIdx.x * NT + threadIdx.x;
  if (at >= total) return;
  const float mn = range[2 * at], mx = range[2 * at + 1];
  bool s = false;
  if (!nonfinite[at] && mn <= mx) {
    const float big = fmaxf(fabsf(mn), fabsf(mx));
    const float wd = big > 0.f ? 0x1p-20f * big + 0x1p-126f : 0.f;  // (a brick of zeros interpolates to exactly 0)
    const float a = mn - wd, b = mx + wd;
    if (mode == FS_RC_MIP) {
      s = b <= lo;
    } else {
      const double ua = fmin(fmax(((double)a - (double)lo) * (double)inv_range, 0.0), 1.0);
      const double ub = fmin(fmax(((double)b - (double)lo) * (double)inv_range, 0.0), 1.0);
      int j0 = (int)floor(ua * (n - 1)) - 1, j1 = (int)ceil(ub * (n - 1)) + 1;
      j0 = j0 < 0 ? 0 : j0;
      j1 = j1 > n - 1 ? n - 1 : j1;
      s = true;
      for (int j = j0; j <= j1 && s; ++j) s = tf[4 * j + 3] == 0.f;
    }
  }
  skip[at] = s ? 1 : 0;
}

inline int nbricks(int n) { return (n - 1 + kBrick - 1) / kBrick; }

// FS_OK, or what is wrong with the volumes' geometry
int check_volumes(int K, int D, int H, int W, long long sstride) {
  if (K < 1 || K > 65535 || D < 2 || H < 2 || W < 2) return FS_ERR_SHAPE;
  const long long P = (long long)D * H * W;
  if (P > 0x7fffffffLL || sstride < P) return FS_ERR_SHAPE;
  return FS_OK;
}

template <int MODE>
void launch_ray(bool with_skip, dim3 grid, hipStream_t s, const RP& f) {
  if (with_skip)
    hipLaunchKernelGGL((raycast_kernel<MODE, true>), grid, dim3(NT), 0, s, f);
  else
    hipLaunchKernelGGL((raycast_kernel<MODE, false>), grid, dim3(NT), 0, s, f);
}

}  // namespace

extern "C" int fs_brick_range3d(const float* volumes, int K, int D, int H, int W, long long sstride, float* range,
                                unsigned char* nonfinite, fs_stream_t stream) {
  FS_ENTER();
  FS_REQUIRE_PTR(volumes); FS_REQUIRE_PTR(range); FS_REQUIRE_PTR(nonfinite);
  const int rc = check_volumes(K, D, H, W, sstride);
  if (rc != FS_OK) return rc;
  const int nbx = nbricks(W), nby = nbricks(H), nbz = nbricks(D);
  hipLaunchKernelGGL(brick_range_kernel, dim3((unsigned)(nbx * nby * nbz), (unsigned)K), dim3(64), 0,
                     (hipStream_t)stream, volumes, sstride, W, H, D, nbx, nby, nbz, range, nonfinite);
  FS_LAUNCH_CHECK();
  return FS_OK;
}

extern "C" long long fs_raycast3d_ws_bytes(int K, int D, int H, int W) {
  const int rc = check_volumes(K, D, H, W, (long long)D * H * W);
  if (rc != FS_OK) return -rc;
  return (long long)K * nbricks(W) * nbricks(H) * nbricks(D);
}

extern "C" int fs_raycast3d(const float* volumes, int K, int D, int H, int W, long long sstride, const float* cameras,
                            const float* tf, int n, double lo, double hi, double dt, const double* spacing, int mode,
                            double t_min, int Hi, int Wi, const float* brick_range,
                            const unsigned char* brick_nonfinite, unsigned char* ws, float* image, int* counts,
                            fs_stream_t stream) {
  FS_ENTER();
  FS_REQUIRE_PTR(volumes); FS_REQUIRE_PTR(cameras); FS_REQUIRE_PTR(tf); FS_REQUIRE_PTR(spacing); FS_REQUIRE_PTR(image);
  if (brick_range) { FS_REQUIRE_PTR(brick_nonfinite); FS_REQUIRE_PTR(ws); }
  const int rc = check_volumes(K, D, H, W, sstride);
  if (rc != FS_OK) return rc;
  if (Hi < 1 || Wi < 1 || Hi > 65535 * kTile || Wi > 65535 * kTile) return FS_ERR_SHAPE;
  if (n < 2 || n > FS_RC_MAX_TF) return FS_ERR_SHAPE;
  if (mode != FS_RC_DVR && mode != FS_RC_MIP) return FS_ERR_ARG;
  if (!(lo < hi) || !(lo > -HUGE_VAL) || !(hi < HUGE_VAL) || !fs::pos_finite(dt) || !(t_min >= 0.0 && t_min < 1.0))
    return FS_ERR_ARG;
  if (((uintptr_t)tf | (uintptr_t)image) & 15u) return FS_ERR_ARG;
  RP f;
  const int N[3] = {W, H, D};
  double reach = 0.0;
  for (int a = 0; a < 3; ++a) {
    if (!fs::pos_finite(spacing[a])) return FS_ERR_ARG;
    f.N[a] = N[a];
    f.nb[a] = nbricks(N[a]);
    f.ih[a] = (float)(1.0 / spacing[a]);
    reach += (N[a] + 1) * spacing[a];
  }
  const float inv_range = (float)(1.0 / (hi - lo));
  // (what is finite and positive in fp64 must still be so in fp32)
  if (!(reach / dt <= (double)FS_RC_MAX_STEPS) || !fs::pos_finite((float)dt) || !fs::pos_finite(f.ih[0]) ||
      !fs::pos_finite(f.ih[1]) || !fs::pos_finite(f.ih[2]) || !fs::pos_finite(inv_range) ||
      !fs::pos_finite((float)(1.0 / dt)))
    return FS_ERR_ARG;
  f.vol = volumes; f.sstride = sstride; f.cams = cameras; f.tf = tf; f.skip = brick_range ? ws : nullptr;
  f.img = image; f.counts = counts;
  f.Hi = Hi; f.Wi = Wi; f.n = n;
  f.lo = (float)lo; f.inv_range = inv_range;
  f.dt = (float)dt; f.inv_dt = (float)(1.0 / dt); f.t_min = (float)t_min;
  const hipStream_t s = (hipStream_t)stream;
  if (brick_range) {
    const size_t total = (size_t)K * f.nb[0] * f.nb[1] * f.nb[2];
    hipLaunchKernelGGL(brick_skip_kernel, dim3((unsigned)((total + NT - 1) / NT)), dim3(NT), 0, s, brick_range,
                       brick_nonfinite, total, tf, n, f.lo, f.inv_range, mode, ws);
  }
  const dim3 grid((unsigned)((Wi + kTile - 1) / kTile), (unsigned)((Hi + kTile - 1) / kTile), (unsigned)K);
  if (mode == FS_RC_MIP)
    launch_ray<FS_RC_MIP>(brick_range != nullptr, grid, s, f);
  else
    launch_ray<FS_RC_DVR>(brick_range != nullptr, grid, s, f);
  FS_LAUNCH_CHECK();
  return FS_OK;
}
