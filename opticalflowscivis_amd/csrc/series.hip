// series.hip -- training batches out of a volume time series that lives on the GPU in its stored type.
//
// fs_triplet_gather: the reference keeps its simulation output in host memory as fp32, appends flipped copies (4x the
// memory, Flow-3D/load_datasets.py:147-152), cuts (img0, img1, gt) triplets (:171-183) and copies every batch to the
// GPU in front of the step (Flow-3D/train.py:144).  Here the stored array (u8 / u16 / f16 / f32) is uploaded once and
// a batch is ONE launch: per sample a 64-byte record in device memory names the three frames (element offsets), the
// crop origin, the mirrors and the normalisation; the kernel converts, mirrors, normalises and writes the fp32
// [B,3,Do,Ho,Wo] tensor the step reads.  Nothing is materialised but that tensor.
//
// Per element: v = stored value converted exactly to fp32; a non-finite v becomes 0; out = (v - lo) * inv, two
// separately rounded fp32 operations (contraction off), so numpy fp32 reproduces it bit for bit.
//
// The records are device data the library cannot check, so the kernel never forms an address outside
// [base, base + n_elems): a source coordinate outside the frame or an element index outside the array reads as 0.
// A record whose three frames and crop lie inside the array and the frame (wave-uniform test on the record) takes
// unconditional loads; anything else goes through the per-element checks.
//
// Layout: a pure stream, HBM-bound, no LDS.  With Wo % 4 == 0 and a 16-byte aligned output a lane owns 4 consecutive
// outputs of a row for all three frames (3 loads in flight, 3 16-byte stores); its 4 source elements are one 16 / 8 /
// 4-byte load (f32 / u16,f16 / u8) when offsets, origin and row length are multiples of 4, else 4 element loads.
// The W mirror reads the mirrored group and reverses it in registers; D and H mirrors are row arithmetic.  Otherwise
// (Wo % 4 != 0) one element per lane.  Workgroups of one sample step through its rows together.
//
// fs_series_stats: per stored frame the minimum and maximum over the finite elements and the count of non-finite
// ones; per-workgroup partials in `ws`, a second launch combines them in a fixed order (no atomics).
//
// fs_series_encode: the way back -- the corner [0:D, 0:H, 0:W] of padded fp32 planes [N,C,Dp,Hp,Wp] written as a
// contiguous [N,C,D,H,W] array of a stored type (the crop and the conversion in one pass).  Per element y = x * span,
// then y = y + lo (two separately rounded fp32 operations); a non-finite y is stored as 0; u8 / u16 clamp to the type
// and round to nearest even, f16 saturates at +-65504 and converts with round to nearest even, f32 stores y.
// Optionally per item {min y, max y over the finite y before clamping, n below, n above, n non-finite}: partials per
// workgroup, a second launch in fixed order.  The same stream layout as the gather: with W % 4 == 0 and Wp % 4 == 0 a
// lane owns 4 consecutive outputs of a row (one 16-byte load and one 4 / 8 / 16-byte store when both pointers allow
// it, 4 element accesses otherwise -- which lane reduces which elements is a function of the shape alone), else one
// element per lane.
#include "common.hpp"

namespace {

constexpr int NT = 256;
constexpr long long kTargetBlocks = 2048;  // 8 workgroups per CU

struct U8 {
  typedef unsigned char S;
  static __device__ __forceinline__ float cv(S s) { return (float)s; }
};
struct U16 {
  typedef unsigned short S;
  static __device__ __forceinline__ float cv(S s) { return (float)s; }
};
struct F16 {
  typedef unsigned short S;
  static __device__ __forceinline__ float cv(S s) {
    _Float16 h;
    __builtin_memcpy(&h, &s, 2);
    return (float)h;
  }
};
struct F32 {
  typedef float S;
  static __device__ __forceinline__ float cv(S s) { return s; }
};

__device__ __forceinline__ bool finite32(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

template <typename S, int N>
struct alignas(N * sizeof(S)) Pack { S s[N]; };

struct GP {
  unsigned long long n_elems;
  unsigned long long F;   // elements per frame = Ds*Hs*Ws
  unsigned Q;             // work items per sample: Do*Ho*Wo / V
  int Ds, Hs, Ws, Do, Ho, Wo;
  int G;                  // workgroups per sample
  int src_vec;            // base is 16-byte aligned and Ws % 4 == 0: aligned records may use vector loads
};

template <class K, int V>
__global__ __launch_bounds__(NT) void triplet_gather_kernel(const typename K::S* __restrict__ base,
                                                            const FsTripletJob* __restrict__ jobs,
                                                            float* __restrict__ out, GP g) {
#pragma clang fp contract(off)
  typedef typename K::S S;
  const int b = blockIdx.x / g.G, blk = blockIdx.x - b * g.G;
  const FsTripletJob j = jobs[b];
  const bool fw = j.flip & 1u, fh = j.flip & 2u, fd = j.flip & 4u;
  const unsigned long long off[3] = {(unsigned long long)j.off[0], (unsigned long long)j.off[1],
                                     (unsigned long long)j.off[2]};
  // the whole record inside the frame and the array: loads need no check (uniform over the workgroup)
  bool inside = j.z0 >= 0 && j.y0 >= 0 && j.x0 >= 0 && j.z0 <= g.Ds - g.Do && j.y0 <= g.Hs - g.Ho &&
                j.x0 <= g.Ws - g.Wo;
#pragma unroll
  for (int c = 0; c < 3; ++c) inside = inside && off[c] <= g.n_elems && g.n_elems - off[c] >= g.F;
  const bool vec = V == 4 && inside && g.src_vec && ((off[0] | off[1] | off[2]) & 3ull) == 0 && (j.x0 & 3) == 0;
  const unsigned GW = (unsigned)(g.Wo / V);
  const size_t P = (size_t)g.Do * g.Ho * g.Wo;
  float* ob = out + (size_t)b * 3 * P;
  const float lo = j.lo, inv = j.inv;
  for (unsigned q = (unsigned)blk * NT + threadIdx.x; q < g.Q; q += (unsigned)g.G * NT) {
    const unsigned row = q / GW;
    const int x = (int)(q - row * GW) * V;
    const int z = (int)(row / (unsigned)g.Ho), y = (int)(row - (unsigned)z * g.Ho);
    const long long zs = (long long)j.z0 + (fd ? g.Do - 1 - z : z);
    const long long ys = (long long)j.y0 + (fh ? g.Ho - 1 - y : y);
    const long long xs0 = (long long)j.x0 + (fw ? g.Wo - V - x : x);  // source x of the group's lowest element
    const bool rowok = zs >= 0 && zs < g.Ds && ys >= 0 && ys < g.Hs;
    const unsigned long long roff = rowok ? (unsigned long long)((zs * g.Hs + ys) * g.Ws) : 0ull;
    float v[3][V];
    if (vec) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const Pack<S, V> pk = *reinterpret_cast<const Pack<S, V>*>(base + (off[c] + roff + (unsigned long long)xs0));
#pragma unroll
        for (int i = 0; i < V; ++i) v[c][i] = K::cv(pk.s[i]);
      }
    } else {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
#pragma unroll
        for (int i = 0; i < V; ++i) {
          const long long xs = xs0 + i;
          const unsigned long long e = off[c] + roff + (unsigned long long)xs;  // (modular: a negative offset is fine)
          const bool ok = rowok && xs >= 0 && xs < g.Ws && e < g.n_elems;
          v[c][i] = ok ? K::cv(base[e]) : 0.f;
        }
      }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      float o[V];
#pragma unroll
      for (int i = 0; i < V; ++i) {
        float t = v[c][fw ? V - 1 - i : i];
        t = finite32(t) ? t : 0.f;
        t = t - lo;
        o[i] = t * inv;
      }
      float* op = ob + c * P + (size_t)row * g.Wo + x;
      if (V == 4)
        *reinterpret_cast<float4*>(op) = make_float4(o[0], o[V > 1 ? 1 : 0], o[V > 2 ? 2 : 0], o[V > 3 ? 3 : 0]);
      else
        op[0] = o[0];
    }
  }
}

inline bool aligned(const void* p, size_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

template <class K>
void launch_gather(const void* base, const FsTripletJob* jobs, float* out, GP g, int B, bool v4, hipStream_t s) {
  typedef typename K::S S;
  const unsigned long long items = (unsigned long long)g.Do * g.Ho * g.Wo / (v4 ? 4 : 1);
  g.Q = (unsigned)items;
  long long G = (kTargetBlocks + B - 1) / B;
  const long long gmax = (long long)((items + NT - 1) / NT);
  if (G > gmax) G = gmax;
  if (G < 1) G = 1;
  g.G = (int)G;
  const dim3 grid((unsigned)(B * G)), blk(NT);
  if (v4)
    hipLaunchKernelGGL((triplet_gather_kernel<K, 4>), grid, blk, 0, s, (const S*)base, jobs, out, g);
  else
    hipLaunchKernelGGL((triplet_gather_kernel<K, 1>), grid, blk, 0, s, (const S*)base, jobs, out, g);
}

int elem_size(int dtype) {
  switch (dtype) {
    case FS_SERIES_U8: return 1;
    case FS_SERIES_U16: case FS_SERIES_F16: return 2;
    case FS_SERIES_F32: return 4;
    default: return 0;
  }
}

// ---------------------------------------------------------------------------------------------- fs_series_stats
__device__ __forceinline__ void stat1(float v, float& mn, float& mx, unsigned long long& bad) {
  if (finite32(v)) { mn = fminf(mn, v); mx = fmaxf(mx, v); } else { ++bad; }
}

template <class K>
__global__ __launch_bounds__(NT) void series_stats_kernel(const typename K::S* __restrict__ base,
                                                          double* __restrict__ ws, unsigned long long F, int G,
                                                          int vec) {
  typedef typename K::S S;
  constexpr int VE = 16 / (int)sizeof(S);
  const int t = blockIdx.x / G, blk = blockIdx.x - t * G;
  const S* p = base + (size_t)t * F;
  float mn = HUGE_VALF, mx = -HUGE_VALF;
  unsigned long long bad = 0;
  const unsigned long long step = (unsigned long long)G * NT;
  if (vec) {
    const unsigned long long n = F / VE;
    for (unsigned long long q = (unsigned long long)blk * NT + threadIdx.x; q < n; q += step) {
      const Pack<S, VE> pk = *reinterpret_cast<const Pack<S, VE>*>(p + q * VE);
#pragma unroll
      for (int i = 0; i < VE; ++i) stat1(K::cv(pk.s[i]), mn, mx, bad);
    }
  } else {
    for (unsigned long long q = (unsigned long long)blk * NT + threadIdx.x; q < F; q += step)
      stat1(K::cv(p[q]), mn, mx, bad);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    mn = fminf(mn, __shfl_xor(mn, o, 64));
    mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    bad += __shfl_xor(bad, o, 64);
  }
  __shared__ float rmn[NT / 64], rmx[NT / 64];
  __shared__ unsigned long long rbad[NT / 64];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if (lane == 0) { rmn[wv] = mn; rmx[wv] = mx; rbad[wv] = bad; }
  __syncthreads();
  if (threadIdx.x == 0) {
    double* w = ws + ((size_t)t * G + blk) * 3;
    w[0] = (double)fminf(fminf(rmn[0], rmn[1]), fminf(rmn[2], rmn[3]));
    w[1] = (double)fmaxf(fmaxf(rmx[0], rmx[1]), fmaxf(rmx[2], rmx[3]));
    w[2] = (double)rbad[0] + (double)rbad[1] + (double)rbad[2] + (double)rbad[3];
  }
}

// Second stage: one workgroup per frame combines its G partials -> out[t] = {min, max, non-finite count}.
__global__ __launch_bounds__(NT) void series_stats_final_kernel(const double* __restrict__ ws, int G,
                                                                double* __restrict__ out) {
  __shared__ double red[3][NT];
  const double* w = ws + (size_t)blockIdx.x * G * 3;
  double mn = HUGE_VAL, mx = -HUGE_VAL, bad = 0.0;
  for (int i = threadIdx.x; i < G; i += NT) {
    mn = fmin(mn, w[3 * i]);
    mx = fmax(mx, w[3 * i + 1]);
    bad += w[3 * i + 2];  // integers below 2^53: exact in any order
  }
  red[0][threadIdx.x] = mn; red[1][threadIdx.x] = mx; red[2][threadIdx.x] = bad;
  __syncthreads();
  for (int s = NT / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) {
      red[0][threadIdx.x] = fmin(red[0][threadIdx.x], red[0][threadIdx.x + s]);
      red[1][threadIdx.x] = fmax(red[1][threadIdx.x], red[1][threadIdx.x + s]);
      red[2][threadIdx.x] += red[2][threadIdx.x + s];
    }
    __syncthreads();
  }
  if (threadIdx.x < 3) out[(size_t)blockIdx.x * 3 + threadIdx.x] = red[threadIdx.x][0];
}

int stats_plan(int T, long long F, int& G) {
  if (T < 1 || F < 1 || F > (1LL << 40) || T > (1 << 22)) return FS_ERR_SHAPE;
  long long g = (kTargetBlocks + T - 1) / T;
  const long long gmax = (F + NT * 4 - 1) / (NT * 4);
  if (g > gmax) g = gmax;
  if (g < 1) g = 1;
  G = (int)g;
  return FS_OK;
}

template <class K>
void launch_stats(const void* base, double* ws, double* out, int T, long long F, int G, hipStream_t s) {
  typedef typename K::S S;
  const int vec = aligned(base, 16) && (F * (long long)sizeof(S)) % 16 == 0;
  hipLaunchKernelGGL((series_stats_kernel<K>), dim3((unsigned)(T * G)), dim3(NT), 0, s, (const S*)base, ws,
                     (unsigned long long)F, G, vec);
  hipLaunchKernelGGL(series_stats_final_kernel, dim3((unsigned)T), dim3(NT), 0, s, ws, G, out);
}

// ---------------------------------------------------------------------------------------------- fs_series_encode
struct EncAcc {
  float mn, mx;
  unsigned long long low, high, bad;
};

// y -> the stored value; counts what clamping and the non-finite rule changed.
struct EU8 {
  typedef unsigned char S;
  static __device__ __forceinline__ S enc(float y, EncAcc& a) {
    a.low += y < 0.f; a.high += y > 255.f;
    return (S)(int)rintf(fminf(fmaxf(y, 0.f), 255.f));
  }
};
struct EU16 {
  typedef unsigned short S;
  static __device__ __forceinline__ S enc(float y, EncAcc& a) {
    a.low += y < 0.f; a.high += y > 65535.f;
    return (S)(int)rintf(fminf(fmaxf(y, 0.f), 65535.f));
  }
};
struct EF16 {
  typedef unsigned short S;
  static __device__ __forceinline__ S enc(float y, EncAcc& a) {
    a.low += y < -65504.f; a.high += y > 65504.f;
    const _Float16 h = (_Float16)fminf(fmaxf(y, -65504.f), 65504.f);  // round to nearest even
    S s;
    __builtin_memcpy(&s, &h, 2);
    return s;
  }
};
struct EF32 {
  typedef float S;
  static __device__ __forceinline__ S enc(float y, EncAcc&) { return y; }
};

struct EP {
  unsigned Q;        // work items per item of the batch: C*D*H*W / V
  int C, Dp, Hp, Wp, D, H, W;
  int G;             // workgroups per item
  int vec;           // src 16-byte aligned and dst aligned to 4 elements: vector accesses (V == 4 only)
  float lo, span;
};

template <class E, int V, bool STATS>
__global__ __launch_bounds__(NT) void series_encode_kernel(const float* __restrict__ src,
                                                           typename E::S* __restrict__ dst, double* __restrict__ ws,
                                                           EP g) {
#pragma clang fp contract(off)
  typedef typename E::S S;
  const int n = blockIdx.x / g.G, blk = blockIdx.x - n * g.G;
  const unsigned GW = (unsigned)(g.W / V);
  const unsigned DH = (unsigned)g.D * (unsigned)g.H;
  const size_t rows = (size_t)g.C * DH;  // output rows per item
  const float* sb = src + (size_t)n * g.C * g.Dp * g.Hp * g.Wp;
  S* db = dst + (size_t)n * rows * g.W;
  EncAcc a = {HUGE_VALF, -HUGE_VALF, 0ull, 0ull, 0ull};
  for (unsigned q = (unsigned)blk * NT + threadIdx.x; q < g.Q; q += (unsigned)g.G * NT) {
    const unsigned row = q / GW;
    const unsigned x = (q - row * GW) * V;
    const unsigned c = row / DH, r = row - c * DH;
    const unsigned z = r / (unsigned)g.H, y0 = r - z * (unsigned)g.H;
    const float* sp = sb + (((size_t)c * g.Dp + z) * g.Hp + y0) * g.Wp + x;
    S* dp = db + (size_t)row * g.W + x;
    float v[V];
    if (V == 4 && g.vec) {
      const float4 f = *reinterpret_cast<const float4*>(sp);
      v[0] = f.x; v[V > 1 ? 1 : 0] = f.y; v[V > 2 ? 2 : 0] = f.z; v[V > 3 ? 3 : 0] = f.w;
    } else {
#pragma unroll
      for (int i = 0; i < V; ++i) v[i] = sp[i];
    }
    Pack<S, V> pk;
#pragma unroll
    for (int i = 0; i < V; ++i) {
      float y = v[i] * g.span;
      y = y + g.lo;
      if (finite32(y)) {
        a.mn = fminf(a.mn, y); a.mx = fmaxf(a.mx, y);
        pk.s[i] = E::enc(y, a);
      } else {
        ++a.bad;
        pk.s[i] = (S)0;
      }
    }
    if (V == 4 && g.vec) {
      *reinterpret_cast<Pack<S, V>*>(dp) = pk;
    } else {
#pragma unroll
      for (int i = 0; i < V; ++i) dp[i] = pk.s[i];
    }
  }
  if (!STATS) return;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    a.mn = fminf(a.mn, __shfl_xor(a.mn, o, 64));
    a.mx = fmaxf(a.mx, __shfl_xor(a.mx, o, 64));
    a.low += __shfl_xor(a.low, o, 64);
    a.high += __shfl_xor(a.high, o, 64);
    a.bad += __shfl_xor(a.bad, o, 64);
  }
  __shared__ float rmn[NT / 64], rmx[NT / 64];
  __shared__ unsigned long long rcnt[3][NT / 64];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if (lane == 0) { rmn[wv] = a.mn; rmx[wv] = a.mx; rcnt[0][wv] = a.low; rcnt[1][wv] = a.high; rcnt[2][wv] = a.bad; }
  __syncthreads();
  if (threadIdx.x == 0) {
    double* w = ws + ((size_t)n * g.G + blk) * 5;
    w[0] = (double)fminf(fminf(rmn[0], rmn[1]), fminf(rmn[2], rmn[3]));
    w[1] = (double)fmaxf(fmaxf(rmx[0], rmx[1]), fmaxf(rmx[2], rmx[3]));
#pragma unroll
    for (int k = 0; k < 3; ++k)
      w[2 + k] = (double)rcnt[k][0] + (double)rcnt[k][1] + (double)rcnt[k][2] + (double)rcnt[k][3];
  }
}

// Second stage: one workgroup per item combines its G partials -> out[n] = {min, max, n_low, n_high, n_nonfinite}.
__global__ __launch_bounds__(NT) void series_encode_final_kernel(const double* __restrict__ ws, int G,
                                                                 double* __restrict__ out) {
  __shared__ double red[5][NT];
  const double* w = ws + (size_t)blockIdx.x * G * 5;
  double v[5] = {HUGE_VAL, -HUGE_VAL, 0.0, 0.0, 0.0};
  for (int i = threadIdx.x; i < G; i += NT) {
    v[0] = fmin(v[0], w[5 * i]);
    v[1] = fmax(v[1], w[5 * i + 1]);
#pragma unroll
    for (int k = 2; k < 5; ++k) v[k] += w[5 * i + k];  // integers below 2^53: exact in any order
  }
#pragma unroll
  for (int k = 0; k < 5; ++k) red[k][threadIdx.x] = v[k];
  __syncthreads();
  for (int s = NT / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) {
      red[0][threadIdx.x] = fmin(red[0][threadIdx.x], red[0][threadIdx.x + s]);
      red[1][threadIdx.x] = fmax(red[1][threadIdx.x], red[1][threadIdx.x + s]);
#pragma unroll
      for (int k = 2; k < 5; ++k) red[k][threadIdx.x] += red[k][threadIdx.x + s];
    }
    __syncthreads();
  }
  if (threadIdx.x < 5) out[(size_t)blockIdx.x * 5 + threadIdx.x] = red[threadIdx.x][0];
}

// Workgroups per item: a function of the OUTPUT shape alone (the workspace query does not know the padded extents).
int encode_plan(int N, int C, int D, int H, int W, int& G) {
  if (N < 1 || C < 1 || D < 1 || H < 1 || W < 1 || N > (1 << 20)) return FS_ERR_SHAPE;
  const long long per = (long long)C * D;  // < 2^62
  if (per > 0x7fffffffLL || per * H > 0x7fffffffLL || per * H * W > 0x7fffffffLL) return FS_ERR_SHAPE;
  const long long e = per * H * W;
  if (e * N > (1LL << 40)) return FS_ERR_SHAPE;
  long long g = (kTargetBlocks + N - 1) / N;
  const long long gmax = (e + NT * 4 - 1) / (NT * 4);
  if (g > gmax) g = gmax;
  if (g < 1) g = 1;
  G = (int)g;
  return FS_OK;
}

template <class E>
void launch_encode(const float* src, void* dst, double* ws, double* stats, EP g, int N, hipStream_t s) {
  typedef typename E::S S;
  const bool v4 = g.W % 4 == 0 && g.Wp % 4 == 0;
  g.Q = (unsigned)((long long)g.C * g.D * g.H * g.W / (v4 ? 4 : 1));
  g.vec = v4 && aligned(src, 16) && aligned(dst, 4 * sizeof(S));
  const dim3 grid((unsigned)(N * g.G)), blk(NT);
  if (ws) {
    if (v4)
      hipLaunchKernelGGL((series_encode_kernel<E, 4, true>), grid, blk, 0, s, src, (S*)dst, ws, g);
    else
      hipLaunchKernelGGL((series_encode_kernel<E, 1, true>), grid, blk, 0, s, src, (S*)dst, ws, g);
    hipLaunchKernelGGL(series_encode_final_kernel, dim3((unsigned)N), dim3(NT), 0, s, ws, g.G, stats);
  } else {
    if (v4)
      hipLaunchKernelGGL((series_encode_kernel<E, 4, false>), grid, blk, 0, s, src, (S*)dst, ws, g);
    else
      hipLaunchKernelGGL((series_encode_kernel<E, 1, false>), grid, blk, 0, s, src, (S*)dst, ws, g);
  }
}

}  // namespace

extern "C" int fs_triplet_gather(const void* base, int dtype, long long n_elems, int Ds, int Hs, int Ws,
                                 const FsTripletJob* jobs, int B, int Do, int Ho, int Wo, float* out,
                                 fs_stream_t stream) {
  FS_ENTER();
  FS_REQUIRE_PTR(base); FS_REQUIRE_PTR(jobs); FS_REQUIRE_PTR(out);
  if (B < 1 || B > (1 << 20) || Ds < 1 || Hs < 1 || Ws < 1 || Do < 1 || Ho < 1 || Wo < 1) return FS_ERR_SHAPE;
  if (Do > Ds || Ho > Hs || Wo > Ws || n_elems < 1) return FS_ERR_SHAPE;
  const long long F = (long long)Ds * Hs;
  if (F > (1LL << 40) / Ws || F * Ws > n_elems) return FS_ERR_SHAPE;
  if ((long long)Do * Ho * Wo > 0x7fffffffLL) return FS_ERR_SHAPE;
  const int es = elem_size(dtype);
  if (es == 0) return FS_ERR_ARG;
  if (!aligned(base, (size_t)es) || !aligned(jobs, 8) || !aligned(out, 4)) return FS_ERR_ARG;
  GP g;
  g.n_elems = (unsigned long long)n_elems;
  g.F = (unsigned long long)(F * Ws);
  g.Ds = Ds; g.Hs = Hs; g.Ws = Ws; g.Do = Do; g.Ho = Ho; g.Wo = Wo;
  g.src_vec = aligned(base, 16) && Ws % 4 == 0;
  const bool v4 = Wo % 4 == 0 && aligned(out, 16);
  const hipStream_t s = (hipStream_t)stream;
  switch (dtype) {
    case FS_SERIES_U8: launch_gather<U8>(base, jobs, out, g, B, v4, s); break;
    case FS_SERIES_U16: launch_gather<U16>(base, jobs, out, g, B, v4, s); break;
    case FS_SERIES_F16: launch_gather<F16>(base, jobs, out, g, B, v4, s); break;
    default: launch_gather<F32>(base, jobs, out, g, B, v4, s); break;
  }
  FS_LAUNCH_CHECK();
  return FS_OK;
}

extern "C" long long fs_series_stats_ws_bytes(int T, long long frame_elems) {
  int G = 0;
  const int rc = stats_plan(T, frame_elems, G);
  if (rc != FS_OK) return -rc;
  return (long long)T * G * 3 * (long long)sizeof(double);
}

extern "C" int fs_series_stats(const void* base, int dtype, int T, long long frame_elems, double* ws, double* out,
                               fs_stream_t stream) {
  FS_ENTER();
  FS_REQUIRE_PTR(base); FS_REQUIRE_PTR(ws); FS_REQUIRE_PTR(out);
  int G = 0;
  const int rc = stats_plan(T, frame_elems, G);
  if (rc != FS_OK) return rc;
  const int es = elem_size(dtype);
  if (es == 0) return FS_ERR_ARG;
  if (!aligned(base, (size_t)es) || !aligned(ws, 8) || !aligned(out, 8)) return FS_ERR_ARG;
  const hipStream_t s = (hipStream_t)stream;
  switch (dtype) {
    case FS_SERIES_U8: launch_stats<U8>(base, ws, out, T, frame_elems, G, s); break;
    case FS_SERIES_U16: launch_stats<U16>(base, ws, out, T, frame_elems, G, s); break;
    case FS_SERIES_F16: launch_stats<F16>(base, ws, out, T, frame_elems, G, s); break;
    default: launch_stats<F32>(base, ws, out, T, frame_elems, G, s); break;
  }
  FS_LAUNCH_CHECK();
  return FS_OK;
}

extern "C" long long fs_series_encode_ws_bytes(int N, int C, int D, int H, int W) {
  int G = 0;
  const int rc = encode_plan(N, C, D, H, W, G);
  if (rc != FS_OK) return -rc;
  return (long long)N * G * 5 * (long long)sizeof(double);
}

extern "C" int fs_series_encode(const float* src, int N, int C, int Dp, int Hp, int Wp, void* dst, int dtype, int D,
                                int H, int W, float lo, float span, double* ws, double* stats, fs_stream_t stream) {
  FS_ENTER();
  FS_REQUIRE_PTR(src); FS_REQUIRE_PTR(dst);
  if ((ws == nullptr) != (stats == nullptr)) return FS_ERR_NULLPTR;
  EP g;
  int rc = encode_plan(N, C, D, H, W, g.G);
  if (rc != FS_OK) return rc;
  if (Dp < 1 || Hp < 1 || Wp < 1 || D > Dp || H > Hp || W > Wp) return FS_ERR_SHAPE;
  int Gp = 0;  // the padded planes obey the same limits
  rc = encode_plan(N, C, Dp, Hp, Wp, Gp);
  if (rc != FS_OK) return rc;
  const int es = elem_size(dtype);
  if (es == 0) return FS_ERR_ARG;
  if (!aligned(src, 4) || !aligned(dst, (size_t)es) || !aligned(ws, 8) || !aligned(stats, 8)) return FS_ERR_ARG;
  g.C = C; g.Dp = Dp; g.Hp = Hp; g.Wp = Wp; g.D = D; g.H = H; g.W = W;
  g.lo = lo; g.span = span;
  const hipStream_t s = (hipStream_t)stream;
  switch (dtype) {
    case FS_SERIES_U8: launch_encode<EU8>(src, dst, ws, stats, g, N, s); break;
    case FS_SERIES_U16: launch_encode<EU16>(src, dst, ws, stats, g, N, s); break;
    case FS_SERIES_F16: launch_encode<EF16>(src, dst, ws, stats, g, N, s); break;
    default: launch_encode<EF32>(src, dst, ws, stats, g, N, s); break;
  }
  FS_LAUNCH_CHECK();
  return FS_OK;
}
