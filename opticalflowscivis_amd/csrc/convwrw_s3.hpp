// convwrw_s3.hpp -- round 6: the weight gradient of the k = 4, stride 2 layers (IFBlock's conv0 pair, deconv1 and the flow
// head's deconv2) with fp32 ACCURACY on the bf16 matrix rate: the split-operand form of convfwd_s3.hpp (every fp32 operand =
// three bf16 pieces, six v_mfma_f32_32x32x16_bf16 products accumulated in fp32, 192 instead of 512 matrix cycles per 16
// reduction elements) on the staging of the fp32 loader-wave kernel.  Included by convwrw.hip inside its anonymous namespace.
//
// Decomposition.  Bricks, chunks, loader waves, LDS images and the epilogue are those of conv3d_wrw_dma_kernel
// (wrw_dma_loader: fp32 images of G and of the source brick, LDS-DMA'd one brick ahead into the other of two buffers, ONE
// barrier per brick, no register ever in flight under an inline-assembly load).  Only the matrix waves change: the 16
// reduction elements of one MFMA are 16 consecutive positions of a 32-element reduction row, the lane half `kh` takes the
// upper or lower 8.  A lane's G operand is then 8 contiguous floats of its channel (two ds_read_b128); its source operand
// is the same 8 positions at the column's tap, every second float of a staged row (stride 2: four ds_read2_b32).  The
// matrix wave splits both operands in registers (11 VALU per pair of values, v_cvt_pk_bf16_f32 rounding to nearest) and
// issues the six products: the G operand of a step is split once for all the wave's column tiles, a column tile's source
// operand once for both row tiles.  Why the split is not done once per LDS image by the loaders (as in convfwd_s3.hpp): the
// fp32 staging is kept exactly as validated (ms / det / ragged / Wo == 16 forms, cold-cache behaviour), and the splitting
// VALU work runs beside the MFMAs of the same wave instead of on the loaders' critical path; the ablation switches below
// measure what it costs.
//
// Non-finite operands: +-inf splits into (inf, NaN, NaN), so a dW entry that the fp32 kernel gives as +-inf comes out NaN
// here (still non-finite).
#pragma once

typedef __bf16 w3_bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned w3_u32x4 __attribute__((ext_vector_type(4)));
typedef float w3_f32x4 __attribute__((ext_vector_type(4)));
typedef float w3_f32x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ unsigned w3_pack(float a, float b) {  // {bf16(a), bf16(b)}, round to nearest even
  typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
  const bf16x2_t h = {(__bf16)a, (__bf16)b};
  return __builtin_bit_cast(unsigned, h);
}

// One piece of the split: the word {bf16 of ra, bf16 of rc}, and (ra, rc) become what the piece leaves of them.
// OPAQUE: the packed word is hidden from the optimiser, which otherwise converts ra a second time (v_cvt_pk_bf16_f32 ra, 0)
// to take the low half: 5 instead of 6 instructions (w3_split2<true>: convwrwwino4.hpp; the k4 kernels keep the
// instruction stream they were validated and measured with).
template <bool OPAQUE>
__device__ __forceinline__ unsigned w3_peel(float& ra, float& rc) {
  unsigned w = w3_pack(ra, rc);
  if (OPAQUE) asm volatile("" : "+v"(w));
  ra -= __uint_as_float(w << 16); rc -= __uint_as_float(w & 0xffff0000u);
  asm volatile("" : "+v"(ra), "+v"(rc));  // (keeps the SLP vectoriser from pairing the subtractions: v_pk_add_f32 + moves)
  return w;
}

// (ra, rc) -> word {bf16 of ra, bf16 of rc} of each of the three pieces; ab: measurement forms (FLOWSCI_WRW_S3_AB)
template <bool OPAQUE = false>
__device__ __forceinline__ void w3_split2(float ra, float rc, unsigned& w0, unsigned& w1, unsigned& w2, int ab) {
#ifdef FS_ABLATION
  if (ab & 1) {  // (measurement: no conversion -- the raw words as "pieces", wrong by design)
    w0 = __float_as_uint(ra); w1 = __float_as_uint(rc); w2 = __float_as_uint(ra);
    return;
  }
#endif
  (void)ab;
  w0 = w3_peel<OPAQUE>(ra, rc);
  w1 = w3_peel<OPAQUE>(ra, rc);
  w2 = w3_pack(ra, rc);
}

// v[0..7] -> three bf16x8 pieces (element i of a piece is piece of v[i])
__device__ __forceinline__ void w3_split(const float (&v)[8], w3_bf16x8 (&h)[3], int ab) {
  unsigned w[3][4];
#pragma unroll
  for (int i = 0; i < 4; ++i) w3_split2(v[2 * i], v[2 * i + 1], w[0][i], w[1][i], w[2][i], ab);
#pragma unroll
  for (int pc = 0; pc < 3; ++pc) {
    const w3_u32x4 u = {w[pc][0], w[pc][1], w[pc][2], w[pc][3]};
    h[pc] = __builtin_bit_cast(w3_bf16x8, u);
  }
}

template <int NC, int MT, int TZ, int TY, int FULL, int HALF, int KWX = 32>
__global__ __launch_bounds__(512, 2) void conv3d_wrw_s3_kernel(const float* __restrict__ G,
                                                            const float* __restrict__ Src,
                                                            float* __restrict__ dW, WB p) {
  constexpr int K = 4, S = 2;
  constexpr int K3 = K * K * K;
  constexpr int NTOT = NC * K3;
  constexpr int NT32 = 4 * FULL + 2 * HALF;
  static_assert(NT32 * 32 >= NTOT && (NT32 - 1) * 32 < NTOT + 32, "column tiles cover the chunk");
  static_assert(HALF == 0 || MT == 2, "a shared column tile is split by row tile");
  constexpr int NB = FULL + HALF;  // source operands per reduction step
  using Geo = WrwDmaGeom<K, S, NC, MT, TZ, TY, KWX>;
  constexpr int ROWS = Geo::ROWS, YR = Geo::YR, XL = Geo::XL, XP = Geo::XP, PSP = Geo::PSP, CHSP = Geo::CHSP,
                GP = Geo::GP, NGL = Geo::NGL, BUF = Geo::BUF;
  __shared__ __attribute__((aligned(16))) float lds[2 * BUF];

  const int t = threadIdx.x, lane = t & 63;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int wv = wave & 3;           // waves 0-3: matrix waves, one per SIMD; waves 4-7: their loader partners
  const int l31 = lane & 31, kh = lane >> 5;
  const int c0 = blockIdx.y * NC;
  const int g0 = blockIdx.z * 32 * MT;
  const long long s0 = (long long)blockIdx.x * p.spw;
  const long long s1 = min(s0 + p.spw, p.bricks);

  if (wave >= 4) {
    wrw_dma_loader<K, S, NC, MT, TZ, TY, KWX>(G, Src, p, lds, wv, lane, s0, s1);
    return;
  }

  // ---- matrix waves.  Source operand of column tile n: float boff[n] + 2 i of a row (i = 0..7), boff carrying the
  // column's (channel, kz, ky, kx) and the lane half's 8 positions
  int boff[NB];
#pragma unroll
  for (int n = 0; n < NB; ++n) {
    const int tile = (n < FULL) ? wv * FULL + n : 4 * FULL + (wv >> 1);
    const int j = tile * 32 + l31;
    int off = 0;
    if (j < NTOT) {
      const int c = j / K3, r = j - c * K3;
      const int kz = r / (K * K), ky = (r / K) % K, kx = r % K;
      off = c * CHSP + kz * PSP + ky * XP + kx;
    }
    boff[n] = off + XL - p.pad + 8 * kh * S;
  }
  const int aoff = l31 * GP + 8 * kh;                      // G operand: channel l31 of row tile m, positions 8 kh ..
  const int hoff = ((wv & 1) * 32 + l31) * GP + 8 * kh;    // ... of the shared column tile's row tile
  const int ab = p.ab;

  f32x16 acc[FULL > 0 ? FULL : 1][MT];
  f32x16 acch;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    acch[r] = 0.f;
#pragma unroll
    for (int n = 0; n < FULL; ++n)
#pragma unroll
      for (int m = 0; m < MT; ++m) acc[n][m][r] = 0.f;
  }

  __builtin_amdgcn_s_barrier();  // brick s0 has landed
  int buf = 0;
  for (long long st = s0; st < s1; ++st) {
    const float* sG = lds + buf * BUF;
    const float* sS = sG + NGL;
    // The brick is a sequence of UNITS u = (step q = u / NB, column tile n = u % NB); step q is row q / 2, positions
    // 16 (q & 1) + 8 kh .. + 7 of its 32 (KWX = 16: y sub-row q & 1, x 8 kh ..).  Iteration u issues the MFMAs of unit u,
    // splits the operands of unit u + 1 (read an iteration ago) and reads those of unit u + 2: the splitting VALU work and
    // the operand reads sit between the MFMAs of the same wave.
    constexpr int NQ = ROWS * (KW / 16), NU = NQ * NB;
    auto srow = [&](int q) {
      const int row = q >> 1, hq = q & 1;
      return (row / TY) * S * PSP + ((row % TY) * YR + (KWX == 16 ? hq : 0)) * S * XP + (KWX == 32 ? 16 * hq * S : 0);
    };
    auto read_a = [&](int q, float (&ra)[MT][8], float (&rh)[8]) {
      const int gb = (q >> 1) * KW + 16 * (q & 1);
#pragma unroll
      for (int m = 0; m < MT; ++m) {
        const w3_f32x4 lo = *reinterpret_cast<const w3_f32x4*>(sG + m * 32 * GP + aoff + gb);
        const w3_f32x4 hi = *reinterpret_cast<const w3_f32x4*>(sG + m * 32 * GP + aoff + gb + 4);
#pragma unroll
        for (int i = 0; i < 4; ++i) { ra[m][i] = lo[i]; ra[m][4 + i] = hi[i]; }
      }
      if (HALF) {
        const w3_f32x4 lo = *reinterpret_cast<const w3_f32x4*>(sG + hoff + gb);
        const w3_f32x4 hi = *reinterpret_cast<const w3_f32x4*>(sG + hoff + gb + 4);
#pragma unroll
        for (int i = 0; i < 4; ++i) { rh[i] = lo[i]; rh[4 + i] = hi[i]; }
      }
    };
    auto read_b = [&](int u, float (&rb)[8]) {
      const float* q = sS + boff[u % NB] + srow(u / NB);
#pragma unroll
      for (int i = 0; i < 8; ++i) rb[i] = q[S * i];
    };
    constexpr int PA[6] = {2, 0, 1, 1, 0, 0}, PB[6] = {0, 2, 1, 0, 1, 0};  // the six products, small terms first
    w3_bf16x8 pa[2][MT][3], ph[2][3], pb[2][3];  // pieces: G operands by step parity, source operands by unit parity
    float ra[MT][8], rh[8], rb[8];
    read_a(0, ra, rh);
    read_b(0, rb);
#pragma unroll
    for (int m = 0; m < MT; ++m) w3_split(ra[m], pa[0][m], ab);
    if (HALF) w3_split(rh, ph[0], ab);
    w3_split(rb, pb[0], ab);
    if (NU > 1) {
      if (NB == 1) read_a(1, ra, rh);
      read_b(1, rb);
    }
#pragma unroll
    for (int u = 0; u < NU; ++u) {
      __builtin_amdgcn_sched_barrier(0);
      const int q = u / NB, n = u % NB;
#ifdef FS_ABLATION
      if (!(ab & 2))  // (measurement: no MFMAs, wrong by design)
#endif
      {
        if (n < FULL) {
#pragma unroll
          for (int q6 = 0; q6 < 6; ++q6)
#pragma unroll
            for (int m = 0; m < MT; ++m)
              acc[n][m] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(pa[q & 1][m][PA[q6]], pb[u & 1][PB[q6]], acc[n][m], 0, 0, 0);
        } else {
#pragma unroll
          for (int q6 = 0; q6 < 6; ++q6) acch = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ph[q & 1][PA[q6]], pb[u & 1][PB[q6]], acch, 0, 0, 0);
        }
      }
      if (u + 1 < NU) {
        if ((u + 1) % NB == 0) {  // unit u + 1 starts step q + 1: its G operands were read with its source operand
#pragma unroll
          for (int m = 0; m < MT; ++m) w3_split(ra[m], pa[(q + 1) & 1][m], ab);
          if (HALF) w3_split(rh, ph[(q + 1) & 1], ab);
        }
        w3_split(rb, pb[(u + 1) & 1], ab);
      }
      if (u + 2 < NU) {
        if ((u + 2) % NB == 0) read_a((u + 2) / NB, ra, rh);
        read_b(u + 2, rb);
      }
#ifdef FS_ABLATION
      if (ab & 2) {
#pragma unroll
        for (int pc = 0; pc < 3; ++pc) {
          asm volatile("" ::"v"(pb[u & 1][pc]));
#pragma unroll
          for (int m = 0; m < MT; ++m) asm volatile("" ::"v"(pa[q & 1][m][pc]));
          if (HALF) asm volatile("" ::"v"(ph[q & 1][pc]));
        }
      }
#endif
    }
    __builtin_amdgcn_s_barrier();  // the next brick has landed, everyone is done reading `buf`
    buf ^= 1;
  }

  auto flush = [&](const f32x16& a, int tile, int m) {
    const int j = tile * 32 + l31;
    if (j >= NTOT || c0 * K3 + j >= p.Cs * K3) return;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int g = g0 + m * 32 + (r & 3) + 8 * (r >> 2) + 4 * kh;
      if (g < p.Cg) {
        float* q = dW + (size_t)blockIdx.x * p.slab + (size_t)g * p.Cs * K3 + (size_t)c0 * K3 + j;
        if (p.slab) *q = a[r]; else atomicAdd(q, a[r]);
      }
    }
  };
#pragma unroll
  for (int n = 0; n < FULL; ++n)
#pragma unroll
    for (int m = 0; m < MT; ++m) flush(acc[n][m], wv * FULL + n, m);
  if (HALF) flush(acch, 4 * FULL + (wv >> 1), wv & 1);
}

// same grid, runs and deterministic-mode bookkeeping as launch_dma
template <int NC, int MT, int TZ, int TY, int FULL, int HALF, int KWX = 32>
int launch_wrw_s3(const float* G, const float* Src, float* dW, const WP& w, hipStream_t st, const WDet* det = nullptr) {
  constexpr int K = 4;
  WB p;
  p.B = w.B; p.Cg = w.Cg; p.Cs = w.Cs; p.Do = w.Do; p.Ho = w.Ho; p.Wo = w.Wo;
  p.Di = w.Di; p.Hi = w.Hi; p.Wi = w.Wi; p.pad = w.pad;
  p.nsrc = w.nsrc;
  for (int c = 0; c < w.nsrc; ++c) { p.src[c] = w.srcv[c]; p.sbs[c] = w.sbsv[c]; }
  p.bz = fs::cdiv(p.Do, TZ); p.by = fs::cdiv(p.Ho, TY * (KW / KWX)); p.bx = fs::cdiv(p.Wo, KWX);
  p.bricks = (long long)p.B * p.bz * p.by * p.bx;
  const int mtiles = fs::cdiv(p.Cg, 32 * MT);
  const int nchunks = fs::cdiv(p.Cs, NC);
  long long want = 256 / ((long long)mtiles * nchunks);
  if (want < 1) want = 1;
  long long spw = (p.bricks + want - 1) / want;
  if (spw < 1) spw = 1;
  p.spw = (int)(spw > (1 << 20) ? (1 << 20) : spw);
  const long long gx = (p.bricks + p.spw - 1) / p.spw;
  if (gx >= (1ll << 31) || nchunks > 65535 || mtiles > 65535) return FS_ERR_SHAPE;
#ifdef FS_ABLATION
  static const int s3_ab = (int)FS_AB_ENV_LL("FLOWSCI_WRW_S3_AB", 0);  // 1: no conversion, 2: no MFMAs (wrong results by design)
  p.ab = s3_ab;
#else
  p.ab = 0;
#endif
  constexpr int K3 = K * K * K;
  float* out;
  const long long dwf = (long long)p.Cg * p.Cs * K3;
  const int drc = wrw_det_begin(det, gx, dwf, dW, &out, &p.slab);
  if (drc >= 0) return drc;
  hipLaunchKernelGGL((conv3d_wrw_s3_kernel<NC, MT, TZ, TY, FULL, HALF, KWX>), dim3((unsigned)gx, nchunks, mtiles), dim3(512), 0,
                     st, G, Src, out, p);
  wrw_det_end(det, gx, dwf, dW, st);
  FS_LAUNCH_CHECK();
  return FS_OK;
}
