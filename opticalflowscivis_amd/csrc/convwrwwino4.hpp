// convwrwwino4.hpp -- weight gradient of the 64-channel k3 s1 p1 trunk convolutions in the 1-D Winograd F(4,3) domain
// of convwino4.hpp: HALF the matrix-core work of the direct form (convwrwwino.hpp's F(2,3): two thirds).  Included
// inside convwrw.hip's anonymous namespace, after convwrwwino.hpp (same staging, same loader waves, same grid).
//
//   forward (convwino4.hpp): M_t = sum U_t V_t (t = 0..5),  y = A^T M,  U = G g,  V = B^T d, x-tile = 4 outputs.  So
//     dM = A dy:   dM0 = dy0   dM1 = (dy0 + dy2) + (dy1 + dy3)   dM2 = (dy0 + dy2) - (dy1 + dy3)
//                  dM3 = (dy0 + 4 dy2) + (2 dy1 + 8 dy3)   dM4 = (dy0 + 4 dy2) - (2 dy1 + 8 dy3)   dM5 = dy3
//     dU_t[co, ci, kz, ky] = sum_{b, p, j} dM_t[co, p, j] V_t[ci, p + (kz, ky) - 1, j]
//     dg = G^T dU: dg0 = dU0/4 - (dU1 + dU2)/6 + (dU3 + dU4)/24      dg1 = (dU2 - dU1)/6 + (dU3 - dU4)/12
//                  dg2 = -(dU1 + dU2)/6 + (dU3 + dU4)/6 + dU5
//   Six GEMMs with K = x-TILES (a quarter as many as outputs): 6 x 9 instead of 27 x 4 multiply-adds per (co, ci, four
//   outputs).  fp32 rounding against fp64: ~3x the direct kernel's in the mean (tests/test_gpu_wino.py).
//
// Both operands are transformed when they are READ from LDS (16-byte reads at channel pitches of an odd number of
// 16-byte slots: conflict-free), as in convwrwwino.hpp.  The 36 accumulator tiles (2 row tiles x 3 ky x 6 components)
// of a workgroup's (64 co x 32 ci x one kz) share are dealt to its four matrix waves as (row tile m) x (component
// triple {0,1,2} / {3,4,5}): 9 tiles (144 VGPRs) per wave, every wave walks both rows of the 1 x 2 x 64 brick.
//
// Round 11: the products run on the bf16 matrix cores in the split-operand form of convwrw_s3.hpp.  The TRANSFORMED
// values (A dy and B^T d, formed in fp32 exactly as before) are split into three bf16 pieces each and six
// v_mfma_f32_32x32x16_bf16 products are accumulated in fp32, small terms first.  The 16 reduction elements of one MFMA
// are the 16 x-tiles of one brick row, the lane half kh holding tiles 8 kh .. 8 kh + 7: 108 MFMAs of 32 cycles per brick
// and wave instead of 144 of 64.  What bounds the loop now is the wave's VALU stream (transform + split: ~18 instructions
// per pair of values), so the split work is kept to the distinct operands: the loop is component-major, and inside a
// component the four source rows of the brick are transformed and split ONCE each and multiplied with the gradient rows
// they meet (source row r: brick row 0 at ky = r, brick row 1 at ky = r - 1) -- 12 source units and 6 gradient units of
// four pairs per brick where the (h, ky, c) order needs 18 + 6.  The fp32 form lives on in the ablation build
// (FLOWSCI_WRW_WINO4_NO_S3=1).  +-inf splits into (inf, NaN, NaN): an entry the fp32 form gives as +-inf comes out NaN.

// One SUB-STEP of the matrix waves' brick loop (72 per brick): MFMAs [m0, m1) of unit (component uc, source row ur) and one
// JOB beside them -- the transform + split of one pair of x-tiles: job 1 = source row jr, component jc, pair jp; job 2 =
// gradient row jr (slot (2 jc + jr) % 3 of the three piece sets); jn: the job belongs to the NEXT brick.  A unit's
// MFMAs: rows 1, 2 meet both gradient rows (index i = product i / 2 of gradient row i % 2), rows 0 and 3 one (index =
// product).  Source unit (r, c) is split during the unit before it; gradient set (0, c + 1) takes the slot that (1, c - 1)
// left after unit (c - 1, 3), gradient set (1, c + 1) the slot that (0, c) leaves after unit (c, 2).  Component 2 does
// the next brick's three first jobs in its last unit, behind the brick's barrier.
struct W4Step { int uc, ur, m0, m1, job, jr, jc, jp, jn; };
constexpr W4Step w4_step(int s) {
  const int c = s / 24, t = s % 24, cn = (c + 1) % 3;
  constexpr int two[5] = {0, 2, 3, 5, 6};
  if (t < 4) return {c, 0, two[t], two[t + 1], 1, 1, c, t, 0};
  if (c < 2) {
    if (t < 8) return {c, 1, 2 * (t - 4), 2 * (t - 4) + 2, 1, 2, c, t - 4, 0};
    if (t < 10) return {c, 1, 2 * (t - 4), 2 * (t - 4) + 2, 2, 0, cn, t - 8, 0};
    if (t < 12) return {c, 2, 2 * (t - 10), 2 * (t - 10) + 2, 2, 0, cn, t - 8, 0};
    if (t < 16) return {c, 2, 2 * (t - 10), 2 * (t - 10) + 2, 1, 3, c, t - 12, 0};
    const int k = t - 16, m = (k / 4) * 3 + k % 4;
    return {c, 3, m, m + (k % 4 < 3 ? 1 : 0), k < 4 ? 1 : 2, k < 4 ? 0 : 1, cn, k % 4, 0};
  }
  if (t < 8) return {c, 1, 3 * (t - 4), 3 * (t - 4) + 3, 1, 2, c, t - 4, 0};
  if (t < 12) return {c, 2, 3 * (t - 8), 3 * (t - 8) + 3, 1, 3, c, t - 8, 0};
  const int k = t - 12;
  return {c, 3, k / 2, k / 2 + (k % 2 == 0 ? 1 : 0), k < 4 ? 1 : 2, k < 4 ? 0 : (k < 8 ? 0 : 1), 0, k % 4, 1};
}
// a job's operands are read W4_PF sub-steps ahead (2 measured the same as 1); step 59's job -- source row 3, component 2,
// pair 3 -- is the last of the brick
constexpr int W4_PF = 1;
constexpr int W4_BARRIER_STEP = 60 - W4_PF;

template <class F, int... I>
__device__ __forceinline__ void w4_static_for(F&& f, std::integer_sequence<int, I...>) {
  (f(std::integral_constant<int, I>{}), ...);
}

template <int DBG>
__global__ __launch_bounds__(512, 1) void conv3d_wrw_wino4_kernel(const float* __restrict__ G,
                                                                 const float* __restrict__ Src,
                                                                 float* __restrict__ dW, WWP p) {
  __shared__ __attribute__((aligned(16))) float lds[2 * WW_BUF];

  const int t = threadIdx.x, lane = t & 63;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int wv = wave & 3;
  // (run of bricks, column group) of this workgroup.  The six column groups of a run read the SAME gradient / source bricks;
  // dispatched as (blockIdx.x, blockIdx.y) they landed on four XCDs (linear id % 8) and each XCD's L2 fetched the bricks
  // for itself: 3.4x the algorithmic bytes from HBM (profiles/r04_pmc_traffic.json).  So the linear id is re-read as
  // (XCD, slot) and an XCD takes a contiguous range of (run, group) tasks: the groups of a run share one L2.
  int bx = blockIdx.x, by = blockIdx.y;
  {
    const int total = gridDim.x * 6, lin = blockIdx.y * gridDim.x + blockIdx.x;
    const int c = lin & 7, j = lin >> 3;
    const int q8 = total >> 3, r8 = total & 7;                 // XCD c holds q8 + (c < r8) workgroups
    const int task = c * q8 + (c < r8 ? c : r8) + j;           // its tasks: a contiguous range, group-major inside a run
    bx = task / 6; by = task - bx * 6;
  }
  const int kz = by % 3, chalf = by / 3;  // column group: kz, source-channel half
  const int c0 = chalf * 32;
  const long long s0 = (long long)bx * p.spw;
  const long long s1 = min(s0 + (long long)p.spw, p.bricks);

  if (wave >= 4) {
    ww_loader_waves<(DBG == 1 ? 1 : 0)>(G, Src, p, lds, wv, lane, kz, c0, s0, s1);
    return;
  }

  const int l31 = lane & 31, kh = lane >> 5;
  const int m = wv >> 1;
  const int aBo = (m * 32 + l31) * WW_GP + 32 * kh;            // + h * 64 + 8 pr: dy[4j .. 4j + 3] of x-tiles j = 8 kh + 2 pr, + 1
  const int bPo = WW_NG + l31 * WW_CHS + 4 + 32 * kh;          // + (h + ky) * XP + 8 pr: (d1 .. d4) of the same two x-tiles
  const int bEo = bPo + ((wv & 1) ? 8 : -1);                   // d5 of the second tile (triple 1) or d0 of the first (triple 0)
  constexpr int ab = DBG >= 4 ? DBG - 4 : 0;  // measurement forms (FLOWSCI_WRW_WINO4_S3_AB): 1 no conversion, 2 no MFMAs

  f32x16 acc[3][3];  // [ky][component of the triple]
  auto kloop = [&](auto C3c) {
    constexpr int c3 = decltype(C3c)::value;
#pragma unroll
    for (int n = 0; n < 3; ++n)
#pragma unroll
      for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[n][c][r] = 0.f;

    // Registers (144 of 256 are accumulators) leave no room for a raw operand row: operands are consumed in PAIRS of
    // x-tiles -- two 16-byte reads (and the one neighbour value they do not hold), two transformed values, one word of
    // each of the three pieces.  A sub-step, between two scheduling barriers: the reads of the NEXT sub-step's pair,
    // this sub-step's MFMAs, and beside them the transform + split of its own pair (read a sub-step ago).
    w3_u32x4 paw[3][3], pbw[2][3];  // pieces: gradient sets by slot, source units by row parity; a word per pair of x-tiles
    w3_f32x4 xr[W4_PF + 1][2];      // raw pairs, read W4_PF sub-steps ahead of their job
    float er[W4_PF + 1] = {};
    auto piece = [](const w3_u32x4& w) __attribute__((always_inline)) { return __builtin_bit_cast(w3_bf16x8, w); };
    // job 1: source row `row` (0..3 of the staged rows y - 1 .. y + 2), job 2: gradient row `row`; pair pr into `slot`
    auto load = [&](const float* base, int job, int row, int c, int pr, int slot) __attribute__((always_inline)) {
      const float* q = base + (job == 1 ? bPo + row * WW_XP : aBo + row * 64) + 8 * pr;
      xr[slot][0] = *reinterpret_cast<const w3_f32x4*>(q);
      xr[slot][1] = *reinterpret_cast<const w3_f32x4*>(q + 4);
      if (job == 1 && (c3 == 0 ? c == 0 : c == 2)) er[slot] = base[bEo + row * WW_XP + 8 * pr];  // (d0 / d5: these components only)
    };
    auto tf_b = [&](const w3_f32x4& d, float e, int c) __attribute__((always_inline)) {  // e: d0 (triple 0) or d5 (triple 1)
      const float d1 = d[0], d2 = d[1], d3 = d[2], d4 = d[3];
      if (c3 == 0) return c == 0 ? fmaf(4.f, e, fmaf(-5.f, d2, d4)) : c == 1 ? fmaf(-4.f, d1 + d2, d3 + d4) : fmaf(4.f, d1 - d2, d4 - d3);
      const float p31 = d3 - d1, r42 = d4 - d2;
      return c == 0 ? fmaf(2.f, p31, r42) : c == 1 ? fmaf(-2.f, p31, r42) : fmaf(4.f, d1, fmaf(-5.f, d3, e));
    };
    auto tf_a = [&](const w3_f32x4& a, int c) __attribute__((always_inline)) {
      if (c3 == 0) {
        const float s02 = a[0] + a[2], s13 = a[1] + a[3];
        return c == 0 ? a[0] : c == 1 ? s02 + s13 : s02 - s13;
      }
      const float e = fmaf(4.f, a[2], a[0]), o = fmaf(8.f, a[3], 2.f * a[1]);
      return c == 0 ? e + o : c == 1 ? e - o : a[3];
    };
    auto use = [&](int job, int row, int c, int pr, int slot) __attribute__((always_inline)) {
      asm volatile("" : "+v"(xr[slot][0]), "+v"(xr[slot][1]));  // (read a sub-step ago: nothing of it is consumed before this point)
      float v0, v1;
      if (job == 1) {
        v0 = tf_b(xr[slot][0], c3 ? xr[slot][1][0] : er[slot], c);
        v1 = tf_b(xr[slot][1], c3 ? er[slot] : xr[slot][0][3], c);
      } else {
        v0 = tf_a(xr[slot][0], c); v1 = tf_a(xr[slot][1], c);
      }
      // (opaque: the SLP vectoriser would grow its tree from the bf16 pairs into the transforms of two x-tiles, whose
      // operands sit in different register quads -- three moves per packed operation; and the split stays in its sub-step)
      asm volatile("" : "+v"(v0), "+v"(v1));
      unsigned w0, w1, w2;
      w3_split2<true>(v0, v1, w0, w1, w2, ab);
      w3_u32x4(&w)[3] = job == 1 ? pbw[row & 1] : paw[(2 * c + row) % 3];
      w[0][pr] = w0; w[1][pr] = w1; w[2][pr] = w2;
    };
    constexpr int PA[6] = {2, 0, 1, 1, 0, 0}, PB[6] = {0, 2, 1, 0, 1, 0};  // the six products, small terms first

    __builtin_amdgcn_s_barrier();  // brick s0 has landed
    if (DBG != 2 && s0 < s1) {     // (once per workgroup, nothing beside it: gradient sets (0, 0), (1, 0), source unit (0, 0))
#pragma unroll
      for (int k = 0; k < 12; ++k) {
        load(lds, k < 4 ? 1 : 2, k < 8 ? 0 : 1, 0, k & 3, 0);
        use(k < 4 ? 1 : 2, k < 8 ? 0 : 1, 0, k & 3, 0);
      }
#pragma unroll
      for (int k = 0; k < W4_PF; ++k) {
        const W4Step f = w4_step(k);
        load(lds, f.job, f.jr, f.jc, f.jp, k);
      }
    }
    int buf = 0;
    for (long long st = s0; st < s1; ++st) {
      const float* base = lds + buf * WW_BUF;
      const float* nbase = lds + (buf ^ 1) * WW_BUF;
      const bool more = st + 1 < s1;
      auto substep = [&](auto Sc) __attribute__((always_inline)) {
        constexpr int s = decltype(Sc)::value;
        constexpr W4Step x = w4_step(s), y = w4_step((s + W4_PF) % 72);
        constexpr int ys = (s + W4_PF) % (W4_PF + 1), xs = s % (W4_PF + 1);
        __builtin_amdgcn_sched_barrier(0);
        if (s == W4_BARRIER_STEP) {  // every read of `buf` has been issued: once they are back, the next brick has landed
          asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
          __builtin_amdgcn_s_barrier();
        }
        if (!(y.jn || s + W4_PF >= 72)) load(base, y.job, y.jr, y.jc, y.jp, ys);
        else if (more) load(nbase, y.job, y.jr, y.jc, y.jp, ys);
        auto mfma = [&](int i) __attribute__((always_inline)) {
          if (i >= x.m1) return;
          const bool both = x.ur == 1 || x.ur == 2;
          const int h = both ? (i & 1) : (x.ur == 3 ? 1 : 0), q6 = both ? (i >> 1) : i;
          const w3_bf16x8 fa = piece(paw[(2 * x.uc + h) % 3][PA[q6]]), fb = piece(pbw[x.ur & 1][PB[q6]]);
          f32x16& d = acc[x.ur - h][x.uc];  // ky = source row - brick row
          if (ab & 2) asm volatile("" ::"v"(fa), "v"(fb));  // (measurement: no MFMAs, wrong by design)
          else d = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa, fb, d, 0, 0, 0);
        };
        // (the MFMAs of a sub-step are issued together at its head.  Dealing them between the three stages of the split, one in
        // front of each, was measured SLOWER: 0.577 against 0.534 ms per launch, profiles/r11_wrw_wino4_s3.txt)
#pragma unroll
        for (int i = x.m0; i < x.m1; ++i) mfma(i);
        if (!x.jn || more) use(x.job, x.jr, x.jc, x.jp, xs);
      };
      if (DBG == 2) __builtin_amdgcn_s_barrier();
      else w4_static_for(substep, std::make_integer_sequence<int, 72>{});
      buf ^= 1;
    }
  };
  if (wv & 1) kloop(std::integral_constant<int, 1>{}); else kloop(std::integral_constant<int, 0>{});

  // ---- epilogue.  G^T dU of the two component triples is combined in LDS (dg[co][ci][ky, kx], 72 KB of the now idle
  // staging buffers: the triple-0 waves store, the triple-1 waves add), then added to dW with float atomics whose lanes
  // walk dW's own order (see convwrwwino.hpp).
  float* dg = lds;
  constexpr int NDG = 64 * 32 * 9;
  static_assert(NDG <= 2 * WW_BUF, "the combine buffer fits the staging buffers");
  const bool second = (wv & 1) != 0;
#pragma unroll
  for (int pass = 0; pass < 2; ++pass) {
    if ((pass == 1) == second) {  // wave-uniform
#pragma unroll
      for (int n = 0; n < 3; ++n)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int co = m * 32 + (r & 3) + 8 * (r >> 2) + 4 * kh;
          float* dst = dg + (co * 32 + l31) * 9 + n * 3;  // lane stride 9 floats: conflict-free
          const float u0 = acc[n][0][r], u1 = acc[n][1][r], u2 = acc[n][2][r];
          if (!second) {  // (dU0, dU1, dU2)
            const float s12 = u1 + u2;
            dst[0] = fmaf(0.25f, u0, (-1.f / 6.f) * s12);
            dst[1] = (1.f / 6.f) * (u2 - u1);
            dst[2] = (-1.f / 6.f) * s12;
          } else {        // (dU3, dU4, dU5)
            const float s34 = u0 + u1;
            dst[0] += (1.f / 24.f) * s34;
            dst[1] += (1.f / 12.f) * (u0 - u1);
            dst[2] += fmaf(1.f / 6.f, s34, u2);
          }
        }
    }
    __builtin_amdgcn_s_barrier();  // (the loaders have left: the barrier counts the live waves only)
  }
  for (int i = t; i < NDG; i += 256) {
    const int co = i / 288, r2 = i - co * 288;
    const int ci = r2 / 9, k9 = r2 - ci * 9;
    float* q = dW + (size_t)bx * p.slab + ((size_t)co * 64 + c0 + ci) * 27 + kz * 9 + k9;
    if (p.slab) *q = dg[i]; else atomicAdd(q, dg[i]);
  }
}

#ifdef FS_ABLATION  // the fp32-MFMA form this kernel had before round 11 (FLOWSCI_WRW_WINO4_NO_S3=1: measurement builds only)
template <int DBG>
__global__ __launch_bounds__(512, 1) void conv3d_wrw_wino4_f32_kernel(const float* __restrict__ G,
                                                                 const float* __restrict__ Src,
                                                                 float* __restrict__ dW, WWP p) {
  __shared__ __attribute__((aligned(16))) float lds[2 * WW_BUF];

  const int t = threadIdx.x, lane = t & 63;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int wv = wave & 3;
  // (run of bricks, column group) of this workgroup.  The six column groups of a run read the SAME gradient / source bricks;
  // dispatched as (blockIdx.x, blockIdx.y) they landed on four XCDs (linear id % 8) and each XCD's L2 fetched the bricks
  // for itself: 3.4x the algorithmic bytes from HBM (profiles/r04_pmc_traffic.json).  So the linear id is re-read as
  // (XCD, slot) and an XCD takes a contiguous range of (run, group) tasks: the groups of a run share one L2.
  int bx = blockIdx.x, by = blockIdx.y;
  {
    const int total = gridDim.x * 6, lin = blockIdx.y * gridDim.x + blockIdx.x;
    const int c = lin & 7, j = lin >> 3;
    const int q8 = total >> 3, r8 = total & 7;                 // XCD c holds q8 + (c < r8) workgroups
    const int task = c * q8 + (c < r8 ? c : r8) + j;           // its tasks: a contiguous range, group-major inside a run
    bx = task / 6; by = task - bx * 6;
  }
  const int kz = by % 3, chalf = by / 3;  // column group: kz, source-channel half
  const int c0 = chalf * 32;
  const long long s0 = (long long)bx * p.spw;
  const long long s1 = min(s0 + (long long)p.spw, p.bricks);

  if (wave >= 4) {
    ww_loader_waves<DBG>(G, Src, p, lds, wv, lane, kz, c0, s0, s1);
    return;
  }

  const int l31 = lane & 31, kh = lane >> 5;
  const int m = wv >> 1;
  const int aBo = (m * 32 + l31) * WW_GP + 4 * kh;             // + h * 64 + 8 kk: dy[4j .. 4j + 3], x-tile j = 2 kk + kh
  const int bPo = WW_NG + l31 * WW_CHS + 4 + 4 * kh;           // + (h + ky) * XP + 8 kk: (d1 .. d4)
  const int bEo = bPo + ((wv & 1) ? 4 : -1);                   // d5 (triple 1) or d0 (triple 0)

  f32x16 acc[3][3];  // [ky][component of the triple]
  auto kloop = [&](auto C3c) {
    constexpr int c3 = decltype(C3c)::value;
#pragma unroll
    for (int n = 0; n < 3; ++n)
#pragma unroll
      for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[n][c][r] = 0.f;

    __builtin_amdgcn_s_barrier();  // brick s0 has landed
    int buf = 0;
    for (long long st = s0; st < s1; ++st) {
      const float* base = lds + buf * WW_BUF;
      // reduction step s = 8 h + kk: x-tiles 2 kk + kh of brick row h
      auto lds_ops = [&](int s, float4& a, float4 (&bp)[3], float (&be)[3]) {
        const int h = s >> 3, kk = s & 7;
        a = *reinterpret_cast<const float4*>(base + aBo + h * 64 + 8 * kk);
#pragma unroll
        for (int n = 0; n < 3; ++n) {
          bp[n] = *reinterpret_cast<const float4*>(base + bPo + (h + n) * WW_XP + 8 * kk);
          be[n] = base[bEo + (h + n) * WW_XP + 8 * kk];
        }
      };
      auto mma = [&](const float4& a, const float4 (&bp)[3], const float (&be)[3]) {
        float am[3];
        if (c3 == 0) {
          const float s02 = a.x + a.z, s13 = a.y + a.w;
          am[0] = a.x; am[1] = s02 + s13; am[2] = s02 - s13;
        } else {
          const float e = fmaf(4.f, a.z, a.x), o = fmaf(8.f, a.w, 2.f * a.y);
          am[0] = e + o; am[1] = e - o; am[2] = a.w;
        }
#pragma unroll
        for (int n = 0; n < 3; ++n) {
          const float d1 = bp[n].x, d2 = bp[n].y, d3 = bp[n].z, d4 = bp[n].w;
          float v[3];
          if (c3 == 0) {
            v[0] = fmaf(4.f, be[n], fmaf(-5.f, d2, d4));
            v[1] = fmaf(-4.f, d1 + d2, d3 + d4);
            v[2] = fmaf(4.f, d1 - d2, d4 - d3);
          } else {
            const float p31 = d3 - d1, r42 = d4 - d2;
            v[0] = fmaf(2.f, p31, r42);
            v[1] = fmaf(-2.f, p31, r42);
            v[2] = fmaf(4.f, d1, fmaf(-5.f, d3, be[n]));
          }
#pragma unroll
          for (int c = 0; c < 3; ++c) acc[n][c] = __builtin_amdgcn_mfma_f32_32x32x2f32(am[c], v[c], acc[n][c], 0, 0, 0);
        }
      };
      float4 a0, a1, p0[3], p1[3];
      float e0[3], e1[3];
      if (DBG != 2) lds_ops(0, a0, p0, e0);
#pragma unroll
      for (int q = 0; q < (DBG == 2 ? 0 : 16); q += 2) {
        lds_ops(q + 1, a1, p1, e1);
        __builtin_amdgcn_sched_barrier(0);
        mma(a0, p0, e0);
        if (q + 2 < 16) lds_ops(q + 2, a0, p0, e0);
        __builtin_amdgcn_sched_barrier(0);
        mma(a1, p1, e1);
      }
      __builtin_amdgcn_s_barrier();  // the next brick has landed, everyone is done reading `buf`
      buf ^= 1;
    }
  };
  if (wv & 1) kloop(std::integral_constant<int, 1>{}); else kloop(std::integral_constant<int, 0>{});

  // ---- epilogue.  G^T dU of the two component triples is combined in LDS (dg[co][ci][ky, kx], 72 KB of the now idle
  // staging buffers: the triple-0 waves store, the triple-1 waves add), then added to dW with float atomics whose lanes
  // walk dW's own order (see convwrwwino.hpp).
  float* dg = lds;
  constexpr int NDG = 64 * 32 * 9;
  static_assert(NDG <= 2 * WW_BUF, "the combine buffer fits the staging buffers");
  const bool second = (wv & 1) != 0;
#pragma unroll
  for (int pass = 0; pass < 2; ++pass) {
    if ((pass == 1) == second) {  // wave-uniform
#pragma unroll
      for (int n = 0; n < 3; ++n)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int co = m * 32 + (r & 3) + 8 * (r >> 2) + 4 * kh;
          float* dst = dg + (co * 32 + l31) * 9 + n * 3;  // lane stride 9 floats: conflict-free
          const float u0 = acc[n][0][r], u1 = acc[n][1][r], u2 = acc[n][2][r];
          if (!second) {  // (dU0, dU1, dU2)
            const float s12 = u1 + u2;
            dst[0] = fmaf(0.25f, u0, (-1.f / 6.f) * s12);
            dst[1] = (1.f / 6.f) * (u2 - u1);
            dst[2] = (-1.f / 6.f) * s12;
          } else {        // (dU3, dU4, dU5)
            const float s34 = u0 + u1;
            dst[0] += (1.f / 24.f) * s34;
            dst[1] += (1.f / 12.f) * (u0 - u1);
            dst[2] += fmaf(1.f / 6.f, s34, u2);
          }
        }
    }
    __builtin_amdgcn_s_barrier();  // (the loaders have left: the barrier counts the live waves only)
  }
  for (int i = t; i < NDG; i += 256) {
    const int co = i / 288, r2 = i - co * 288;
    const int ci = r2 / 9, k9 = r2 - ci * 9;
    float* q = dW + (size_t)bx * p.slab + ((size_t)co * 64 + c0 + ci) * 27 + kz * 9 + k9;
    if (p.slab) *q = dg[i]; else atomicAdd(q, dg[i]);
  }
}
#endif  // FS_ABLATION

inline bool wrw_wino4_ok(const WP& w, const float* g, const float* src, int kernel, int stride) {
  static const bool off = FS_AB_ENV("FLOWSCI_WRW_NO_WINO4");
  return !off && wrw_wino_ok(w, g, src, kernel, stride);  // same shapes, same bricks
}

inline int launch_wrw_wino4(const float* G, const float* Src, float* dW, const WP& w, hipStream_t st, const WDet* det = nullptr) {
  WWP p;
  p.B = w.B; p.D = w.Do; p.H = w.Ho; p.W = w.Wo;
  p.by = w.Ho / WW_TY;
  p.bricks = (long long)w.B * w.Do * p.by * (w.Wo / 64);
  const long long slabs = 42;  // x 6 column groups = 252 workgroups: one per CU
  long long spw = (p.bricks + slabs - 1) / slabs;
  p.spw = (int)spw;
  const long long gx = (p.bricks + spw - 1) / spw;
  float* out;
  const long long dwf = 64ll * 64 * 27;
  const int drc = wrw_det_begin(det, gx, dwf, dW, &out, &p.slab);
  if (drc >= 0) return drc;
  float* const real = dW;
  dW = out;
#ifdef FS_ABLATION  // the fp32-MFMA form, and instantiations that SKIP work (wrong results by design): measurement builds only
  static const int dbg = (int)FS_AB_ENV_LL("FLOWSCI_WINO_DBG", 0);
  static const bool no_s3 = FS_AB_ENV("FLOWSCI_WRW_WINO4_NO_S3");
  static const int s3_ab = (int)FS_AB_ENV_LL("FLOWSCI_WRW_WINO4_S3_AB", 0);  // 1: no conversion, 2: no MFMAs
  const dim3 grid((unsigned)gx, 6, 1);
#define W4_LAUNCH(kern) hipLaunchKernelGGL(kern, grid, dim3(512), 0, st, G, Src, dW, p)
  if (no_s3) {
    if (dbg == 1) W4_LAUNCH(conv3d_wrw_wino4_f32_kernel<1>);
    else if (dbg == 2) W4_LAUNCH(conv3d_wrw_wino4_f32_kernel<2>);
    else W4_LAUNCH(conv3d_wrw_wino4_f32_kernel<0>);
  } else if (dbg == 1) W4_LAUNCH(conv3d_wrw_wino4_kernel<1>);
  else if (dbg == 2) W4_LAUNCH(conv3d_wrw_wino4_kernel<2>);
  else if ((s3_ab & 3) == 1) W4_LAUNCH(conv3d_wrw_wino4_kernel<5>);  // (compile-time forms: <0> is the product's code)
  else if ((s3_ab & 3) == 2) W4_LAUNCH(conv3d_wrw_wino4_kernel<6>);
  else if ((s3_ab & 3) == 3) W4_LAUNCH(conv3d_wrw_wino4_kernel<7>);
  else
#undef W4_LAUNCH
#endif
    hipLaunchKernelGGL(conv3d_wrw_wino4_kernel<0>, dim3((unsigned)gx, 6, 1), dim3(512), 0, st, G, Src, dW, p);
  wrw_det_end(det, gx, dwf, real, st);
  FS_LAUNCH_CHECK();
  return FS_OK;
}
