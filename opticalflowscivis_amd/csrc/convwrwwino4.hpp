// convwrwwino4.hpp -- weight gradient of the 64-channel k3 s1 p1 trunk convolutions in the 1-D Winograd F(4,3) domain
// of convwino4.hpp: HALF the matrix-core work of the direct form (convwrwwino.hpp's F(2,3): two thirds).  Included
// inside convwrw.hip's anonymous namespace, after convwrwwino.hpp (same grid and brick runs; its loader waves serve the
// ablation forms).
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
// The 36 accumulator tiles (2 row tiles x 3 ky x 6 components) of a workgroup's (64 co x 32 ci x one kz) share are dealt
// to its four matrix waves as (row tile m) x (component triple {0,1,2} / {3,4,5}): 9 tiles (144 VGPRs) per wave, every
// wave walks every gradient row of the workgroup's run.
//
// Round 11: the products run on the bf16 matrix cores in the split-operand form of convwrw_s3.hpp.  The TRANSFORMED
// values (A dy and B^T d, formed in fp32 exactly as before) are split into three bf16 pieces each and six
// v_mfma_f32_32x32x16_bf16 products are accumulated in fp32, small terms first.  The 16 reduction elements of one MFMA
// are the 16 x-tiles of one row, the lane half kh holding tiles 8 kh .. 8 kh + 7: 54 MFMAs of 32 cycles per gradient row
// and wave.  +-inf splits into (inf, NaN, NaN): an entry the fp32 form gives as +-inf comes out NaN.
//
// Round 12: the SOURCE operand reaches the matrix waves as ready-made pieces.  Round 11's matrix waves transformed and
// split both operands, and their VALU stream was the kernel's period (matrix pipe 0.164 busy); two thirds of it was the
// source side, of which three quarters were repeats: the waves (m = 0, triple) and (m = 1, triple) did the same source
// work, and two of a brick's four source rows came back as the next brick's.  Now the loader waves -- idle but for a
// handful of LDS-DMA instructions -- transform and split every source row ONCE, a row per step, into a ring of piece
// rows in LDS; a matrix wave fetches a (row, component) unit's piece with one 16-byte read and keeps only the gradient's
// transform + split (24 of 72 pair-jobs per two rows).  The step schedule (ring slots, what is staged when, barriers) is
// convwrwwino4_sched.hpp; round 11's form stays in the ablation build (FLOWSCI_WRW_WINO4_MW=1), the fp32 form of round
// 10 too (FLOWSCI_WRW_WINO4_NO_S3=1).
#include "convwrwwino4_sched.hpp"

// ---- round 12 staging: one STEP = one gradient row (convwrwwino4_sched.hpp).  LDS, in floats:
constexpr int W4_GP = 64 + 4;                    // raw gradient row pitch per channel: 17 16-byte slots, conflict-free
constexpr int W4_GB = 64 * W4_GP;                // one raw gradient row [64 co][64 + 4]: 4352 = 17 LDS-DMA wave-instructions
constexpr int W4_SR = 32 * WW_XP;                // one raw source row [32 ci][4 + 64 + 4]: 2304 = 9 wave-instructions
constexpr int W4_S0 = 2 * W4_GB;                 // two gradient buffers, then two raw source buffers,
constexpr int W4_R0 = W4_S0 + 2 * W4_SR;         // then the piece ring:
constexpr int W4_CP = 32 * 2 * 4;                // one (component, piece) of a row: [ci][kh] entries of 16 bytes = four pairs of x-tiles
constexpr int W4_RR = 6 * 3 * W4_CP;             // one row of pieces [component][piece][ci][kh]: 4608 words
constexpr int W4_LDS = W4_R0 + (W4S_RING + 1) * W4_RR;  // 36352 floats = 142 KB
static_assert(W4_GB % 256 == 0 && W4_SR % 256 == 0, "the raw images end on a wave-instruction boundary");
static_assert(W4_LDS * 4 <= 160 * 1024, "gradient + raw source double buffers and the five-slot piece ring fit in LDS");

// the XCD re-mapping of the grid, see the kernel: linear workgroup id -> (run of bricks, column group)
__device__ __forceinline__ void w4_task(int& bx, int& by) {
  const int total = gridDim.x * 6, lin = blockIdx.y * gridDim.x + blockIdx.x;
  const int c = lin & 7, j = lin >> 3;
  const int q8 = total >> 3, r8 = total & 7;                 // XCD c holds q8 + (c < r8) workgroups
  const int task = c * q8 + (c < r8 ? c : r8) + j;           // its tasks: a contiguous range, group-major inside a run
  bx = task / 6; by = task - bx * 6;
}

// B^T d of one x-tile, all six components (the expressions of the matrix waves' tf_b, bit for bit: the ablation form
// conv3d_wrw_wino4_mw_kernel below still forms them there)
__device__ __forceinline__ void w4_tf_b6(float d0, float d1, float d2, float d3, float d4, float d5, float (&v)[6]) {
  const float p31 = d3 - d1, r42 = d4 - d2;
  v[0] = fmaf(4.f, d0, fmaf(-5.f, d2, d4));
  v[1] = fmaf(-4.f, d1 + d2, d3 + d4);
  v[2] = fmaf(4.f, d1 - d2, d4 - d3);
  v[3] = fmaf(2.f, p31, r42);
  v[4] = fmaf(-2.f, p31, r42);
  v[5] = fmaf(4.f, d1, fmaf(-5.f, d3, d5));
}

// The loader waves (4-7) of conv3d_wrw_wino4_kernel.  Per step (convwrwwino4_sched.hpp: w4s_fill) they move ONE raw
// gradient row [64][64] and ONE raw source row [32][4 + 64 + 4] into LDS with `buffer_load_dwordx4 ... lds`, and turn
// the raw source row that landed a step ago into the bf16 pieces of its six Winograd components in a ring slot: wave =
// 8 source channels, lane = (channel, lane half kh of the matrix waves, pair pr of x-tiles 8 kh + 2 pr, + 1).  The four
// pairs of a 16-byte ring entry are consecutive lanes and the entries of a wave are consecutive: every store of the wave
// is 64 consecutive words.  LD (measurement builds): 1 = no LDS-DMA, 3 = no transform / split / piece stores.
template <int LD>
__device__ __forceinline__ void w4_loader_waves(const float* __restrict__ G, const float* __restrict__ Src, const WWP& p,
                                                float* lds, int wv, int lane, int kz, int c0, long long q0, long long N) {
#if defined(__HIP_DEVICE_COMPILE__)
  __builtin_amdgcn_s_setprio(3);  // (few instructions per step: they should not queue behind the matrix wave's)
  constexpr int NGP = W4_GB / 256, NSP = W4_SR / 256;  // wave-instructions per image
  constexpr int NGW = (NGP + 3) / 4, NSW = (NSP + 3) / 4;
  const size_t vol = (size_t)p.D * p.H * p.W;
  const int bxn = p.W / 64;
  // piece k of loader wave wv fills the 16-byte slots 64 (wv + 4 k) + lane of an image
  unsigned goff[NGW], soff[NSW];
  int sx[NSW];
#pragma unroll
  for (int k = 0; k < NGW; ++k) {
    const int f = (64 * (wv + 4 * k) + lane) * 4;
    const int co = f / W4_GP, x = f - co * W4_GP;
    goff[k] = (f < W4_GB && x < 64) ? ((unsigned)co * (unsigned)vol + (unsigned)x) * 4u : DMA_OOB;
  }
#pragma unroll
  for (int k = 0; k < NSW; ++k) {
    const int f = (64 * (wv + 4 * k) + lane) * 4;
    const int c = f / WW_XP, x = f - c * WW_XP;  // staged column x = source column 64 xb - 4 + x
    soff[k] = f < W4_SR ? ((unsigned)c * (unsigned)vol + (unsigned)x) * 4u : DMA_OOB;
    sx[k] = x - 4;
  }
  unsigned* const ring = reinterpret_cast<unsigned*>(lds) + W4_R0;
#pragma unroll
  for (int k = 0; k < W4_RR / 256; ++k) ring[W4S_ZERO * W4_RR + 256 * k + 64 * wv + lane] = 0u;  // the padding row's pieces

  W4SRow rs = w4s_row(q0 - 1, p.D, p.H, bxn), rg = w4s_row(q0, p.D, p.H, bxn);  // next source row / gradient row to stage
  auto stage_src = [&](int buf) {
    const int sz = rs.z + kz - 1;
    const bool ok = w4s_live(rs, p.B) && sz >= 0 && sz < p.D;  // otherwise: all zeros
    const int ox0 = rs.xb * 64;
    const long long org = ok ? ((long long)sz * p.H + rs.y) * p.W + (ox0 - 4) : 0;
    __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc((void*)(Src + ((size_t)(ok ? rs.b : 0) * 64 + c0) * vol + org),
                                                                  (short)0, ok ? 0x7fffffff : 0, 0x00020000);
    float* dbase = lds + W4_S0 + buf * W4_SR;
#pragma unroll
    for (int k = 0; k < NSW; ++k)
      if (wv + 4 * k < NSP) {  // wave-uniform
        const int gx = ox0 + sx[k];
        const bool in = gx >= 0 && gx < p.W;  // W % 64 == 0: a 16-byte piece is in or out whole
        __builtin_amdgcn_raw_ptr_buffer_load_lds(r, (lds_ptr_t)(dbase + 256 * (wv + 4 * k)), 16, in ? soff[k] : DMA_OOB, 0, 0, 0);
      }
    rs = w4s_next(rs, p.D, p.H, bxn);
  };
  auto stage_grad = [&](int buf) {  // (only rows of the run's own steps: always inside the volume)
    __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc((void*)(G + (size_t)rg.b * 64 * vol), (short)0, 0x7fffffff, 0x00020000);
    const unsigned pos0 = (unsigned)(((rg.z * p.H + rg.y) * p.W + rg.xb * 64) * 4);
    float* dbase = lds + buf * W4_GB;
#pragma unroll
    for (int k = 0; k < NGW; ++k)
      if (wv + 4 * k < NGP)  // wave-uniform
        __builtin_amdgcn_raw_ptr_buffer_load_lds(r, (lds_ptr_t)(dbase + 256 * (wv + 4 * k)), 16, goff[k], pos0, 0, 0);
    rg = w4s_next(rg, p.D, p.H, bxn);
  };
  // the lane's two x-tiles in a raw source row: (d1 .. d4) of each, d0 of the first and d5 of the second beside them
  const int tro = (8 * wv + (lane >> 3)) * WW_XP + 4 + 32 * ((lane >> 2) & 1) + 8 * (lane & 3);
  auto transform = [&](int buf, int slot) {
    const float* q = lds + W4_S0 + buf * W4_SR + tro;
    const w3_f32x4 x0 = *reinterpret_cast<const w3_f32x4*>(q), x1 = *reinterpret_cast<const w3_f32x4*>(q + 4);
    const float e0 = q[-1], e1 = q[8];
    float v0[6], v1[6];
    w4_tf_b6(e0, x0[0], x0[1], x0[2], x0[3], x1[0], v0);
    w4_tf_b6(x0[3], x1[0], x1[1], x1[2], x1[3], e1, v1);
    unsigned* dst = ring + slot * W4_RR + 64 * wv + lane;
#pragma unroll
    for (int c = 0; c < 6; ++c) {
      unsigned w0, w1, w2;
      w3_split2<true>(v0[c], v1[c], w0, w1, w2, 0);
      dst[(3 * c + 0) * W4_CP] = w0; dst[(3 * c + 1) * W4_CP] = w1; dst[(3 * c + 2) * W4_CP] = w2;
    }
  };
  for (long long n = -W4S_PRO; n < N; ++n) {
    const W4SFill f = w4s_fill(n, N);
    if (LD != 1) {
      if (f.src) stage_src(f.src_buf);
      if (f.grad) stage_grad(f.grad_buf);
    }
    if (LD != 3 && f.tf) transform(f.tf_buf, f.tf_slot);
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
  }
#endif
}

// G^T dU of the two component triples is combined in LDS (dg[co][ci][ky, kx], 72 KB of the now idle staging buffers: the
// triple-0 waves store, the triple-1 waves add), then added to dW with float atomics whose lanes walk dW's own order
// (see convwrwwino.hpp).
__device__ __forceinline__ void w4_epilogue(const f32x16 (&acc)[3][3], float* dg, float* __restrict__ dW, const WWP& p, int t,
                                            int wv, int l31, int kh, int bx, int kz, int c0) {
  constexpr int NDG = 64 * 32 * 9;
  const int m = wv >> 1;
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

template <class F, int... I>
__device__ __forceinline__ void w4_static_for(F&& f, std::integer_sequence<int, I...>) {
  (f(std::integral_constant<int, I>{}), ...);
}

// DBG (measurement builds): 1 = loaders without LDS-DMA, 3 = loaders without transform / split / piece stores (the matrix
// waves read whatever the ring holds), 2 = the matrix waves keep only the barriers, 5 / 6 / 7 = the matrix waves without
// the gradient's conversion / without MFMAs / without both.  All but <0> give wrong results by design.
template <int DBG>
__global__ __launch_bounds__(512, 1) void conv3d_wrw_wino4_kernel(const float* __restrict__ G,
                                                                 const float* __restrict__ Src,
                                                                 float* __restrict__ dW, WWP p) {
  __shared__ __attribute__((aligned(16))) float lds[W4_LDS];

  const int t = threadIdx.x, lane = t & 63;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int wv = wave & 3;
  // (run of bricks, column group) of this workgroup.  The six column groups of a run read the SAME gradient / source rows;
  // dispatched as (blockIdx.x, blockIdx.y) they landed on four XCDs (linear id % 8) and each XCD's L2 fetched the bricks
  // for itself: 3.4x the algorithmic bytes from HBM (profiles/r04_pmc_traffic.json).  So the linear id is re-read as
  // (XCD, slot) and an XCD takes a contiguous range of (run, group) tasks: the groups of a run share one L2.
  int bx, by;
  w4_task(bx, by);
  const int kz = by % 3, chalf = by / 3;  // column group: kz, source-channel half
  const int c0 = chalf * 32;
  const long long s0 = (long long)bx * p.spw;
  const long long s1 = min(s0 + (long long)p.spw, p.bricks);
  const long long q0 = 2 * s0, N = w4s_steps(s1 > s0 ? s1 - s0 : 0);  // the run's steps: global q0 .. q0 + N - 1

  if (wave >= 4) {
    w4_loader_waves<(DBG == 1 || DBG == 3 ? DBG : 0)>(G, Src, p, lds, wv, lane, kz, c0, q0, N);
    return;
  }

  const int l31 = lane & 31, kh = lane >> 5;
  const int m = wv >> 1;
  const int aBo = (m * 32 + l31) * W4_GP + 32 * kh;            // + 8 pr: dy[4j .. 4j + 3] of x-tiles j = 8 kh + 2 pr, + 1
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

    // A step's work on this wave: per component c of the triple, the transform + split of the gradient row (four JOBS of
    // one pair of x-tiles each: two 16-byte reads, two transformed values, one word of each of the three pieces) and three
    // UNITS (c, ky) of six MFMAs whose source pieces come ready-made from the ring, three 16-byte reads per unit.  Two
    // steps are unrolled into 36 SUB-STEPS of three MFMAs, so that the piece registers alternate statically: sub-step
    // i = 0 .. 17 of a step is the half i & 1 of unit u = i / 2 = 3 c + ky.  Beside its MFMAs a sub-step reads the pieces of
    // the next unit (even i) and runs one job of the next component (i % 6 = 2 .. 5, its operands read a sub-step before).
    w3_u32x4 paw[2][3], pbw[2][3];  // pieces: gradient by component parity, source by unit parity; a word per pair of x-tiles
    w3_f32x4 xr[2][2];              // raw gradient pairs, read a sub-step ahead of their job
    auto piece = [](const w3_u32x4& w) __attribute__((always_inline)) { return __builtin_bit_cast(w3_bf16x8, w); };
    auto load = [&](int gbuf, int pr, int slot) __attribute__((always_inline)) {
      const float* q = lds + gbuf * W4_GB + aBo + 8 * pr;
      xr[slot][0] = *reinterpret_cast<const w3_f32x4*>(q);
      xr[slot][1] = *reinterpret_cast<const w3_f32x4*>(q + 4);
    };
    auto tf_a = [&](const w3_f32x4& a, int c) __attribute__((always_inline)) {
      if (c3 == 0) {
        const float s02 = a[0] + a[2], s13 = a[1] + a[3];
        return c == 0 ? a[0] : c == 1 ? s02 + s13 : s02 - s13;
      }
      const float e = fmaf(4.f, a[2], a[0]), o = fmaf(8.f, a[3], 2.f * a[1]);
      return c == 0 ? e + o : c == 1 ? e - o : a[3];
    };
    auto use = [&](int c, int pr, int slot, w3_u32x4 (&w)[3]) __attribute__((always_inline)) {
      asm volatile("" : "+v"(xr[slot][0]), "+v"(xr[slot][1]));  // (read a sub-step ago: nothing of it is consumed before this point)
      float v0 = tf_a(xr[slot][0], c), v1 = tf_a(xr[slot][1], c);
      // (opaque: keeps the SLP vectoriser out of the transforms of two x-tiles, and the split in its sub-step)
      asm volatile("" : "+v"(v0), "+v"(v1));
      unsigned w0, w1, w2;
      w3_split2<true>(v0, v1, w0, w1, w2, ab);
      w[0][pr] = w0; w[1][pr] = w1; w[2][pr] = w2;
    };
    // the lane's entry (ci = l31, kh) of the triple's first component in ring slot 0
    const unsigned* const ringw = reinterpret_cast<const unsigned*>(lds) + W4_R0 + (2 * l31 + kh) * 4 + c3 * 9 * W4_CP;
    auto pieces = [&](int slot, int c, w3_u32x4 (&w)[3]) __attribute__((always_inline)) {
      const unsigned* q = ringw + slot * W4_RR + c * 3 * W4_CP;
#pragma unroll
      for (int pc = 0; pc < 3; ++pc) w[pc] = *reinterpret_cast<const w3_u32x4*>(q + pc * W4_CP);
    };
    constexpr int PA[6] = {2, 0, 1, 1, 0, 0}, PB[6] = {0, 2, 1, 0, 1, 0};  // the six products, small terms first
    // the matrix waves' barrier of a step sits in front of sub-step W4_BAR: every read of the step's gradient row and of
    // its ky = 0 slot -- what the loaders overwrite during the NEXT step -- has been issued by then (the pieces of unit
    // (2, 0) in sub-step 10, the last job's operands in sub-step 10), and the first read of the next step's gradient row
    // (sub-step 13) and of its new ring row (ky = 2: the next step's sub-step 2) follow it
    constexpr int W4_BAR = 13;

#pragma unroll
    for (int k = 0; k < W4S_PRO; ++k) __builtin_amdgcn_s_barrier();  // rows 0 .. 2 are pieces, gradient row 0 has landed
    int y = (int)(q0 % p.H);  // of step n; q0 and H are even: so are n and y at the head of a pair of steps
    if (DBG != 2 && N > 0) {  // (once per workgroup, nothing beside it: the first component's gradient pieces, the first unit's source pieces)
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        load(w4s_grad_buf(0), k, 0);
        use(0, k, 0, paw[0]);
      }
      pieces(w4s_read_slot(0, 0, y, p.H), 0, pbw[0]);
    }
    for (long long n = 0; n < N; n += 2) {
      const bool more = n + 2 < N;
      const int y2 = y + 2 == p.H ? 0 : y + 2;
      const int slot[3][3] = {{w4s_read_slot(n, 0, y, p.H), w4s_read_slot(n, 1, y, p.H), w4s_read_slot(n, 2, y, p.H)},
                              {w4s_read_slot(n + 1, 0, y + 1, p.H), w4s_read_slot(n + 1, 1, y + 1, p.H), w4s_read_slot(n + 1, 2, y + 1, p.H)},
                              {w4s_read_slot(n + 2, 0, y2, p.H), 0, 0}};
      auto substep = [&](auto Sc) __attribute__((always_inline)) {
        constexpr int S = decltype(Sc)::value;
        constexpr int h = S / 18, i = S % 18, u = i / 2, c = u / 3, ky = u % 3, t6 = i % 6;
        constexpr int U = 9 * h + u, C = 3 * h + c;  // unit and component of the pair of steps: their parities pick the registers
        const bool next = h == 0 || more;            // there is a step after this one
        __builtin_amdgcn_sched_barrier(0);
        if (i == W4_BAR) {
          asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
          __builtin_amdgcn_s_barrier();
        }
        if ((i & 1) == 0) {
          if (u < 8) pieces(slot[h][(u + 1) % 3], (u + 1) / 3, pbw[(U + 1) & 1]);
          else if (next) pieces(slot[h + 1][0], 0, pbw[(U + 1) & 1]);
        }
        // component 2's jobs are the next step's component 0: the other gradient buffer, behind the barrier
        if (t6 >= 1 && t6 <= 4 && (c < 2 || next)) load(w4s_grad_buf(c < 2 ? h : h + 1), t6 - 1, (S + 1) & 1);
#pragma unroll
        for (int q6 = 3 * (i & 1); q6 < 3 * (i & 1) + 3; ++q6) {
          const w3_bf16x8 fa = piece(paw[C & 1][PA[q6]]), fb = piece(pbw[U & 1][PB[q6]]);
          if (ab & 2) asm volatile("" ::"v"(fa), "v"(fb));  // (measurement: no MFMAs, wrong by design)
          else acc[ky][c] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa, fb, acc[ky][c], 0, 0, 0);
        }
        if (t6 >= 2 && (c < 2 || next)) use((c + 1) % 3, t6 - 2, S & 1, paw[(C + 1) & 1]);
      };
      if (DBG == 2) { __builtin_amdgcn_s_barrier(); __builtin_amdgcn_s_barrier(); }
      else w4_static_for(substep, std::make_integer_sequence<int, 36>{});
      y = y2;
    }
  };
  if (wv & 1) kloop(std::integral_constant<int, 1>{}); else kloop(std::integral_constant<int, 0>{});

  // (the last step's barrier is followed by reads of its ky = 1, 2 slots: every matrix wave is through with the ring and
  // the raw rows before the combine buffer is laid over them)
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  static_assert(64 * 32 * 9 <= W4_LDS, "the combine buffer fits the staging buffers");
  w4_epilogue(acc, lds, dW, p, t, wv, l31, kh, bx, kz, c0);
}

#ifdef FS_ABLATION  // round 11's form of the kernel: two-row bricks, raw source rows in LDS, BOTH operands transformed and
// split by the matrix waves (FLOWSCI_WRW_WINO4_MW=1: measurement builds only; convwrwwino.hpp's loaders and buffers)
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

template <int DBG>
__global__ __launch_bounds__(512, 1) void conv3d_wrw_wino4_mw_kernel(const float* __restrict__ G,
                                                                 const float* __restrict__ Src,
                                                                 float* __restrict__ dW, WWP p) {
  __shared__ __attribute__((aligned(16))) float lds[2 * WW_BUF];

  const int t = threadIdx.x, lane = t & 63;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int wv = wave & 3;
  int bx, by;  // (run of bricks, column group), see conv3d_wrw_wino4_kernel
  w4_task(bx, by);
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

  static_assert(64 * 32 * 9 <= 2 * WW_BUF, "the combine buffer fits the staging buffers");
  w4_epilogue(acc, lds, dW, p, t, wv, l31, kh, bx, kz, c0);
}
#endif  // FS_ABLATION (conv3d_wrw_wino4_mw_kernel)

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
  static const bool mw = FS_AB_ENV("FLOWSCI_WRW_WINO4_MW");  // round 11's form: both operands split on the matrix waves
  static const int s3_ab = (int)FS_AB_ENV_LL("FLOWSCI_WRW_WINO4_S3_AB", 0);  // 1: no conversion, 2: no MFMAs
  const dim3 grid((unsigned)gx, 6, 1);
#define W4_LAUNCH(kern) hipLaunchKernelGGL(kern, grid, dim3(512), 0, st, G, Src, dW, p)
  if (no_s3) {
    if (dbg == 1) W4_LAUNCH(conv3d_wrw_wino4_f32_kernel<1>);
    else if (dbg == 2) W4_LAUNCH(conv3d_wrw_wino4_f32_kernel<2>);
    else W4_LAUNCH(conv3d_wrw_wino4_f32_kernel<0>);
  } else if (mw) W4_LAUNCH(conv3d_wrw_wino4_mw_kernel<0>);
  else if (dbg == 1) W4_LAUNCH(conv3d_wrw_wino4_kernel<1>);  // 1: no LDS-DMA, 3: no source transform, 2: no matrix-wave work
  else if (dbg == 3) W4_LAUNCH(conv3d_wrw_wino4_kernel<3>);
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
