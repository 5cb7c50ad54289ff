// regions.hip -- connected regions of K flag maps and what a series' flows do to them:
//   fs_label_regions{2,3}d   connected components (face or full neighbourhood), label = 1 + smallest linear index
//   fs_region_stats{2,3}d    one row per region: node count, coordinate sums, bounding box, sums / extrema of weights
//   fs_region_follow{2,3}d   the label each foreground node is carried onto by its step flow
// include/flowsci_hip.h states the definitions; tests/regions_ref.py restates them and agrees exactly.
//
// Labelling is union-find with parent < child throughout, in three launches, so that kernel boundaries order the
// phases: (1) every workgroup labels one tile in LDS and writes parent[i] = global index of i's tile-local root (-1 on
// background); (2) foreground nodes on tile faces unite with their earlier neighbours in OTHER tiles -- every access
// to `parent` in that launch is an agent-scope atomic (relaxed load, fetch-min), because the eight XCDs' L2s are not
// coherent and other workgroups write the same words; (3) every node follows its parents to the root and writes
// root + 1 to `labels` (another array: nothing is compressed in place, so no workgroup reads what another writes in
// that launch) and roots are counted, one integer atomic per workgroup.  Every find / retry loop is capped by the
// step's node count; a loop that hits the cap sets bit 0 of `status` and leaves.
#include <limits.h>
#include "common.hpp"

namespace {

constexpr int NT = 256;
constexpr int TN = 2048;                 // nodes of a tile: 8 KB of LDS, 8 nodes per thread
constexpr int kStepsPerLaunch = 32768;   // blockIdx.y

template <int ND> struct Tile;
template <> struct Tile<2> { static constexpr int D = 1, H = FS_REGION_TILE2_H, W = FS_REGION_TILE2_W; };
template <> struct Tile<3> { static constexpr int D = FS_REGION_TILE3_D, H = FS_REGION_TILE3_H, W = FS_REGION_TILE3_W; };
static_assert(Tile<2>::D * Tile<2>::H * Tile<2>::W == TN && Tile<3>::D * Tile<3>::H * Tile<3>::W == TN, "tile size");
static_assert(Tile<2>::W == 64 && Tile<3>::W == 32, "a tile row is a wave or half a wave");

struct GP {
  long long sstride;  // step stride of the strided operand (elements)
  int P;              // nodes of a step
  int W, H, D, WH;
  int nW, nH;         // tiles along W and H
  int require, reject, full;
};

// rows (dz, dy) of the earlier half-neighbourhood, the node's own row excluded
__device__ __forceinline__ int n_rows(int nd, int full) { return nd == 2 ? 1 : full ? 4 : 2; }
__device__ __forceinline__ void row_of(int nd, int full, int r, int& dz, int& dy) {
  if (nd == 2 || r == 0) { dz = 0; dy = -1; return; }
  dz = -1;
  dy = full ? r - 2 : 0;
}

__device__ __forceinline__ void raise(int* status) { atomicOr(status, 1); }

// ---- (1) one tile in LDS ---------------------------------------------------------------------------------------------
__device__ __forceinline__ int lds_load(int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }

__device__ __forceinline__ int lds_find(int* p, int a, int cap, int* status) {
  for (int it = 0; it < cap; ++it) {
    const int n = lds_load(p + a);
    if (n == a) return a;
    a = n;  // n < a: parents strictly decrease
  }
  raise(status);
  return a;
}

__device__ __forceinline__ void lds_unite(int* p, int a, int b, int cap, int* status) {
  for (int it = 0; it < cap; ++it) {
    a = lds_find(p, a, cap, status);
    b = lds_find(p, b, cap, status);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = __hip_atomic_fetch_min(p + a, b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (old == a) return;
    a = old;  // somebody else hung a elsewhere meanwhile: unite what it points to now
  }
  raise(status);
}

template <int ND>
__global__ __launch_bounds__(NT) void label_tile_kernel(const unsigned char* __restrict__ mask, int* __restrict__ parent,
                                                        int* __restrict__ status, const GP f) {
  constexpr int TD = Tile<ND>::D, TH = Tile<ND>::H, TW = Tile<ND>::W;
  __shared__ int p[TN];
  const int k = blockIdx.y;
  int t = blockIdx.x;
  const int tx = t % f.nW;
  t /= f.nW;
  const int ty = t % f.nH, tz = t / f.nH;
  const int x0 = tx * TW, y0 = ty * TH, z0 = tz * TD;
  const unsigned char* __restrict__ m = mask + (size_t)k * f.sstride;
  int* __restrict__ par = parent + (size_t)k * f.P;
  const int lane = threadIdx.x & 63;
  const int ln = lane & (TW - 1), half = lane & ~(TW - 1);
  // foreground test; the x runs of a row come from one ballot: p[l] = first node of l's run
#pragma unroll
  for (int j = 0; j < TN / NT; ++j) {
    const int l = threadIdx.x + j * NT;
    const int lx = l % TW, ly = (l / TW) % TH, lz = l / (TW * TH);
    const int gx = x0 + lx, gy = y0 + ly, gz = z0 + lz;
    bool fg = false;
    if (gx < f.W && gy < f.H && gz < f.D) {
      const int v = m[((size_t)gz * f.H + gy) * f.W + gx];
      fg = (v & f.require) == f.require && (v & f.reject) == 0;
    }
    unsigned long long b = __ballot(fg) >> half;
    if (TW == 32) b &= 0xffffffffull;
    const unsigned long long below = ~b & ((1ull << ln) - 1ull);
    const int start = below ? 64 - __clzll((long long)below) : 0;
    p[l] = fg ? l - ln + start : -1;
  }
  __syncthreads();
  const int cap = TN;
  const int rows = n_rows(ND, f.full);
#pragma unroll 1
  for (int j = 0; j < TN / NT; ++j) {
    const int l = threadIdx.x + j * NT;
    if (lds_load(p + l) < 0) continue;
    const int lx = l % TW, ly = (l / TW) % TH, lz = l / (TW * TH);
    const bool left = lx > 0 && lds_load(p + l - 1) >= 0;
    for (int r = 0; r < rows; ++r) {
      int dz, dy;
      row_of(ND, f.full, r, dz, dy);
      const int cz = lz + dz, cy = ly + dy;
      if (cz < 0 || cy < 0 || cy >= TH) continue;
      const int c = (cz * TH + cy) * TW + lx;
      if (lds_load(p + c) >= 0) {
        // the left neighbour is in this node's run and, by induction along the run, joined to its own c
        if (!(left && lds_load(p + c - 1) >= 0)) lds_unite(p, l, c, cap, status);
      } else if (f.full) {  // c's neighbours along x are not joined through c
        if (lx > 0 && lds_load(p + c - 1) >= 0) lds_unite(p, l, c - 1, cap, status);
        if (lx + 1 < TW && lds_load(p + c + 1) >= 0) lds_unite(p, l, c + 1, cap, status);
      }
    }
  }
  __syncthreads();
#pragma unroll 1
  for (int j = 0; j < TN / NT; ++j) {
    const int l = threadIdx.x + j * NT;
    const int lx = l % TW, ly = (l / TW) % TH, lz = l / (TW * TH);
    const int gx = x0 + lx, gy = y0 + ly, gz = z0 + lz;
    if (gx >= f.W || gy >= f.H || gz >= f.D) continue;
    int g = -1;
    if (p[l] >= 0) {
      const int r = lds_find(p, l, cap, status);
      const int rx = r % TW, ry = (r / TW) % TH, rz = r / (TW * TH);
      g = ((z0 + rz) * f.H + (y0 + ry)) * f.W + (x0 + rx);  // below P < 2^31 - 1
    }
    par[((size_t)gz * f.H + gy) * f.W + gx] = g;
  }
}

// ---- (2) tile faces: agent-scope atomics only ------------------------------------------------------------------------
__device__ __forceinline__ int g_load(int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ __forceinline__ int g_find(int* p, int a, int cap, int* status) {
  for (int it = 0; it < cap; ++it) {
    const int n = g_load(p + a);
    if (n == a || n < 0) return a;  // (n < 0 cannot happen on a foreground chain: leave rather than index with it)
    a = n;
  }
  raise(status);
  return a;
}

__device__ __forceinline__ void g_unite(int* p, int a, int b, int cap, int* status) {
  for (int it = 0; it < cap; ++it) {
    a = g_find(p, a, cap, status);
    b = g_find(p, b, cap, status);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = __hip_atomic_fetch_min(p + a, b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (old == a) return;
    a = old;
  }
  raise(status);
}

template <int ND>
__global__ __launch_bounds__(NT) void label_border_kernel(int* parent, int* __restrict__ status, const GP f) {
  constexpr int TD = Tile<ND>::D, TH = Tile<ND>::H, TW = Tile<ND>::W;
  const long long q = (long long)blockIdx.x * NT + threadIdx.x;
  if (q >= f.P) return;
  const int i = (int)q;
  int* par = parent + (size_t)blockIdx.y * f.P;
  const int x = i % f.W, y = (i / f.W) % f.H, z = i / f.WH;
  const int lx = x % TW, ly = y % TH, lz = z % TD;
  const bool face = lx == 0 || ly == 0 || (ND == 3 && lz == 0) || (f.full && (lx == TW - 1 || ly == TH - 1));
  if (!face) return;
  if (g_load(par + i) < 0) return;
  const int cap = f.P;
  if (lx == 0 && x > 0 && g_load(par + i - 1) >= 0) g_unite(par, i, i - 1, cap, status);
  const int rows = n_rows(ND, f.full);
  for (int r = 0; r < rows; ++r) {
    int dz, dy;
    row_of(ND, f.full, r, dz, dy);
    const int cz = z + dz, cy = y + dy;
    if (cz < 0 || cy < 0 || cy >= f.H) continue;
    const bool cross = (dz < 0 && lz == 0) || (dy < 0 && ly == 0) || (dy > 0 && ly == TH - 1);
    const bool lo = f.full && x > 0 && (cross || lx == 0), hi = f.full && x + 1 < f.W && (cross || lx == TW - 1);
    if (!(cross || lo || hi)) continue;
    const int c = (cz * f.H + cy) * f.W + x;
    if (g_load(par + c) >= 0) {
      if (cross) g_unite(par, i, c, cap, status);  // (in this tile: joined in LDS, and c joins its own x neighbours)
    } else {
      if (lo && g_load(par + c - 1) >= 0) g_unite(par, i, c - 1, cap, status);
      if (hi && g_load(par + c + 1) >= 0) g_unite(par, i, c + 1, cap, status);
    }
  }
}

// ---- (3) roots to labels, roots counted ------------------------------------------------------------------------------
__global__ __launch_bounds__(NT) void label_flatten_kernel(const int* parent, int* __restrict__ labels,
                                                           int* __restrict__ n_regions, int* __restrict__ status,
                                                           int P) {
  __shared__ int cnt;
  if (threadIdx.x == 0) cnt = 0;
  __syncthreads();
  const long long q = (long long)blockIdx.x * NT + threadIdx.x;
  const int* par = parent + (size_t)blockIdx.y * P;
  bool root = false;
  if (q < P) {
    const int i = (int)q;
    int a = par[i];
    root = a == i;
    if (a >= 0) {
      int it = 0;
      for (; it < P; ++it) {
        const int n = par[a];
        if (n == a || n < 0) break;
        a = n;
      }
      if (it == P) raise(status);
    }
    labels[(size_t)blockIdx.y * P + i] = a + 1;  // background: -1 + 1
  }
  const int c = __popcll(__ballot(root));
  if ((threadIdx.x & 63) == 0 && c) atomicAdd(&cnt, c);
  __syncthreads();
  if (threadIdx.x == 0 && cnt) atomicAdd(n_regions + blockIdx.y, cnt);
}

int geometry(bool is3d, int D, int H, int W, GP& f) {
  if (W < 1 || H < 1 || D < 1) return FS_ERR_SHAPE;
  const long long P = (long long)D * H * W;
  if (P >= 0x7fffffffLL) return FS_ERR_SHAPE;
  f.P = (int)P;
  f.W = W; f.H = H; f.D = D;
  f.WH = (int)((long long)W * H);
  f.nW = fs::cdiv(W, is3d ? Tile<3>::W : Tile<2>::W);
  f.nH = fs::cdiv(H, is3d ? Tile<3>::H : Tile<2>::H);
  return FS_OK;
}

long long label_ws_bytes(bool is3d, int K, int D, int H, int W) {
  GP f;
  const int rc = geometry(is3d, D, H, W, f);
  if (rc != FS_OK) return -rc;
  if (K < 1) return -FS_ERR_ARG;
  return (long long)K * f.P * (long long)sizeof(int);
}

int label(bool is3d, const unsigned char* mask, int K, int D, int H, int W, long long sstride, int require, int reject,
          int conn, int* labels, int* n_regions, int* status, int* ws, fs_stream_t stream) {
  FS_ENTER();
  FS_REQUIRE_PTR(mask); FS_REQUIRE_PTR(labels); FS_REQUIRE_PTR(n_regions); FS_REQUIRE_PTR(status); FS_REQUIRE_PTR(ws);
  GP f;
  const int rc = geometry(is3d, D, H, W, f);
  if (rc != FS_OK) return rc;
  if (sstride < f.P) return FS_ERR_SHAPE;
  if ((conn != 0 && conn != 1) || K < 1 || (require & ~255) || (reject & ~255)) return FS_ERR_ARG;
  f.sstride = sstride;
  f.require = require; f.reject = reject; f.full = conn;
  const hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(n_regions, 0, (size_t)K * sizeof(int), s) != hipSuccess) return FS_ERR_LAUNCH;
  if (hipMemsetAsync(status, 0, sizeof(int), s) != hipSuccess) return FS_ERR_LAUNCH;
  const unsigned tiles = (unsigned)((long long)f.nW * f.nH * (is3d ? fs::cdiv(D, Tile<3>::D) : 1));
  const unsigned blocks = (unsigned)fs::cdiv(f.P, NT);
  for (int k0 = 0; k0 < K; k0 += kStepsPerLaunch) {
    const unsigned kc = (unsigned)(K - k0 < kStepsPerLaunch ? K - k0 : kStepsPerLaunch);
    const unsigned char* mk = mask + (size_t)k0 * sstride;
    int* pk = ws + (size_t)k0 * f.P;
    if (is3d) {
      hipLaunchKernelGGL(label_tile_kernel<3>, dim3(tiles, kc), dim3(NT), 0, s, mk, pk, status, f);
      hipLaunchKernelGGL(label_border_kernel<3>, dim3(blocks, kc), dim3(NT), 0, s, pk, status, f);
    } else {
      hipLaunchKernelGGL(label_tile_kernel<2>, dim3(tiles, kc), dim3(NT), 0, s, mk, pk, status, f);
      hipLaunchKernelGGL(label_border_kernel<2>, dim3(blocks, kc), dim3(NT), 0, s, pk, status, f);
    }
    hipLaunchKernelGGL(label_flatten_kernel, dim3(blocks, kc), dim3(NT), 0, s, (const int*)pk,
                       labels + (size_t)k0 * f.P, n_regions + k0, status, f.P);
  }
  FS_LAUNCH_CHECK();
  return FS_OK;
}

// ---- region table ----------------------------------------------------------------------------------------------------
// fp32 <-> a signed integer with the same order (-0 below +0): integer atomic min / max are then exact
__device__ __forceinline__ int f2key(float v) {
  const int b = __float_as_int(v);
  return b >= 0 ? b : b ^ 0x7fffffff;
}
__device__ __forceinline__ float key2f(int k) { return __int_as_float(k >= 0 ? k : k ^ 0x7fffffff); }

__global__ __launch_bounds__(NT) void stats_init_kernel(long long R, int nd, int F, long long* __restrict__ count,
                                                        long long* __restrict__ csum, int* __restrict__ bbox,
                                                        double* __restrict__ wsum, int* __restrict__ wmin,
                                                        int* __restrict__ wmax) {
  const long long r = (long long)blockIdx.x * NT + threadIdx.x;
  if (r >= R) return;
  count[r] = 0;
  for (int a = 0; a < nd; ++a) {
    csum[r * nd + a] = 0;
    bbox[(r * 2 + 0) * nd + a] = INT_MAX;
    bbox[(r * 2 + 1) * nd + a] = INT_MIN;
  }
  for (int c = 0; c < F; ++c) {
    wsum[r * F + c] = 0.0;
    wmin[r * F + c] = INT_MAX;
    wmax[r * F + c] = INT_MIN;
  }
}

__global__ __launch_bounds__(NT) void stats_final_kernel(long long n, int* __restrict__ wmin, int* __restrict__ wmax) {
  const long long i = (long long)blockIdx.x * NT + threadIdx.x;
  if (i >= n) return;
  wmin[i] = __float_as_int(key2f(wmin[i]));
  wmax[i] = __float_as_int(key2f(wmax[i]));
}

// One thread per node and round, a wave = 64 consecutive nodes, a workgroup = kStatRounds * NT consecutive nodes.  A run
// = consecutive lanes of one row of the grid with the same table row: its count, coordinate sums and box follow from its
// first node and its length, its weights are reduced by a segmented butterfly, and the run's first lane alone goes on.
// It adds the run to the workgroup's table in LDS (kSlots direct-mapped rows, claimed by one compare-and-swap: no
// waiting); a run whose slot belongs to another row goes to global memory at once.  At the end every claimed slot is
// added to global memory once: a large region costs one set of global atomics per workgroup, not per run.
constexpr int kStatRounds = 8;
constexpr int kSlots = 64;

template <int ND>
__global__ __launch_bounds__(NT) void stats_kernel(const int* __restrict__ labels, const int* __restrict__ rank,
                                                   const long long* __restrict__ offsets,
                                                   const float* __restrict__ weights, int F, long long R,
                                                   long long* __restrict__ count, long long* __restrict__ csum,
                                                   int* __restrict__ bbox, double* __restrict__ wsum,
                                                   int* __restrict__ wmin, int* __restrict__ wmax, const GP f) {
  __shared__ long long s_key[kSlots];
  __shared__ unsigned long long s_cnt[kSlots];
  __shared__ unsigned long long s_sum[kSlots][3];
  __shared__ int s_min[kSlots][3], s_max[kSlots][3];
  __shared__ double s_w[kSlots][FS_REGION_MAX_WEIGHTS];
  __shared__ int s_wmin[kSlots][FS_REGION_MAX_WEIGHTS], s_wmax[kSlots][FS_REGION_MAX_WEIGHTS];
  if (threadIdx.x < kSlots) {
    const int t = threadIdx.x;
    s_key[t] = -1;
    s_cnt[t] = 0;
    for (int a = 0; a < 3; ++a) { s_sum[t][a] = 0; s_min[t][a] = INT_MAX; s_max[t][a] = INT_MIN; }
    for (int c = 0; c < FS_REGION_MAX_WEIGHTS; ++c) { s_w[t][c] = 0.0; s_wmin[t][c] = INT_MAX; s_wmax[t][c] = INT_MIN; }
  }
  __syncthreads();
  const int k = blockIdx.y;
  const int lane = threadIdx.x & 63;
  const long long lo = offsets[k], hi = offsets[k + 1];
#pragma unroll 1
  for (int round = 0; round < kStatRounds; ++round) {
    const long long q = ((long long)blockIdx.x * kStatRounds + round) * NT + threadIdx.x;
    const bool in = q < f.P;
    const int i = in ? (int)q : 0;
    long long row = -1;
    if (in) {
      const int L = labels[(size_t)k * f.P + i];
      if (L > 0 && L <= f.P) {
        const long long r = rank[(size_t)k * f.P + (L - 1)];
        if (r >= 0 && lo >= 0 && lo + r < hi && hi <= R) row = lo + r;  // anything else: not a row of this table
      }
    }
    const int x = i % f.W, y = (i / f.W) % f.H, z = i / f.WH;
    const long long prev = __shfl_up(row, 1, 64);
    const bool head = row >= 0 && (lane == 0 || x == 0 || prev != row);
    const unsigned long long brk = __ballot(head || row < 0);
    const unsigned long long above = lane == 63 ? 0ull : brk & ~((2ull << lane) - 1ull);
    const int end = above ? __ffsll((long long)above) - 1 : 64;
    const int n = end - lane;
    const int slot = (int)((unsigned long long)row & (kSlots - 1));
    bool mine = false;  // the run goes to the workgroup's table
    if (head) {
      const long long old = atomicCAS((unsigned long long*)&s_key[slot], (unsigned long long)-1LL, (unsigned long long)row);
      mine = old == -1LL || old == row;
      const int c[3] = {x, y, z};
      if (mine) atomicAdd(&s_cnt[slot], (unsigned long long)n);
      else atomicAdd((unsigned long long*)(count + row), (unsigned long long)n);
#pragma unroll
      for (int a = 0; a < ND; ++a) {
        const int ax = ND - 1 - a;  // column of axis a in the tensor's order
        const unsigned long long s =
            (unsigned long long)(a == 0 ? (long long)n * x + (long long)n * (n - 1) / 2 : (long long)n * c[a]);
        const int cmax = a == 0 ? x + n - 1 : c[a];
        if (mine) {
          atomicAdd(&s_sum[slot][ax], s);
          atomicMin(&s_min[slot][ax], c[a]);
          atomicMax(&s_max[slot][ax], cmax);
        } else {
          atomicAdd((unsigned long long*)(csum + row * ND + ax), s);
          atomicMin(bbox + (row * 2 + 0) * ND + ax, c[a]);
          atomicMax(bbox + (row * 2 + 1) * ND + ax, cmax);
        }
      }
    }
    for (int c = 0; c < F; ++c) {
      const float w = row >= 0 ? weights[((size_t)k * F + c) * f.P + i] : 0.f;
      double s = (double)w;
      int mn = f2key(w), mx = mn;  // the extrema travel as their integer images: exact, -0 below +0
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const double so = __shfl_down(s, o, 64);
        const int no = __shfl_down(mn, o, 64), xo = __shfl_down(mx, o, 64);
        if (lane + o < end) { s += so; mn = no < mn ? no : mn; mx = xo > mx ? xo : mx; }
      }
      if (head) {
        if (mine) {
          atomicAdd(&s_w[slot][c], s);
          atomicMin(&s_wmin[slot][c], mn);
          atomicMax(&s_wmax[slot][c], mx);
        } else {
          unsafeAtomicAdd(wsum + row * F + c, s);
          atomicMin(wmin + row * F + c, mn);
          atomicMax(wmax + row * F + c, mx);
        }
      }
    }
  }
  __syncthreads();
  if (threadIdx.x < kSlots) {
    const int t = threadIdx.x;
    const long long row = s_key[t];
    if (row >= 0) {  // (a claimed slot's row was checked against R by the lane that claimed it)
      atomicAdd((unsigned long long*)(count + row), s_cnt[t]);
      for (int ax = 0; ax < ND; ++ax) {
        atomicAdd((unsigned long long*)(csum + row * ND + ax), s_sum[t][ax]);
        atomicMin(bbox + (row * 2 + 0) * ND + ax, s_min[t][ax]);
        atomicMax(bbox + (row * 2 + 1) * ND + ax, s_max[t][ax]);
      }
      for (int c = 0; c < F; ++c) {
        unsafeAtomicAdd(wsum + row * F + c, s_w[t][c]);
        atomicMin(wmin + row * F + c, s_wmin[t][c]);
        atomicMax(wmax + row * F + c, s_wmax[t][c]);
      }
    }
  }
}

int stats(bool is3d, const int* labels, const int* rank, const long long* offsets, const float* weights, int K, int F,
          int D, int H, int W, long long R, long long* count, long long* csum, int* bbox, double* wsum, float* wmin,
          float* wmax, fs_stream_t stream) {
  FS_ENTER();
  FS_REQUIRE_PTR(labels); FS_REQUIRE_PTR(rank); FS_REQUIRE_PTR(offsets);
  if (R > 0) { FS_REQUIRE_PTR(count); FS_REQUIRE_PTR(csum); FS_REQUIRE_PTR(bbox); }
  if (F > 0) {
    FS_REQUIRE_PTR(weights);
    if (R > 0) { FS_REQUIRE_PTR(wsum); FS_REQUIRE_PTR(wmin); FS_REQUIRE_PTR(wmax); }
  }
  GP f;
  const int rc = geometry(is3d, D, H, W, f);
  if (rc != FS_OK) return rc;
  if (K < 1 || K > kStepsPerLaunch || F < 0 || F > FS_REGION_MAX_WEIGHTS || R < 0) return FS_ERR_ARG;
  if (R == 0) return FS_OK;
  const hipStream_t s = (hipStream_t)stream;
  const int nd = is3d ? 3 : 2;
  hipLaunchKernelGGL(stats_init_kernel, dim3((unsigned)fs::cdiv(R, NT)), dim3(NT), 0, s, R, nd, F, count, csum, bbox, wsum,
                     (int*)wmin, (int*)wmax);
  const dim3 grid((unsigned)fs::cdiv(f.P, NT * kStatRounds), (unsigned)K);
  if (is3d)
    hipLaunchKernelGGL(stats_kernel<3>, grid, dim3(NT), 0, s, labels, rank, offsets, weights, F, R, count, csum, bbox,
                       wsum, (int*)wmin, (int*)wmax, f);
  else
    hipLaunchKernelGGL(stats_kernel<2>, grid, dim3(NT), 0, s, labels, rank, offsets, weights, F, R, count, csum, bbox,
                       wsum, (int*)wmin, (int*)wmax, f);
  if (F > 0)
    hipLaunchKernelGGL(stats_final_kernel, dim3((unsigned)fs::cdiv(R * F, NT)), dim3(NT), 0, s, R * F, (int*)wmin,
                       (int*)wmax);
  FS_LAUNCH_CHECK();
  return FS_OK;
}

// ---- follow ----------------------------------------------------------------------------------------------------------
template <int ND>
__global__ __launch_bounds__(NT) void follow_kernel(const int* __restrict__ labels, const float* __restrict__ flows,
                                                    int* __restrict__ dst, const GP f) {
#pragma clang fp contract(off)
  const long long q = (long long)blockIdx.x * NT + threadIdx.x;
  if (q >= f.P) return;
  const int i = (int)q;
  const size_t j = blockIdx.y;
  int out = 0;
  if (labels[j * f.P + i] > 0) {
    const float* __restrict__ u = flows + j * f.sstride;
    const int c[3] = {i % f.W, (i / f.W) % f.H, i / f.WH};
    const int ext[3] = {f.W, f.H, f.D};
    float r[3] = {0.f, 0.f, 0.f};
    bool inside = true;
#pragma unroll
    for (int a = 0; a < ND; ++a) {
      r[a] = rintf((float)c[a] + u[(size_t)a * f.P + i]);
      inside = inside && r[a] >= 0.f && r[a] <= (float)(ext[a] - 1);  // NaN and +-inf fail; nothing is converted yet
    }
    if (!inside) {
      out = FS_REGION_OUT;
    } else {
      const size_t t = ((size_t)(int)r[2] * f.H + (size_t)(int)r[1]) * f.W + (size_t)(int)r[0];
      const int L = labels[(j + 1) * f.P + t];
      out = L > 0 ? L : FS_REGION_TO_BACKGROUND;
    }
  }
  dst[j * f.P + i] = out;
}

int follow(bool is3d, const int* labels, const float* flows, int K, int C, int D, int H, int W, long long sstride,
           int* dst, fs_stream_t stream) {
  FS_ENTER();
  FS_REQUIRE_PTR(labels); FS_REQUIRE_PTR(flows); FS_REQUIRE_PTR(dst);
  GP f;
  const int rc = geometry(is3d, D, H, W, f);
  if (rc != FS_OK) return rc;
  if (C != (is3d ? 3 : 2) || sstride < (long long)C * f.P) return FS_ERR_SHAPE;
  // every coordinate and extent - 1 must be an exact float for the range test of the rounded position
  if (W > FS_REGION_FOLLOW_MAX_EXTENT || H > FS_REGION_FOLLOW_MAX_EXTENT || D > FS_REGION_FOLLOW_MAX_EXTENT) return FS_ERR_SHAPE;
  if (K < 2) return FS_ERR_ARG;
  f.sstride = sstride;
  const hipStream_t s = (hipStream_t)stream;
  const unsigned blocks = (unsigned)fs::cdiv(f.P, NT);
  for (int k0 = 0; k0 < K - 1; k0 += kStepsPerLaunch) {
    const unsigned kc = (unsigned)(K - 1 - k0 < kStepsPerLaunch ? K - 1 - k0 : kStepsPerLaunch);
    if (is3d)
      hipLaunchKernelGGL(follow_kernel<3>, dim3(blocks, kc), dim3(NT), 0, s, labels + (size_t)k0 * f.P,
                         flows + (size_t)k0 * sstride, dst + (size_t)k0 * f.P, f);
    else
      hipLaunchKernelGGL(follow_kernel<2>, dim3(blocks, kc), dim3(NT), 0, s, labels + (size_t)k0 * f.P,
                         flows + (size_t)k0 * sstride, dst + (size_t)k0 * f.P, f);
  }
  FS_LAUNCH_CHECK();
  return FS_OK;
}

}  // namespace

extern "C" long long fs_label_regions2d_ws_bytes(int K, int H, int W) { return label_ws_bytes(false, K, 1, H, W); }

extern "C" long long fs_label_regions3d_ws_bytes(int K, int D, int H, int W) { return label_ws_bytes(true, K, D, H, W); }

extern "C" int fs_label_regions2d(const unsigned char* mask, int K, int H, int W, long long mask_sstride, int require,
                                  int reject, int conn, int* labels, int* n_regions, int* status, int* ws,
                                  fs_stream_t stream) {
  return label(false, mask, K, 1, H, W, mask_sstride, require, reject, conn, labels, n_regions, status, ws, stream);
}

extern "C" int fs_label_regions3d(const unsigned char* mask, int K, int D, int H, int W, long long mask_sstride,
                                  int require, int reject, int conn, int* labels, int* n_regions, int* status, int* ws,
                                  fs_stream_t stream) {
  return label(true, mask, K, D, H, W, mask_sstride, require, reject, conn, labels, n_regions, status, ws, stream);
}

extern "C" int fs_region_stats2d(const int* labels, const int* rank, const long long* offsets, const float* weights,
                                 int K, int F, int H, int W, long long R, long long* count, long long* coord_sum,
                                 int* bbox, double* wsum, float* wmin, float* wmax, fs_stream_t stream) {
  return stats(false, labels, rank, offsets, weights, K, F, 1, H, W, R, count, coord_sum, bbox, wsum, wmin, wmax, stream);
}

extern "C" int fs_region_stats3d(const int* labels, const int* rank, const long long* offsets, const float* weights,
                                 int K, int F, int D, int H, int W, long long R, long long* count, long long* coord_sum,
                                 int* bbox, double* wsum, float* wmin, float* wmax, fs_stream_t stream) {
  return stats(true, labels, rank, offsets, weights, K, F, D, H, W, R, count, coord_sum, bbox, wsum, wmin, wmax, stream);
}

extern "C" int fs_region_follow2d(const int* labels, const float* flows, int K, int C, int H, int W,
                                  long long flow_sstride, int* dst, fs_stream_t stream) {
  return follow(false, labels, flows, K, C, 1, H, W, flow_sstride, dst, stream);
}

extern "C" int fs_region_follow3d(const int* labels, const float* flows, int K, int C, int D, int H, int W,
                                  long long flow_sstride, int* dst, fs_stream_t stream) {
  return follow(true, labels, flows, K, C, D, H, W, flow_sstride, dst, stream);
}
