// isosurface.hip -- K volumes and one isovalue to K indexed triangle meshes by marching tetrahedra on the Kuhn split of
// every cell (fs_iso_count3d, fs_iso_emit3d).  include/flowsci_hip.h states the definition; tests/isosurface_ref.py
// restates it; iso_tables.hpp (scripts/gen_iso_tables.py) holds the one table, derived from that definition.
//
// Two streaming passes with a prefix sum over the rows between them (the caller's: plumbing).  In both one wave owns
// one row (k, z, y) and walks it in chunks of 64 nodes, one node -- and the cell it is the origin of -- per lane; a
// workgroup is four consecutive rows, which share their loads in the vector cache.
//   count: the eight corners of the cell -> the node's 7-bit mask of active edges (one byte), the cell's triangles;
//          their sums over the row (wave reduction) -> two int32 per row.
//   emit:  a row that owns no vertex and no triangle ends after reading its four offsets.  Otherwise the in-row prefix
//          of the row -- and, for faces, of the three rows its cells reach into -- is recomputed from the mask bytes:
//          the counts are at most 7 (12 for triangles), so the prefix over a chunk is three (four) ballots and their
//          v_mbcnt, and a running carry joins the chunks.  A vertex lands at row offset + in-row prefix + rank of its
//          edge in the owner's mask, which is also how a face finds it: nothing is searched, no atomic decides a
//          position or an order, and the result is bitwise reproducible.
// No workgroup waits on another, every loop is bounded by W / 64 or by F <= 8, no LDS, no scratch.  Positions are
// formed without fused multiply-adds (the restatement's bits); normals and values may fuse.
#include "common.hpp"
#include "iso_tables.hpp"

namespace {

constexpr int NT = 256;
constexpr int kRows = NT / 64;  // rows per workgroup

// Corner c of a cell sits at the offset (dz, dy, dx) = (c >> 2 & 1, c >> 1 & 1, c & 1) from its origin.  Edge e of a
// node leads to the corner kEdgeCorner[e] of the cell the node is the origin of; kEdgeOfDiff is the inverse.
__device__ constexpr int kEdgeCorner[7] = {1, 2, 4, 3, 5, 6, 7};
__device__ constexpr int kEdgeOfDiff[8] = {-1, 0, 1, 3, 2, 4, 5, 6};
// c1 and c2 of the six tetrahedra (c0 = 0, c3 = 7): the permutations of (x, y, z) in lexicographic order
__device__ constexpr int kC1[6] = {1, 1, 2, 2, 4, 4};
__device__ constexpr int kC2[6] = {3, 5, 3, 6, 5, 6};
__device__ constexpr int kPair[6][2] = {{0, 1}, {0, 2}, {0, 3}, {1, 2}, {1, 3}, {2, 3}};

struct Vol {
  const float* vols;
  long long sstride, rows;  // rows = K * D * H
  int W, H, D;
  float iso;
};

struct Row {
  long long k;
  int z, y;
  bool hy, hz;  // the rows y + 1 and z + 1 exist
};

__device__ __forceinline__ Row row_of(const Vol& g, long long row) {
  Row r;
  r.y = (int)(row % g.H);
  const long long kz = row / g.H;
  r.z = (int)(kz % g.D);
  r.k = kz / g.D;
  r.hy = r.y + 1 < g.H;
  r.hz = r.z + 1 < g.D;
  return r;
}

// The eight corners of the cell whose origin is node x of the row at r00: bit c of fin = corner c exists and is finite,
// bit c of ins = it is inside (finite and >= iso).
__device__ __forceinline__ void classify(const Vol& g, const Row& r, const float* __restrict__ r00, int x, unsigned& fin,
                                         unsigned& ins) {
  const size_t sy = (size_t)g.W, sz = (size_t)g.W * g.H;
  const bool hx = x + 1 < g.W;
  const float nan = __builtin_nanf("");
  float f[8];
  f[0] = r00[x];
  f[1] = hx ? r00[x + 1] : nan;
  f[2] = r.hy ? r00[sy + x] : nan;
  f[3] = r.hy && hx ? r00[sy + x + 1] : nan;
  f[4] = r.hz ? r00[sz + x] : nan;
  f[5] = r.hz && hx ? r00[sz + x + 1] : nan;
  f[6] = r.hz && r.hy ? r00[sz + sy + x] : nan;
  f[7] = r.hz && r.hy && hx ? r00[sz + sy + x + 1] : nan;
  fin = 0;
  ins = 0;
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const bool ok = isfinite(f[c]);
    fin |= (ok ? 1u : 0u) << c;
    ins |= (ok && f[c] >= g.iso ? 1u : 0u) << c;
  }
}

// the active edges of the origin node: both ends finite, exactly one inside
__device__ __forceinline__ unsigned edge_mask(unsigned fin, unsigned ins) {
  unsigned m = 0;
#pragma unroll
  for (int e = 0; e < 7; ++e) {
    const int c = kEdgeCorner[e];
    m |= ((fin & (fin >> c) & (ins ^ (ins >> c))) & 1u) << e;
  }
  return m;
}

// triangles of a cell with eight finite corners: per tetrahedron 1 for one or three corners inside, 2 for two
__device__ __forceinline__ int cell_triangles(unsigned ins) {
  int t = 0;
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    const int n = (int)((ins & 1u) + (ins >> kC1[j] & 1u) + (ins >> kC2[j] & 1u) + (ins >> 7 & 1u));
    t += (n & 1) + (n == 2 ? 2 : 0);
  }
  return t;
}

__device__ __forceinline__ int lanes_below(unsigned long long b) {
  return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(b >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)b, 0u));
}

// Exclusive prefix over the wave of a count below 2^BITS, and the wave's total: one ballot per bit of the count.
// Every lane of the wave calls it.
template <int BITS>
__device__ __forceinline__ int wave_prefix(int c, int& total) {
  int pre = 0;
  total = 0;
#pragma unroll
  for (int b = 0; b < BITS; ++b) {
    const unsigned long long m = __ballot((c >> b) & 1);
    pre += lanes_below(m) << b;
    total += __popcll(m) << b;
  }
  return pre;
}

__global__ __launch_bounds__(NT) void iso_count_kernel(const Vol g, unsigned char* __restrict__ mask,
                                                       int* __restrict__ nv, int* __restrict__ nt) {
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * kRows + (threadIdx.x >> 6);
  if (row >= g.rows) return;  // (the whole wave)
  const Row r = row_of(g, row);
  const float* __restrict__ r00 = g.vols + r.k * g.sstride + ((size_t)r.z * g.H + r.y) * g.W;
  unsigned char* __restrict__ mrow = mask + (size_t)row * g.W;
  int cv = 0, ct = 0;
  for (int x = lane; x < g.W; x += 64) {
    unsigned fin, ins;
    classify(g, r, r00, x, fin, ins);
    const unsigned m = edge_mask(fin, ins);
    mrow[x] = (unsigned char)m;
    cv += __popc(m);
    if (fin == 0xffu) ct += cell_triangles(ins);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    cv += __shfl_xor(cv, o, 64);
    ct += __shfl_xor(ct, o, 64);
  }
  if (lane == 0) {
    nv[row] = cv;
    nt[row] = ct;
  }
}

struct EP {
  Vol g;
  const unsigned char* mask;
  const long long* voff;  // [rows + 1]
  const long long* toff;  // [rows + 1]
  const float* vals;      // [K][F][D*H*W] or NULL
  float* verts;
  float* normals;  // or NULL
  float* vout;     // [V][F]
  int* faces;
  int* status;
  long long V, T;
  int F;
  float h[3];  // spacing along x, y, z
};

__device__ __forceinline__ float edge_t(float iso, float fa, float fb) {
#pragma clang fp contract(off)
  return fminf(fmaxf((iso - fa) / (fb - fa), 0.f), 1.f);
}

__device__ __forceinline__ float coord(int i, bool moves, float t, float h) {
#pragma clang fp contract(off)
  const float q = (float)i + (moves ? t : 0.f);
  return q * h;
}

// central differences, one-sided on the boundary, divided by the distance between the two nodes used
__device__ __forceinline__ void node_gradient(const EP& p, const float* __restrict__ vol, int z, int y, int x,
                                              float (&G)[3]) {
  const size_t sy = (size_t)p.g.W, sz = (size_t)p.g.W * p.g.H;
  const float* __restrict__ at = vol + (size_t)z * sz + (size_t)y * sy + x;
  const int xl = x > 0, xh = x + 1 < p.g.W, yl = y > 0, yh = y + 1 < p.g.H, zl = z > 0, zh = z + 1 < p.g.D;
  G[0] = (at[xh] - at[-xl]) / (xl + xh == 2 ? 2.f * p.h[0] : p.h[0]);
  G[1] = (at[yh ? sy : 0] - *(at - (yl ? sy : 0))) / (yl + yh == 2 ? 2.f * p.h[1] : p.h[1]);
  G[2] = (at[zh ? sz : 0] - *(at - (zl ? sz : 0))) / (zl + zh == 2 ? 2.f * p.h[2] : p.h[2]);
}

// the vertex on edge E of node (z, y, x), whose value is fa and whose gradient Ga, to row `idx` of the outputs
template <int E>
__device__ __forceinline__ void emit_vertex(const EP& p, const Row& r, const float* __restrict__ vol, int x, float fa,
                                            const float (&Ga)[3], long long idx) {
  constexpr int c = kEdgeCorner[E], dx = c & 1, dy = c >> 1 & 1, dz = c >> 2 & 1;
  if (idx < 0 || idx >= p.V) return;  // (emit_kernel has reported it)
  // a mask that is not this volume's could name an edge that leaves it: nothing is read out there
  if ((dx && x + 1 >= p.g.W) || (dy && !r.hy) || (dz && !r.hz)) return;
  const size_t P = (size_t)p.g.W * p.g.H * p.g.D;
  const size_t a = ((size_t)r.z * p.g.H + r.y) * p.g.W + x;
  const size_t b = a + ((size_t)dz * p.g.H + dy) * p.g.W + dx;
  const float t = edge_t(p.g.iso, fa, vol[b]);
  float* __restrict__ v = p.verts + 3 * idx;
  v[0] = coord(x, dx, t, p.h[0]);
  v[1] = coord(r.y, dy, t, p.h[1]);
  v[2] = coord(r.z, dz, t, p.h[2]);
  if (p.normals) {
    float Gb[3], G[3];
    node_gradient(p, vol, r.z + dz, r.y + dy, x + dx, Gb);
#pragma unroll
    for (int i = 0; i < 3; ++i) G[i] = Ga[i] + t * (Gb[i] - Ga[i]);
    const float len = sqrtf(G[0] * G[0] + G[1] * G[1] + G[2] * G[2]);
    const bool ok = len > 0.f && isfinite(len);
    float* __restrict__ n = p.normals + 3 * idx;
#pragma unroll
    for (int i = 0; i < 3; ++i) n[i] = ok ? -G[i] / len : 0.f;
  }
  if (p.vals) {
    const float* __restrict__ w = p.vals + (size_t)r.k * p.F * P;
    for (int f = 0; f < p.F; ++f) {
      const float wa = w[f * P + a], wb = w[f * P + b];
      p.vout[idx * p.F + f] = wa + t * (wb - wa);
    }
  }
}

__device__ __forceinline__ int pick6(unsigned id, int a0, int a1, int a2, int a3, int a4, int a5) {
  int r = a0;
  r = id == 1u ? a1 : r;
  r = id == 2u ? a2 : r;
  r = id == 3u ? a3 : r;
  r = id == 4u ? a4 : r;
  return id == 5u ? a5 : r;
}

// What a lane knows of the corners 0..6 of its cell (7 owns nothing in it): m[c] the corner node's mask, v[c] the
// step-local index of the first vertex it owns.  Indexed by constants only: the arrays live in registers.
struct Corners {
  unsigned m[7];
  int v[7];
};

// the step-local index of the vertex on edge J (kPair) of tetrahedron TET
template <int TET, int J>
__device__ __forceinline__ int edge_vertex(const Corners& c) {
  constexpr int C[4] = {0, kC1[TET], kC2[TET], 7};
  constexpr int own = C[kPair[J][0]];
  constexpr int e = kEdgeOfDiff[C[kPair[J][1]] ^ own];
  return c.v[own] + __popc(c.m[own] & ((1u << e) - 1u));
}

// The triangles of tetrahedron TET of a cell, to the face rows tb, tb + 1.  Returns false when an index leaves the
// step's vertices or a row the faces.
template <int TET>
__device__ __forceinline__ bool emit_tet(const EP& p, unsigned ins, const Corners& c, unsigned vcount, long long& tb) {
  const unsigned cs = (ins & 1u) | (ins >> kC1[TET] & 1u) << 1 | (ins >> kC2[TET] & 1u) << 2 | (ins >> 7 & 1u) << 3;
  if (cs == 0u || cs == 15u) return true;
  const unsigned code = kIsoTri[TET][cs];
  const int e0 = edge_vertex<TET, 0>(c), e1 = edge_vertex<TET, 1>(c), e2 = edge_vertex<TET, 2>(c),
            e3 = edge_vertex<TET, 3>(c), e4 = edge_vertex<TET, 4>(c), e5 = edge_vertex<TET, 5>(c);
  bool ok = true;
  const int ntri = (int)(code & 3u);
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    if (j < ntri) {
      const int i0 = pick6(code >> (2 + 9 * j) & 7u, e0, e1, e2, e3, e4, e5);
      const int i1 = pick6(code >> (5 + 9 * j) & 7u, e0, e1, e2, e3, e4, e5);
      const int i2 = pick6(code >> (8 + 9 * j) & 7u, e0, e1, e2, e3, e4, e5);
      ok = ok && (unsigned)i0 < vcount && (unsigned)i1 < vcount && (unsigned)i2 < vcount;
      if (tb >= 0 && tb < p.T) {
        int* __restrict__ f = p.faces + 3 * tb;
        f[0] = i0;
        f[1] = i1;
        f[2] = i2;
      } else {
        ok = false;
      }
      ++tb;
    }
  }
  return ok;
}

// One chunk of mask row Q (0: (z, y), 1: (z, y+1), 2: (z+1, y), 3: (z+1, y+1)) -> the corners 2Q and 2Q + 1.  `carry` is
// the step-local index of the first vertex the chunk's nodes own (wave-uniform); false when the chunk leaves the step.
template <int Q>
__device__ __forceinline__ bool corner_row(const unsigned char* __restrict__ mrow, bool on, bool in, bool hx, int x,
                                           long long vcount, long long& carry, Corners& c) {
  unsigned m = 0, mn = 0;
  int pre = 0, total = 0;
  if (on) {  // (wave-uniform: every lane takes part in the ballots)
    m = in ? mrow[x] : 0u;
    if (Q < 3) mn = hx ? mrow[x + 1] : 0u;
    pre = wave_prefix<3>(__popc(m), total);
  }
  const bool ok = carry >= 0 && carry + total <= vcount;
  c.m[2 * Q] = m;
  c.v[2 * Q] = (int)carry + pre;
  if (Q < 3) {
    c.m[Q < 3 ? 2 * Q + 1 : 0] = mn;
    c.v[Q < 3 ? 2 * Q + 1 : 0] = c.v[2 * Q] + __popc(m);
  }
  carry += total;
  return ok;
}

__global__ __launch_bounds__(NT) void iso_emit_kernel(const EP p) {
  const Vol& g = p.g;
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * kRows + (threadIdx.x >> 6);
  if (row >= g.rows) return;
  const long long v0 = p.voff[row], t0 = p.toff[row];
  const long long nvr = p.voff[row + 1] - v0, ntr = p.toff[row + 1] - t0;
  if (nvr == 0 && ntr == 0) return;  // (most rows of a sparse surface end here)
  const Row r = row_of(g, row);
  const long long step0 = row - ((long long)r.z * g.H + r.y);  // the first row of this step
  const long long vstep = p.voff[step0];
  const long long vcount = p.voff[step0 + (long long)g.D * g.H] - vstep;
  const bool faces = ntr != 0 && r.hy && r.hz;
  const float* __restrict__ vol = g.vols + r.k * g.sstride;
  const float* __restrict__ r00 = vol + ((size_t)r.z * g.H + r.y) * g.W;
  const unsigned char* __restrict__ m00 = p.mask + (size_t)row * g.W;
  const unsigned char* __restrict__ m10 = m00 + (size_t)g.W * g.H;
  // the step-local index of the first vertex each of the four rows owns
  long long c00 = v0 - vstep, c01 = 0, c10 = 0, c11 = 0;
  if (faces) {
    c01 = p.voff[row + 1] - vstep;
    c10 = p.voff[row + g.H] - vstep;
    c11 = p.voff[row + g.H + 1] - vstep;
  }
  long long ct = t0;
  bool ok = vcount >= 0 && vcount <= 0x7fffffffLL && vstep >= 0 && vstep + vcount <= p.V;
  for (int x0 = 0; x0 < g.W; x0 += 64) {
    const int x = x0 + lane;
    const bool in = x < g.W, hx = x + 1 < g.W;
    Corners c;
    ok = corner_row<0>(m00, true, in, hx, x, vcount, c00, c) && ok;
    ok = corner_row<1>(m00 + g.W, faces, in, hx, x, vcount, c01, c) && ok;
    ok = corner_row<2>(m10, faces, in, hx, x, vcount, c10, c) && ok;
    ok = corner_row<3>(m10 + g.W, faces, in, hx, x, vcount, c11, c) && ok;
    if (faces) {
      // all seven edges of the origin lie in its cell and reach every other corner: a cell whose origin owns no vertex
      // is not cut, and its corners are not even loaded
      unsigned fin = 0, ins = 0;
      if (hx && c.m[0]) classify(g, r, r00, x, fin, ins);
      const bool cut = fin == 0xffu;
      int total;
      const int pre = wave_prefix<4>(cut ? cell_triangles(ins) : 0, total);
      if (cut) {
        long long tb = ct + pre;
        ok = emit_tet<0>(p, ins, c, (unsigned)vcount, tb) && ok;
        ok = emit_tet<1>(p, ins, c, (unsigned)vcount, tb) && ok;
        ok = emit_tet<2>(p, ins, c, (unsigned)vcount, tb) && ok;
        ok = emit_tet<3>(p, ins, c, (unsigned)vcount, tb) && ok;
        ok = emit_tet<4>(p, ins, c, (unsigned)vcount, tb) && ok;
        ok = emit_tet<5>(p, ins, c, (unsigned)vcount, tb) && ok;
      }
      ct += total;
    }
    const unsigned m = c.m[0];
    // (edges along x are e0, e3, e4, e6; along y e1, e3, e5, e6; along z e2, e4, e5, e6)
    ok = ok && (m & ((hx ? 0u : 0x59u) | (r.hy ? 0u : 0x6au) | (r.hz ? 0u : 0x74u) | 0x80u)) == 0u;
    if (m && ok) {
      const float fa = r00[x];
      float Ga[3] = {0.f, 0.f, 0.f};
      if (p.normals) node_gradient(p, vol, r.z, r.y, x, Ga);
      const long long base = vstep + c.v[0];
      if (m & 1u) emit_vertex<0>(p, r, vol, x, fa, Ga, base);
      if (m & 2u) emit_vertex<1>(p, r, vol, x, fa, Ga, base + __popc(m & 1u));
      if (m & 4u) emit_vertex<2>(p, r, vol, x, fa, Ga, base + __popc(m & 3u));
      if (m & 8u) emit_vertex<3>(p, r, vol, x, fa, Ga, base + __popc(m & 7u));
      if (m & 16u) emit_vertex<4>(p, r, vol, x, fa, Ga, base + __popc(m & 15u));
      if (m & 32u) emit_vertex<5>(p, r, vol, x, fa, Ga, base + __popc(m & 31u));
      if (m & 64u) emit_vertex<6>(p, r, vol, x, fa, Ga, base + __popc(m & 63u));
    }
  }
  // the masks must add up to what the offsets say this row owns
  ok = ok && c00 - (v0 - vstep) == nvr && (faces ? ct - t0 == ntr : ntr == 0);
  if (__ballot(!ok) != 0ull && lane == 0) atomicOr(p.status, 1);
}

// FS_OK, or what is wrong with the volumes' geometry
int check_volumes(int K, int D, int H, int W, long long sstride) {
  if (K < 1 || D < 2 || H < 2 || W < 2) return FS_ERR_SHAPE;
  const long long P = (long long)D * H * W;
  if (P > 0x7fffffffLL || sstride < P) return FS_ERR_SHAPE;
  if ((long long)K * D * H > 0x7fffffffLL) return FS_ERR_SHAPE;
  return FS_OK;
}

inline bool finite_d(double v) { return v > -HUGE_VAL && v < HUGE_VAL; }

inline long long counts_bytes(int K, int D, int H) { return (2LL * K * D * H * 4 + 15) / 16 * 16; }

Vol make_vol(const float* volumes, int K, int D, int H, int W, long long sstride, double iso) {
  Vol g;
  g.vols = volumes; g.sstride = sstride; g.rows = (long long)K * D * H;
  g.W = W; g.H = H; g.D = D; g.iso = (float)iso;
  return g;
}

}  // namespace

extern "C" long long fs_iso3d_ws_bytes(int K, int D, int H, int W) {
  const int rc = check_volumes(K, D, H, W, (long long)D * H * W);
  if (rc != FS_OK) return -rc;
  return counts_bytes(K, D, H) + (long long)K * D * H * W;
}

extern "C" int fs_iso_count3d(const float* volumes, int K, int D, int H, int W, long long sstride, double iso,
                              unsigned char* ws, fs_stream_t stream) {
  FS_ENTER();
  FS_REQUIRE_PTR(volumes); FS_REQUIRE_PTR(ws);
  const int rc = check_volumes(K, D, H, W, sstride);
  if (rc != FS_OK) return rc;
  if (!finite_d(iso) || !finite_d((double)(float)iso) || ((uintptr_t)ws & 3u)) return FS_ERR_ARG;
  const Vol g = make_vol(volumes, K, D, H, W, sstride, iso);
  int* nv = reinterpret_cast<int*>(ws);
  hipLaunchKernelGGL(iso_count_kernel, dim3((unsigned)((g.rows + kRows - 1) / kRows)), dim3(NT), 0, (hipStream_t)stream, g,
                     ws + counts_bytes(K, D, H), nv, nv + g.rows);
  FS_LAUNCH_CHECK();
  return FS_OK;
}

extern "C" int fs_iso_emit3d(const float* volumes, int K, int D, int H, int W, long long sstride, double iso,
                             const double* spacing, const unsigned char* ws, const long long* row_offsets, long long V,
                             long long T, const float* values, int F, float* vertices, float* normals, float* values_out,
                             int* faces, int* status, fs_stream_t stream) {
  FS_ENTER();
  FS_REQUIRE_PTR(volumes); FS_REQUIRE_PTR(spacing); FS_REQUIRE_PTR(ws); FS_REQUIRE_PTR(row_offsets); FS_REQUIRE_PTR(status);
  if (V > 0) FS_REQUIRE_PTR(vertices);
  if (T > 0) FS_REQUIRE_PTR(faces);
  if (F > 0) { FS_REQUIRE_PTR(values); if (V > 0) FS_REQUIRE_PTR(values_out); }
  const int rc = check_volumes(K, D, H, W, sstride);
  if (rc != FS_OK) return rc;
  if (F < 0 || F > FS_ISO_MAX_VALUES) return FS_ERR_SHAPE;
  if (!finite_d(iso) || !finite_d((double)(float)iso) || V < 0 || T < 0 || ((uintptr_t)ws & 3u)) return FS_ERR_ARG;
  EP p;
  for (int a = 0; a < 3; ++a) {
    p.h[a] = (float)spacing[a];
    // (what is finite and positive in fp64 must still be so in fp32)
    if (!(spacing[a] > 0.0) || !(p.h[a] > 0.f) || !(p.h[a] < HUGE_VALF)) return FS_ERR_ARG;
  }
  if (V == 0 && T == 0) return FS_OK;  // nothing to write: nothing launched
  p.g = make_vol(volumes, K, D, H, W, sstride, iso);
  p.mask = ws + counts_bytes(K, D, H);
  p.voff = row_offsets;
  p.toff = row_offsets + p.g.rows + 1;
  p.vals = F > 0 ? values : nullptr;
  p.verts = vertices; p.normals = normals; p.vout = values_out; p.faces = faces; p.status = status;
  p.V = V; p.T = T; p.F = F;
  hipLaunchKernelGGL(iso_emit_kernel, dim3((unsigned)((p.g.rows + kRows - 1) / kRows)), dim3(NT), 0, (hipStream_t)stream,
                     p);
  FS_LAUNCH_CHECK();
  return FS_OK;
}
