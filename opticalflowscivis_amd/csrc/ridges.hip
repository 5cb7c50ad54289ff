// ridges.hip -- height-ridge surfaces of K scalar volumes (Eberly's definition, extracted by Marching Ridges on the Kuhn
// split of every cell): fs_ridge_nodes3d, fs_ridge_count3d, fs_ridge_emit3d.  include/flowsci_hip.h states the
// definition; tests/ridge_ref.py restates it; iso_tables.hpp holds the triangle table, which is the isosurface's.
//
// Three streaming passes with the caller's prefix sum over the rows between the last two.  In all of them one wave owns
// one row (k, z, y) and walks it in chunks of 64 nodes, one node -- and the cell it is the origin of -- per lane; a
// workgroup is four consecutive rows, which share their loads in the vector cache.
//   nodes: the 19-point stencil -> gradient and Hessian in fp64, FS_RIDGE_SWEEPS cyclic Jacobi sweeps made of
//          correctly rounded + - * / sqrt alone (no fused multiply-add, no estimate instruction: every stored bit can be
//          restated), the minor eigenvector e, d = e . g and the eigenvalue -> five fp32 planes and one class byte.
//   count: the stored operands of the cell's eight corners -> the node's 7-bit mask of active edges, the cell's
//          triangles, twisted and all-eligible tetrahedra; their sums over the row -> four int32 per row.
//   emit:  as fs_iso_emit3d: the in-row prefix is recomputed from the mask bytes by ballots, a vertex lands at row
//          offset + in-row prefix + rank of its edge in the owner's mask, which is also how a face finds it.
// The orientation of e is decided per edge from its two ends, so every cell sharing an edge computes the same vertex;
// the tetrahedron only checks that its six edges' decisions are consistent (else it is TWISTED and emits nothing).
// No workgroup waits on another, every loop is bounded by W / 64 or a constant, no LDS, no scratch, no atomic decides a
// position or an order.
#include "common.hpp"
#include "iso_tables.hpp"

#pragma clang fp contract(off)

namespace {

constexpr int NT = 256;
constexpr int kRows = NT / 64;  // rows per workgroup

// (as in isosurface.hip) corner c of a cell sits at (dz, dy, dx) = (c >> 2 & 1, c >> 1 & 1, c & 1) from its origin; edge
// e of a node leads to the corner kEdgeCorner[e] of the cell the node is the origin of; kEdgeOfDiff is the inverse
__device__ constexpr int kEdgeCorner[7] = {1, 2, 4, 3, 5, 6, 7};
__device__ constexpr int kEdgeOfDiff[8] = {-1, 0, 1, 3, 2, 4, 5, 6};
__device__ constexpr int kC1[6] = {1, 1, 2, 2, 4, 4};
__device__ constexpr int kC2[6] = {3, 5, 3, 6, 5, 6};
__device__ constexpr int kPair[6][2] = {{0, 1}, {0, 2}, {0, 3}, {1, 2}, {1, 3}, {2, 3}};

struct Grid {
  long long rows;  // K * D * H
  int W, H, D;
};

struct Row {
  long long k;
  int z, y;
  bool hy, hz;  // the rows y + 1 and z + 1 exist
};

__device__ __forceinline__ Row row_of(const Grid& g, long long row) {
  Row r;
  r.y = (int)(row % g.H);
  const long long kz = row / g.H;
  r.z = (int)(kz % g.D);
  r.k = kz / g.D;
  r.hy = r.y + 1 < g.H;
  r.hz = r.z + 1 < g.D;
  return r;
}

// ---------------------------------------------------------------------------------------------------------------------
// node pass
// ---------------------------------------------------------------------------------------------------------------------
struct NP {
  Grid g;
  const float* vols;
  long long sstride;
  int valley;
  double i2h[3], ihh[3], i4hh[3], strength, fmin;
  float* operands;     // [K][5][P]
  unsigned char* cls;  // [K][P]
};

// One exact Jacobi rotation of the pair (p, q); r is the third index, v?p and v?q the two columns of the accumulated
// rotations.  a_pq == 0: nothing changes.
__device__ __forceinline__ void rotate(double& app, double& aqq, double& apq, double& arp, double& arq, double& v0p,
                                       double& v0q, double& v1p, double& v1q, double& v2p, double& v2q) {
  if (apq == 0.0) return;
  const double theta = (aqq - app) / (2.0 * apq);
  double t = 1.0 / (fabs(theta) + sqrt(theta * theta + 1.0));  // theta^2 = inf: t = 0, the identity
  t = theta < 0.0 ? -t : t;
  const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
  const double h = t * apq;
  app = app - h;
  aqq = aqq + h;
  apq = 0.0;
  const double rp = c * arp - s * arq, rq = s * arp + c * arq;
  arp = rp;
  arq = rq;
  const double a0 = c * v0p - s * v0q, b0 = s * v0p + c * v0q;
  const double a1 = c * v1p - s * v1q, b1 = s * v1p + c * v1q;
  const double a2 = c * v2p - s * v2q, b2 = s * v2p + c * v2q;
  v0p = a0; v0q = b0;
  v1p = a1; v1q = b1;
  v2p = a2; v2q = b2;
}

__device__ __forceinline__ bool finite_f(float v) { return fabsf(v) < __builtin_inff(); }

__global__ __launch_bounds__(NT) void ridge_node_kernel(const NP p) {
  const Grid& g = p.g;
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * kRows + (threadIdx.x >> 6);
  if (row >= g.rows) return;  // (the whole wave)
  const Row r = row_of(g, row);
  const long long sy = g.W, sz = (long long)g.W * g.H;
  const size_t P = (size_t)sz * g.D;
  const size_t at0 = ((size_t)r.z * g.H + r.y) * g.W;
  const float* __restrict__ f0 = p.vols + r.k * p.sstride + at0;
  float* __restrict__ op = p.operands + (size_t)r.k * 5 * P + at0;
  unsigned char* __restrict__ cl = p.cls + (size_t)r.k * P + at0;
  const bool row_border = r.z == 0 || r.y == 0 || !r.hz || !r.hy;
  const float nanf_ = __builtin_nanf("");
  for (int x = lane; x < g.W; x += 64) {
    int c = FS_RIDGE_BORDER;
    float o0 = nanf_, o1 = nanf_, o2 = nanf_, o3 = nanf_, o4 = nanf_;
    if (!row_border && x > 0 && x + 1 < g.W) {
      const float* __restrict__ f = f0 + x;
      const float sgn = p.valley ? -1.f : 1.f;  // (a product with +-1 is exact: the negation)
      const float fc = sgn * f[0];
      const float xp = sgn * f[1], xm = sgn * f[-1], yp = sgn * f[sy], ym = sgn * f[-sy], zp = sgn * f[sz], zm = sgn * f[-sz];
      const float xypp = sgn * f[sy + 1], xypm = sgn * f[-sy + 1], xymp = sgn * f[sy - 1], xymm = sgn * f[-sy - 1];
      const float xzpp = sgn * f[sz + 1], xzpm = sgn * f[-sz + 1], xzmp = sgn * f[sz - 1], xzmm = sgn * f[-sz - 1];
      const float yzpp = sgn * f[sz + sy], yzpm = sgn * f[-sz + sy], yzmp = sgn * f[sz - sy], yzmm = sgn * f[-sz - sy];
      const bool fin = finite_f(fc) && finite_f(xp) && finite_f(xm) && finite_f(yp) && finite_f(ym) && finite_f(zp) &&
                       finite_f(zm) && finite_f(xypp) && finite_f(xypm) && finite_f(xymp) && finite_f(xymm) &&
                       finite_f(xzpp) && finite_f(xzpm) && finite_f(xzmp) && finite_f(xzmm) && finite_f(yzpp) &&
                       finite_f(yzpm) && finite_f(yzmp) && finite_f(yzmm);
      c = FS_RIDGE_NONFINITE;
      if (fin) {
        const double fd = (double)fc;
        const double g0 = ((double)xp - (double)xm) * p.i2h[0];
        const double g1 = ((double)yp - (double)ym) * p.i2h[1];
        const double g2 = ((double)zp - (double)zm) * p.i2h[2];
        double a00 = (((double)xp - 2.0 * fd) + (double)xm) * p.ihh[0];
        double a11 = (((double)yp - 2.0 * fd) + (double)ym) * p.ihh[1];
        double a22 = (((double)zp - 2.0 * fd) + (double)zm) * p.ihh[2];
        double a01 = (((double)xypp - (double)xypm) - ((double)xymp - (double)xymm)) * p.i4hh[0];
        double a02 = (((double)xzpp - (double)xzpm) - ((double)xzmp - (double)xzmm)) * p.i4hh[1];
        double a12 = (((double)yzpp - (double)yzpm) - ((double)yzmp - (double)yzmm)) * p.i4hh[2];
        double v00 = 1.0, v01 = 0.0, v02 = 0.0, v10 = 0.0, v11 = 1.0, v12 = 0.0, v20 = 0.0, v21 = 0.0, v22 = 1.0;
        for (int s = 0; s < FS_RIDGE_SWEEPS; ++s) {
          rotate(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);  // (0, 1), r = 2
          rotate(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);  // (0, 2), r = 1
          rotate(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);  // (1, 2), r = 0
        }
        // (selects, one per value: a column chosen by an index would put V into scratch)
        const bool b1 = a11 < a00;
        const double l1 = b1 ? a11 : a00;
        const bool b2 = a22 < l1;
        const double lam = b2 ? a22 : l1;
        const double e0 = b2 ? v02 : (b1 ? v01 : v00);
        const double e1 = b2 ? v12 : (b1 ? v11 : v10);
        const double e2 = b2 ? v22 : (b1 ? v21 : v20);
        const double d = (e0 * g0 + e1 * g1) + e2 * g2;
        const float s0 = (float)e0, s1 = (float)e1, s2 = (float)e2, s3 = (float)d, s4 = (float)lam;
        if (finite_f(s0) && finite_f(s1) && finite_f(s2) && finite_f(s3) && finite_f(s4)) {
          if (!(lam <= -p.strength)) {
            c = FS_RIDGE_WEAK;
          } else if (!(fd >= p.fmin)) {
            c = FS_RIDGE_LOW;
          } else {
            c = FS_RIDGE_ELIGIBLE;
            o0 = s0; o1 = s1; o2 = s2; o3 = s3; o4 = s4;
          }
        }
      }
    }
    op[x] = o0;
    op[P + x] = o1;
    op[2 * P + x] = o2;
    op[3 * P + x] = o3;
    op[4 * P + x] = o4;
    cl[x] = (unsigned char)c;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// marching pass: reads the stored operands only
// ---------------------------------------------------------------------------------------------------------------------
struct MP {
  Grid g;
  const float* operands;     // [K][5][P]
  const unsigned char* cls;  // [K][P]
};

// The eight corners of a cell as stored: bit c of el = corner c exists and is ELIGIBLE (its e and d are then finite).
// Indexed by constants only: the arrays live in registers.
struct Cell {
  float e[8][3];
  float d[8];
  unsigned el;
};

__device__ __forceinline__ void load_cell(const MP& m, const Row& r, int x, Cell& c) {
  const size_t P = (size_t)m.g.W * m.g.H * m.g.D;
  const size_t a = ((size_t)r.z * m.g.H + r.y) * m.g.W + x;
  const float* __restrict__ op = m.operands + (size_t)r.k * 5 * P;
  const unsigned char* __restrict__ cl = m.cls + (size_t)r.k * P;
  const bool hx = x + 1 < m.g.W;
  c.el = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int dx = i & 1, dy = i >> 1 & 1, dz = i >> 2 & 1;
    const bool exists = (!dx || hx) && (!dy || r.hy) && (!dz || r.hz);
    const size_t b = a + ((size_t)dz * m.g.H + dy) * m.g.W + dx;
    const bool ok = exists && cl[exists ? b : a] == FS_RIDGE_ELIGIBLE;
    c.el |= (ok ? 1u : 0u) << i;
    c.e[i][0] = ok ? op[b] : 0.f;
    c.e[i][1] = ok ? op[P + b] : 0.f;
    c.e[i][2] = ok ? op[2 * P + b] : 0.f;
    c.d[i] = ok ? op[3 * P + b] : 0.f;
  }
}

template <int A, int B>
__device__ __forceinline__ bool neg_dot(const Cell& c) {
  const double o = ((double)c.e[A][0] * (double)c.e[B][0] + (double)c.e[A][1] * (double)c.e[B][1]) +
                   (double)c.e[A][2] * (double)c.e[B][2];
  return o < 0.0;
}

__device__ __forceinline__ unsigned sign_of(float v) { return __float_as_uint(v) >> 31; }

// What the cell decides: neg0 bit c = e_0 . e_c < 0 (c = 1..7), neg7 bit c = e_c . e_7 < 0 (c = 1..6), negm bit j =
// e_c1 . e_c2 < 0 of tetrahedron j, sb bit c = the sign bit of d_c.
struct Signs {
  unsigned neg0, neg7, negm, sb;
};

__device__ __forceinline__ Signs cell_signs(const Cell& c) {
  Signs s;
  s.neg0 = (neg_dot<0, 1>(c) ? 2u : 0u) | (neg_dot<0, 2>(c) ? 4u : 0u) | (neg_dot<0, 3>(c) ? 8u : 0u) |
           (neg_dot<0, 4>(c) ? 16u : 0u) | (neg_dot<0, 5>(c) ? 32u : 0u) | (neg_dot<0, 6>(c) ? 64u : 0u) |
           (neg_dot<0, 7>(c) ? 128u : 0u);
  s.neg7 = (neg_dot<1, 7>(c) ? 2u : 0u) | (neg_dot<2, 7>(c) ? 4u : 0u) | (neg_dot<3, 7>(c) ? 8u : 0u) |
           (neg_dot<4, 7>(c) ? 16u : 0u) | (neg_dot<5, 7>(c) ? 32u : 0u) | (neg_dot<6, 7>(c) ? 64u : 0u);
  s.negm = (neg_dot<1, 3>(c) ? 1u : 0u) | (neg_dot<1, 5>(c) ? 2u : 0u) | (neg_dot<2, 3>(c) ? 4u : 0u) |
           (neg_dot<2, 6>(c) ? 8u : 0u) | (neg_dot<4, 5>(c) ? 16u : 0u) | (neg_dot<4, 6>(c) ? 32u : 0u);
  s.sb = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) s.sb |= sign_of(c.d[i]) << i;
  return s;
}

// the active edges of the origin node: both ends ELIGIBLE, the sign bits of d_a and of d_b (negated where e_a . e_b < 0)
// differ
__device__ __forceinline__ unsigned edge_mask(const Cell& c, const Signs& s) {
  unsigned m = 0;
#pragma unroll
  for (int e = 0; e < 7; ++e) {
    const int b = kEdgeCorner[e];
    m |= ((c.el & (c.el >> b) & (s.sb ^ (s.sb >> b) ^ (s.neg0 >> b))) & 1u) << e;
  }
  return m;
}

// The six tetrahedra of the cell: 4 bits each of the case (0 where the tetrahedron emits nothing), the number of twisted
// and of all-eligible ones.
__device__ __forceinline__ unsigned cell_cases(const Cell& c, const Signs& s, int& twisted, int& tets) {
  unsigned cases = 0;
  twisted = 0;
  tets = 0;
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    const int c1 = kC1[j], c2 = kC2[j];
    const unsigned ok = c.el & (c.el >> c1) & (c.el >> c2) & (c.el >> 7) & 1u;
    const unsigned s1 = s.neg0 >> c1 & 1u, s2 = s.neg0 >> c2 & 1u, s3 = s.neg0 >> 7 & 1u;
    const unsigned tw = ((s.negm >> j & 1u) ^ s1 ^ s2) | ((s.neg7 >> c1 & 1u) ^ s1 ^ s3) | ((s.neg7 >> c2 & 1u) ^ s2 ^ s3);
    const unsigned cs = ((s.sb & 1u) ^ 1u) | ((s.sb >> c1 & 1u) ^ s1 ^ 1u) << 1 | ((s.sb >> c2 & 1u) ^ s2 ^ 1u) << 2 |
                        ((s.sb >> 7 & 1u) ^ s3 ^ 1u) << 3;
    tets += (int)ok;
    twisted += (int)(ok & tw);
    cases |= (ok & ~tw & 1u ? cs : 0u) << (4 * j);
  }
  return cases;
}

// triangles of a tetrahedron by its case: 1 for one or three corners inside, 2 for two
__device__ __forceinline__ int case_triangles(unsigned cs) {
  const int n = __popc(cs & 15u);
  return (n & 1) + (n == 2 ? 2 : 0);
}

__device__ __forceinline__ int cell_triangles(unsigned cases) {
  int t = 0;
#pragma unroll
  for (int j = 0; j < 6; ++j) t += case_triangles(cases >> (4 * j));
  return t;
}

__device__ __forceinline__ int lanes_below(unsigned long long b) {
  return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(b >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)b, 0u));
}

// Exclusive prefix over the wave of a count below 2^BITS, and the wave's total: one ballot per bit of the count.
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

__global__ __launch_bounds__(NT) void ridge_count_kernel(const MP p, unsigned char* __restrict__ mask,
                                                         int* __restrict__ counts) {
  const Grid& g = p.g;
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * kRows + (threadIdx.x >> 6);
  if (row >= g.rows) return;  // (the whole wave)
  const Row r = row_of(g, row);
  unsigned char* __restrict__ mrow = mask + (size_t)row * g.W;
  const size_t P = (size_t)g.W * g.H * g.D;
  const unsigned char* __restrict__ cl = p.cls + (size_t)r.k * P + ((size_t)r.z * g.H + r.y) * g.W;
  int cv = 0, ct = 0, cw = 0, ce = 0;
  for (int x = lane; x < g.W; x += 64) {
    unsigned m = 0;
    // every edge and every tetrahedron of the cell has the origin as an end or a corner
    if (cl[x] == FS_RIDGE_ELIGIBLE) {
      Cell c;
      load_cell(p, r, x, c);
      const Signs s = cell_signs(c);
      m = edge_mask(c, s);
      int tw, te;
      const unsigned cases = cell_cases(c, s, tw, te);
      cv += __popc(m);
      ct += cell_triangles(cases);
      cw += tw;
      ce += te;
    }
    mrow[x] = (unsigned char)m;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    cv += __shfl_xor(cv, o, 64);
    ct += __shfl_xor(ct, o, 64);
    cw += __shfl_xor(cw, o, 64);
    ce += __shfl_xor(ce, o, 64);
  }
  if (lane == 0) {
    counts[row] = cv;
    counts[g.rows + row] = ct;
    counts[2 * g.rows + row] = cw;
    counts[3 * g.rows + row] = ce;
  }
}

struct EP {
  MP m;
  const float* vols;
  long long sstride;
  int valley;
  const unsigned char* mask;
  const long long* voff;  // [rows + 1]
  const long long* toff;  // [rows + 1]
  float* verts;
  float* vout;  // [V][2] or NULL
  int* faces;
  int* status;
  long long V, T;
  float h[3];  // spacing along x, y, z
};

__device__ __forceinline__ float coord(int i, bool moves, float t, float h) {
  const float q = (float)i + (moves ? t : 0.f);
  return q * h;
}

// the vertex on edge E of node (z, y, x), the origin of `c`, to row `idx` of the outputs
template <int E>
__device__ __forceinline__ void emit_vertex(const EP& p, const Row& r, int x, const Cell& c, long long idx) {
  constexpr int b = kEdgeCorner[E], dx = b & 1, dy = b >> 1 & 1, dz = b >> 2 & 1;
  const Grid& g = p.m.g;
  if (idx < 0 || idx >= p.V) return;  // (emit_kernel has reported it)
  if ((dx && x + 1 >= g.W) || (dy && !r.hy) || (dz && !r.hz)) return;  // nothing is read outside the volume
  const double da = (double)c.d[0];
  const double db = neg_dot<0, b>(c) ? -(double)c.d[b] : (double)c.d[b];
  const double den = da - db;
  double t = den == 0.0 ? 0.5 : da / den;
  t = fmin(fmax(t, 0.0), 1.0);
  const float tf = (float)t;
  float* __restrict__ v = p.verts + 3 * idx;
  v[0] = coord(x, dx, tf, p.h[0]);
  v[1] = coord(r.y, dy, tf, p.h[1]);
  v[2] = coord(r.z, dz, tf, p.h[2]);
  if (p.vout) {
    const size_t P = (size_t)g.W * g.H * g.D;
    const size_t ia = ((size_t)r.z * g.H + r.y) * g.W + x;
    const size_t ib = ia + ((size_t)dz * g.H + dy) * g.W + dx;
    const float* __restrict__ vol = p.vols + r.k * p.sstride;
    const float* __restrict__ lam = p.m.operands + ((size_t)r.k * 5 + 4) * P;
    const float sgn = p.valley ? -1.f : 1.f;
    const float fa = sgn * vol[ia], fb = sgn * vol[ib], la = lam[ia], lb = lam[ib];
    p.vout[2 * idx] = fa + tf * (fb - fa);
    p.vout[2 * idx + 1] = la + tf * (lb - la);
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
// step-local index of the first vertex it owns.
struct Corners {
  unsigned m[7];
  int v[7];
};

// the step-local index of the vertex on edge J (kPair) of tetrahedron TET; -1 when the owner's mask does not hold it
template <int TET, int J>
__device__ __forceinline__ int edge_vertex(const Corners& c) {
  constexpr int C[4] = {0, kC1[TET], kC2[TET], 7};
  constexpr int own = C[kPair[J][0]];
  constexpr int e = kEdgeOfDiff[C[kPair[J][1]] ^ own];
  return (c.m[own] >> e & 1u) ? c.v[own] + __popc(c.m[own] & ((1u << e) - 1u)) : -1;
}

// The triangles of tetrahedron TET of a cell, to the face rows tb, tb + 1.  Returns false when an edge the case uses is
// not active, an index leaves the step's vertices or a row the faces.
template <int TET>
__device__ __forceinline__ bool emit_tet(const EP& p, unsigned cases, const Corners& c, unsigned vcount, long long& tb) {
  const unsigned cs = cases >> (4 * TET) & 15u;
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
      const bool good = (unsigned)i0 < vcount && (unsigned)i1 < vcount && (unsigned)i2 < vcount;  // (-1 fails here)
      ok = ok && good;
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

__global__ __launch_bounds__(NT) void ridge_emit_kernel(const EP p) {
  const Grid& g = p.m.g;
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
    const unsigned m = c.m[0];
    // a tetrahedron that emits has a corner on the other side of the origin, so the origin owns a vertex: a cell whose
    // origin owns none is not loaded
    Cell cell;
    Signs s;
    unsigned again = 0;
    if (m) {
      load_cell(p.m, r, x, cell);
      s = cell_signs(cell);
      again = edge_mask(cell, s);
    }
    ok = ok && again == m;  // the mask must be the one these operands give
    if (faces) {
      unsigned cases = 0;
      int tw, te;
      if (m && again == m) cases = cell_cases(cell, s, tw, te);
      const int mine = cell_triangles(cases);
      int total;
      const int pre = wave_prefix<4>(mine, total);
      if (mine) {
        long long tb = ct + pre;
        ok = emit_tet<0>(p, cases, c, (unsigned)vcount, tb) && ok;
        ok = emit_tet<1>(p, cases, c, (unsigned)vcount, tb) && ok;
        ok = emit_tet<2>(p, cases, c, (unsigned)vcount, tb) && ok;
        ok = emit_tet<3>(p, cases, c, (unsigned)vcount, tb) && ok;
        ok = emit_tet<4>(p, cases, c, (unsigned)vcount, tb) && ok;
        ok = emit_tet<5>(p, cases, c, (unsigned)vcount, tb) && ok;
      }
      ct += total;
    }
    if (m && ok) {
      const long long base = vstep + c.v[0];
      if (m & 1u) emit_vertex<0>(p, r, x, cell, base);
      if (m & 2u) emit_vertex<1>(p, r, x, cell, base + __popc(m & 1u));
      if (m & 4u) emit_vertex<2>(p, r, x, cell, base + __popc(m & 3u));
      if (m & 8u) emit_vertex<3>(p, r, x, cell, base + __popc(m & 7u));
      if (m & 16u) emit_vertex<4>(p, r, x, cell, base + __popc(m & 15u));
      if (m & 32u) emit_vertex<5>(p, r, x, cell, base + __popc(m & 31u));
      if (m & 64u) emit_vertex<6>(p, r, x, cell, base + __popc(m & 63u));
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

inline long long counts_bytes(int K, int D, int H) { return 4LL * K * D * H * 4; }

Grid make_grid(int K, int D, int H, int W) {
  Grid g;
  g.rows = (long long)K * D * H;
  g.W = W; g.H = H; g.D = D;
  return g;
}

inline unsigned blocks_of(const Grid& g) { return (unsigned)((g.rows + kRows - 1) / kRows); }

}  // namespace

extern "C" long long fs_ridge3d_ws_bytes(int K, int D, int H, int W) {
  const int rc = check_volumes(K, D, H, W, (long long)D * H * W);
  if (rc != FS_OK) return -rc;
  return counts_bytes(K, D, H) + (long long)K * D * H * W;
}

extern "C" int fs_ridge_nodes3d(const float* volumes, int K, int D, int H, int W, long long sstride, int valley,
                                const double* inv_2h, const double* inv_hh, const double* inv_4hh, double strength,
                                double fmin, float* operands, unsigned char* cls, fs_stream_t stream) {
  FS_ENTER();
  FS_REQUIRE_PTR(volumes); FS_REQUIRE_PTR(inv_2h); FS_REQUIRE_PTR(inv_hh); FS_REQUIRE_PTR(inv_4hh);
  FS_REQUIRE_PTR(operands); FS_REQUIRE_PTR(cls);
  const int rc = check_volumes(K, D, H, W, sstride);
  if (rc != FS_OK) return rc;
  NP p;
  for (int a = 0; a < 3; ++a) {
    if (!(inv_2h[a] > 0.0) || !finite_d(inv_2h[a]) || !(inv_hh[a] > 0.0) || !finite_d(inv_hh[a]) ||
        !(inv_4hh[a] > 0.0) || !finite_d(inv_4hh[a]))
      return FS_ERR_ARG;
    p.i2h[a] = inv_2h[a]; p.ihh[a] = inv_hh[a]; p.i4hh[a] = inv_4hh[a];
  }
  if (!(strength >= 0.0) || !finite_d(strength) || !(fmin < HUGE_VAL)) return FS_ERR_ARG;  // (fmin = -inf: no filter)
  p.g = make_grid(K, D, H, W);
  p.vols = volumes; p.sstride = sstride; p.valley = valley != 0;
  p.strength = strength; p.fmin = fmin;
  p.operands = operands; p.cls = cls;
  hipLaunchKernelGGL(ridge_node_kernel, dim3(blocks_of(p.g)), dim3(NT), 0, (hipStream_t)stream, p);
  FS_LAUNCH_CHECK();
  return FS_OK;
}

extern "C" int fs_ridge_count3d(const float* operands, const unsigned char* cls, int K, int D, int H, int W,
                                unsigned char* ws, fs_stream_t stream) {
  FS_ENTER();
  FS_REQUIRE_PTR(operands); FS_REQUIRE_PTR(cls); FS_REQUIRE_PTR(ws);
  const int rc = check_volumes(K, D, H, W, (long long)D * H * W);
  if (rc != FS_OK) return rc;
  if ((uintptr_t)ws & 3u) return FS_ERR_ARG;
  MP p;
  p.g = make_grid(K, D, H, W);
  p.operands = operands; p.cls = cls;
  hipLaunchKernelGGL(ridge_count_kernel, dim3(blocks_of(p.g)), dim3(NT), 0, (hipStream_t)stream, p,
                     ws + counts_bytes(K, D, H), reinterpret_cast<int*>(ws));
  FS_LAUNCH_CHECK();
  return FS_OK;
}

extern "C" int fs_ridge_emit3d(const float* volumes, int K, int D, int H, int W, long long sstride, int valley,
                               const float* operands, const unsigned char* cls, const double* spacing,
                               const unsigned char* ws, const long long* row_offsets, long long V, long long T,
                               float* vertices, float* values_out, int* faces, int* status, fs_stream_t stream) {
  FS_ENTER();
  FS_REQUIRE_PTR(volumes); FS_REQUIRE_PTR(operands); FS_REQUIRE_PTR(cls); FS_REQUIRE_PTR(spacing); FS_REQUIRE_PTR(ws);
  FS_REQUIRE_PTR(row_offsets); FS_REQUIRE_PTR(status);
  if (V > 0) FS_REQUIRE_PTR(vertices);
  if (T > 0) FS_REQUIRE_PTR(faces);
  const int rc = check_volumes(K, D, H, W, sstride);
  if (rc != FS_OK) return rc;
  if (V < 0 || T < 0 || ((uintptr_t)ws & 3u)) return FS_ERR_ARG;
  EP p;
  for (int a = 0; a < 3; ++a) {
    p.h[a] = (float)spacing[a];
    // (what is finite and positive in fp64 must still be so in fp32)
    if (!(spacing[a] > 0.0) || !(p.h[a] > 0.f) || !(p.h[a] < HUGE_VALF)) return FS_ERR_ARG;
  }
  if (V == 0 && T == 0) return FS_OK;  // nothing to write: nothing launched
  p.m.g = make_grid(K, D, H, W);
  p.m.operands = operands; p.m.cls = cls;
  p.vols = volumes; p.sstride = sstride; p.valley = valley != 0;
  p.mask = ws + counts_bytes(K, D, H);
  p.voff = row_offsets;
  p.toff = row_offsets + p.m.g.rows + 1;
  p.verts = vertices; p.vout = values_out; p.faces = faces; p.status = status;
  p.V = V; p.T = T;
  hipLaunchKernelGGL(ridge_emit_kernel, dim3(blocks_of(p.m.g)), dim3(NT), 0, (hipStream_t)stream, p);
  FS_LAUNCH_CHECK();
  return FS_OK;
}
