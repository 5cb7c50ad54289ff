// critical.hip -- the critical points of K step flows: where the piecewise-linear field on the Kuhn split of every cell
// vanishes, and what kind of zero it is (fs_critical_count{2,3}d, fs_critical_emit{2,3}d).  include/flowsci_hip.h
// states the definition; tests/critical_ref.py restates it.
//
// Two streaming passes with a prefix sum over the rows between them (the caller's: plumbing), shaped like
// isosurface.hip: one wave owns one row (k, z, y), a workgroup four consecutive rows, which share their loads in the
// vector cache.
//   count: the wave walks its row in chunks of 63 cells.  A lane loads its own node from the rows (z, y), (z, y+1),
//          (z+1, y), (z+1, y+1) -- 4 C coalesced loads -- and folds "finite", "> 0" and "< 0" of those values into two
//          words of corner bits; the x+1 neighbour's share of the cell is the next lane's words, two cross-lane moves.
//          Almost every cell ends at the sign test on those bits.  Only lanes with a surviving simplex fetch the
//          neighbour's values (from the cache), widen a simplex to fp64 and form its minors, each taking its lowest
//          surviving simplex per trip, so a chunk costs as many trips as its busiest cell has survivors.  One mask byte
//          per node, two int32 per row.
//   emit:  a row without a point ends after reading its two offsets.  Otherwise the in-row prefix is recomputed from
//          the mask bytes (a count below 8: three ballots per chunk) and only flagged cells load their corners.  A point
//          lands at row offset + in-row prefix + rank of its simplex in the mask: nothing is searched, no atomic decides
//          a value or an order, and the result is bitwise reproducible.
// No workgroup waits on another, every loop is bounded by W / 63 or by the simplices of a cell, no LDS, no scratch: the
// corners live in registers and are picked by a switch over constants, never by a runtime index.  All fp64 arithmetic
// is formed without fused multiply-adds, in the header's order.
#include "common.hpp"

#pragma clang fp contract(off)

namespace {

constexpr int NT = 256;
constexpr int kRows = NT / 64;  // rows per workgroup
constexpr int kChunk = 63;      // cells per chunk: lane 63 only lends its node's bits to lane 62
constexpr int kSteps = 256;      // steps whose scales one emit launch carries in its arguments (2 KB of the 4 KB)

// Corner c of a cell sits at the offset (dz, dy, dx) = (c >> 2 & 1, c >> 1 & 1, c & 1) from its origin.  Simplex t has
// the corners 0, c1(t), (c2(t),) NC - 1; its k-th edge runs along axis pi_k(t).
template <int ND> struct Geo;
template <> struct Geo<3> {
  static constexpr int NC = 8, NS = 6;
  __device__ static __forceinline__ int c1(int t) { return t < 2 ? 1 : t < 4 ? 2 : 4; }
  __device__ static __forceinline__ int c2(int t) { return t == 0 || t == 2 ? 3 : t == 1 || t == 4 ? 5 : 6; }
  // the corner set {0, c1, c2, 7} of simplex t as a bitmask
  __device__ static __forceinline__ unsigned corners(int t) { return 0x81u | 1u << c1(t) | 1u << c2(t); }
};
template <> struct Geo<2> {
  static constexpr int NC = 4, NS = 2;
  __device__ static __forceinline__ int c1(int t) { return t == 0 ? 1 : 2; }
  __device__ static __forceinline__ unsigned corners(int t) { return 0x9u | 1u << c1(t); }
};

struct Field {
  const float* flows;
  long long sstride, rows;  // rows = K * D * H
  long long P;              // D * H * W
  int W, H, D;
  double vmin2;  // ((double)(float)vmin)^2
};

struct Row {
  long long k;
  int z, y;
  bool cells;  // the rows y + 1 and (3-D) z + 1 exist
};

template <int ND>
__device__ __forceinline__ Row row_of(const Field& g, long long row) {
  Row r;
  const unsigned u = (unsigned)row;  // (rows <= 2^31 - 1: 32-bit divisions)
  r.y = (int)(u % (unsigned)g.H);
  const unsigned kz = u / (unsigned)g.H;
  r.z = (int)(kz % (unsigned)g.D);
  r.k = (long long)(kz / (unsigned)g.D);
  r.cells = r.y + 1 < g.H && (ND == 2 || r.z + 1 < g.D);
  return r;
}

__device__ __forceinline__ double det2(const double (&a)[2], const double (&b)[2]) { return a[0] * b[1] - a[1] * b[0]; }

__device__ __forceinline__ double det3(const double (&a)[3], const double (&b)[3], const double (&c)[3]) {
  return (a[0] * (b[1] * c[2] - b[2] * c[1]) - a[1] * (b[0] * c[2] - b[2] * c[0])) + a[2] * (b[0] * c[1] - b[1] * c[0]);
}

// The corners of simplex t, widened.  One switch arm per simplex, each with constant corner numbers: the corners stay in
// registers (a chain of selects on t is folded into a runtime index, and the array it indexes into scratch).
template <int T>
__device__ __forceinline__ void gather_t(const float (&f)[8][3], double (&v)[4][3]) {
  constexpr int a = T < 2 ? 1 : T < 4 ? 2 : 4, b = T == 0 || T == 2 ? 3 : T == 1 || T == 4 ? 5 : 6;
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    v[0][r] = (double)f[0][r];
    v[1][r] = (double)f[a][r];
    v[2][r] = (double)f[b][r];
    v[3][r] = (double)f[7][r];
  }
}

__device__ __forceinline__ void gather(const float (&f)[8][3], int t, double (&v)[4][3]) {
  switch (t) {
    case 0: gather_t<0>(f, v); break;
    case 1: gather_t<1>(f, v); break;
    case 2: gather_t<2>(f, v); break;
    case 3: gather_t<3>(f, v); break;
    case 4: gather_t<4>(f, v); break;
    default: gather_t<5>(f, v); break;
  }
}

__device__ __forceinline__ void gather(const float (&f)[4][2], int t, double (&v)[3][2]) {
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    v[0][r] = (double)f[0][r];
    v[2][r] = (double)f[3][r];
  }
  if (t == 0) {
    v[1][0] = (double)f[1][0];
    v[1][1] = (double)f[1][1];
  } else {
    v[1][0] = (double)f[2][0];
    v[1][1] = (double)f[2][1];
  }
}

__device__ __forceinline__ double speed2(const double (&a)[3]) { return (a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]; }
__device__ __forceinline__ double speed2(const double (&a)[2]) { return a[0] * a[0] + a[1] * a[1]; }

// s_i = (-1)^i * the determinant of the corners other than i, in increasing corner number
__device__ __forceinline__ void signed_minors(const double (&v)[4][3], double (&s)[4]) {
  s[0] = det3(v[1], v[2], v[3]);
  s[1] = -det3(v[0], v[2], v[3]);
  s[2] = det3(v[0], v[1], v[3]);
  s[3] = -det3(v[0], v[1], v[2]);
}

__device__ __forceinline__ void signed_minors(const double (&v)[3][2], double (&s)[3]) {
  s[0] = det2(v[1], v[2]);
  s[1] = -det2(v[0], v[2]);
  s[2] = det2(v[0], v[1]);
}

enum { kNone = 0, kPoint = 1, kDegenerate = 2 };

// the largest squared corner speed
template <int ND>
__device__ __forceinline__ double max_speed2(const double (&v)[ND + 1][ND]) {
  double m = speed2(v[0]);
#pragma unroll
  for (int i = 1; i <= ND; ++i) m = fmax(m, speed2(v[i]));
  return m;
}

// Steps 2 and 4-6 of the definition for a simplex whose corners are finite and pass the sign test.
template <int ND>
__device__ __forceinline__ int evaluate(const double (&v)[ND + 1][ND], double vmin2) {
  if (max_speed2<ND>(v) <= vmin2) return kNone;  // quiet
  double s[ND + 1];
  signed_minors(v, s);
  bool bad = false, pos = true, neg = true;
#pragma unroll
  for (int i = 0; i <= ND; ++i) {
    bad = bad || s[i] == 0.0 || !isfinite(s[i]);
    pos = pos && s[i] > 0.0;
    neg = neg && s[i] < 0.0;
  }
  return bad ? kDegenerate : (pos || neg) ? kPoint : kNone;
}

// What the sign test needs of a lane's own node in the 2 (4) rows -- the even corners of its cell --, packed so that
// the odd corners' share is the next lane's word shifted by one: bit 8 r + c of `pos` / `neg` = component r of corner c
// is > 0 / < 0; bit 31 of `pos` = a component is not finite.
template <int ND>
__device__ __forceinline__ void sign_words(const float (&e)[1 << (ND - 1)][ND], unsigned& pos, unsigned& neg) {
  bool fin = true;
  pos = 0;
  neg = 0;
#pragma unroll
  for (int j = 0; j < (1 << (ND - 1)); ++j)
#pragma unroll
    for (int r = 0; r < ND; ++r) {
      fin = fin && isfinite(e[j][r]);
      pos |= (e[j][r] > 0.f ? 1u : 0u) << (8 * r + 2 * j);
      neg |= (e[j][r] < 0.f ? 1u : 0u) << (8 * r + 2 * j);
    }
  pos |= fin ? 0u : 0x80000000u;
}

// Bit t = simplex t passes the sign test: no component has one sign at all of its corners.
template <int ND>
__device__ __forceinline__ unsigned survivors(unsigned pos, unsigned neg) {
  unsigned m = 0;
#pragma unroll
  for (int t = 0; t < Geo<ND>::NS; ++t) {
    const unsigned cs = Geo<ND>::corners(t);
    bool one_sign = false;
#pragma unroll
    for (int r = 0; r < ND; ++r) one_sign = one_sign || (pos >> (8 * r) & cs) == cs || (neg >> (8 * r) & cs) == cs;
    m |= (one_sign ? 0u : 1u) << t;
  }
  return m;
}

template <int ND>
__global__ __launch_bounds__(NT) void critical_count_kernel(const Field g, unsigned char* __restrict__ mask,
                                                            int* __restrict__ np, int* __restrict__ ndeg) {
  constexpr int NC = Geo<ND>::NC;
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * kRows + (threadIdx.x >> 6);
  if (row >= g.rows) return;  // (the whole wave)
  const Row r = row_of<ND>(g, row);
  unsigned char* __restrict__ mrow = mask + (size_t)row * g.W;
  int cp = 0, cd = 0;
  if (r.cells) {
    const float* __restrict__ r00 = g.flows + r.k * g.sstride + ((size_t)r.z * g.H + r.y) * g.W;
    const size_t sy = (size_t)g.W, sz = (size_t)g.W * g.H;
    for (int x0 = 0; x0 < g.W; x0 += kChunk) {
      const int x = x0 + lane;
      const bool in = x < g.W;
      float e[NC / 2][ND];  // this lane's node in the 2 (4) rows: the even corners of its cell
#pragma unroll
      for (int c = 0; c < NC; c += 2) {
        const size_t at = (c & 2 ? sy : 0) + (c & 4 ? sz : 0) + (size_t)x;
#pragma unroll
        for (int q = 0; q < ND; ++q) e[c / 2][q] = in ? r00[(size_t)q * g.P + at] : 0.f;
      }
      unsigned pos, neg;
      sign_words<ND>(e, pos, neg);
      const unsigned pos1 = __shfl_down(pos, 1, 64), neg1 = __shfl_down(neg, 1, 64);  // the odd corners: the next lane's
      const bool cell = lane < kChunk && x + 1 < g.W;
      unsigned m = cell && ((pos | pos1) >> 31) ? 0x80u : 0u;
      unsigned todo = cell && !m ? survivors<ND>((pos | pos1 << 1) & 0xffffffu, neg | neg1 << 1) : 0u;
      float f[NC][ND];
      if (todo) {  // the values of the odd corners are needed by these lanes only: from the cache
#pragma unroll
        for (int c = 0; c < NC; c += 2) {
          const size_t at = (c & 2 ? sy : 0) + (c & 4 ? sz : 0) + (size_t)x + 1;
#pragma unroll
          for (int q = 0; q < ND; ++q) {
            f[c][q] = e[c / 2][q];
            f[c + 1][q] = r00[(size_t)q * g.P + at];
          }
        }
      }
      while (todo) {  // (a lane's trips: its surviving simplices, usually none)
        const int t = __builtin_ctz(todo);
        todo &= todo - 1u;
        double v[ND + 1][ND];
        gather(f, t, v);
        const int what = evaluate<ND>(v, g.vmin2);
        if (what == kPoint) m |= 1u << t;
        if (what == kDegenerate) {
          m |= 0x40u;
          ++cd;
        }
      }
      if (lane < kChunk && in) mrow[x] = (unsigned char)m;
      cp += __popc(m & 0x3fu);
    }
  } else {
    for (int x = lane; x < g.W; x += 64) mrow[x] = 0;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    cp += __shfl_xor(cp, o, 64);
    cd += __shfl_xor(cd, o, 64);
  }
  if (lane == 0) {
    np[row] = cp;
    ndeg[row] = cd;
  }
}

struct EP {
  Field g;
  const unsigned char* mask;
  const long long* off;  // [rows + 1]
  int* cell;
  unsigned char* simplex;
  float* pos;
  double* jac;
  double* inv;
  unsigned char* cls;
  float* vmax;
  int* status;
  long long N;
  int k0;  // the first step of this launch; blockIdx.y counts from it
  double inv_h[3];
  double scale[kSteps];
};

__device__ __forceinline__ int lanes_below(unsigned long long b) {
  return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(b >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)b, 0u));
}

// Exclusive prefix over the wave of a count below 8, and the wave's total.  Every lane of the wave calls it.
__device__ __forceinline__ int wave_prefix3(int c, int& total) {
  int pre = 0;
  total = 0;
#pragma unroll
  for (int b = 0; b < 3; ++b) {
    const unsigned long long m = __ballot((c >> b) & 1);
    pre += lanes_below(m) << b;
    total += __popcll(m) << b;
  }
  return pre;
}

__device__ __forceinline__ unsigned classify3(double P, double Q, double R, double Delta) {
  unsigned n = 0;
  const double PQ = P * Q;
  if (R > 0.0) n = (P > 0.0 && PQ > R) ? 3u : 1u;
  if (R < 0.0) n = (P < 0.0 && PQ < R) ? 0u : 2u;
  const bool fin = isfinite(P) && isfinite(Q) && isfinite(R) && isfinite(Delta);
  if (!fin) n = 0;
  return n | (Delta < 0.0 ? FS_CP_SPIRAL : 0u) | (R == 0.0 || !fin ? FS_CP_DEGENERATE : 0u) |
         (PQ == R ? FS_CP_MARGINAL : 0u);
}

__device__ __forceinline__ unsigned classify2(double tr, double det, double disc) {
  unsigned n = 0;
  if (det < 0.0) n = 1;
  if (det > 0.0) n = tr > 0.0 ? 2u : 0u;
  const bool fin = isfinite(tr) && isfinite(det) && isfinite(disc);
  if (!fin) n = 0;
  return n | (disc < 0.0 ? FS_CP_SPIRAL : 0u) | (det == 0.0 || !fin ? FS_CP_DEGENERATE : 0u) |
         (det > 0.0 && tr == 0.0 ? FS_CP_MARGINAL : 0u);
}

// The point of simplex t of the cell at (i[0], i[1], i[2]) = (x, y, z) to row idx of the outputs.
__device__ __forceinline__ void emit_point(const EP& p, const double (&v)[4][3], const double (&s)[4], double vmax2, int t,
                                           const int (&i)[3], double sc, int cellidx, long long idx) {
  // pi_k: the axis of the k-th edge
  const int p0 = t >> 1, p1 = t == 0 || t == 5 ? 1 : t == 1 || t == 3 ? 2 : 0;
  const double S = ((s[0] + s[1]) + s[2]) + s[3];
  const double l1 = s[1] / S, l2 = s[2] / S, l3 = s[3] / S;
  const double o0 = (l1 + l2) + l3, o1 = l2 + l3, o2 = l3;
  float* __restrict__ ps = p.pos + 3 * idx;
  double* __restrict__ J = p.jac + 9 * idx;
  double j[3][3], e[3][3];
#pragma unroll
  for (int k = 0; k < 3; ++k)
#pragma unroll
    for (int r = 0; r < 3; ++r) e[k][r] = v[k + 1][r] - v[k][r];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const double o = p0 == a ? o0 : p1 == a ? o1 : o2;
    ps[a] = (float)(((double)i[a] + o) / p.inv_h[a]);
    const double ih = p.inv_h[a];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      // (the edge along axis a is edge 0, 1 or 2 of the simplex; selects among values, not among the loads of v)
      const double d = p0 == a ? e[0][r] : p1 == a ? e[1][r] : e[2][r];
      j[r][a] = (d * ih) * sc;
    }
  }
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int a = 0; a < 3; ++a) J[3 * r + a] = j[r][a];
  const double P = (j[0][0] + j[1][1]) + j[2][2];
  const double Q = ((j[0][0] * j[1][1] - j[0][1] * j[1][0]) + (j[0][0] * j[2][2] - j[0][2] * j[2][0])) +
                   (j[1][1] * j[2][2] - j[1][2] * j[2][1]);
  const double R = det3(j[0], j[1], j[2]);
  const double Delta =
      (((((18.0 * P) * Q) * R - (4.0 * ((P * P) * P)) * R) + (P * P) * (Q * Q)) - 4.0 * ((Q * Q) * Q)) - 27.0 * (R * R);
  double* __restrict__ iv = p.inv + 4 * idx;
  iv[0] = P;
  iv[1] = Q;
  iv[2] = R;
  iv[3] = Delta;
  p.cls[idx] = (unsigned char)classify3(P, Q, R, Delta);
  p.cell[idx] = cellidx;
  p.simplex[idx] = (unsigned char)t;
  p.vmax[idx] = (float)(sqrt(vmax2) * sc);
}

__device__ __forceinline__ void emit_point(const EP& p, const double (&v)[3][2], const double (&s)[3], double vmax2, int t,
                                           const int (&i)[3], double sc, int cellidx, long long idx) {
  const int p0 = t;  // t = 0: (x, y); t = 1: (y, x)
  const double S = (s[0] + s[1]) + s[2];
  const double l1 = s[1] / S, l2 = s[2] / S;
  const double o0 = l1 + l2, o1 = l2;
  float* __restrict__ ps = p.pos + 2 * idx;
  double* __restrict__ J = p.jac + 4 * idx;
  double j[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a) {
    const double o = p0 == a ? o0 : o1;
    ps[a] = (float)(((double)i[a] + o) / p.inv_h[a]);
    const double ih = p.inv_h[a];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      const double e0 = v[1][r] - v[0][r], e1 = v[2][r] - v[1][r];
      const double d = p0 == a ? e0 : e1;
      j[r][a] = (d * ih) * sc;
    }
  }
#pragma unroll
  for (int r = 0; r < 2; ++r)
#pragma unroll
    for (int a = 0; a < 2; ++a) J[2 * r + a] = j[r][a];
  const double tr = j[0][0] + j[1][1];
  const double det = j[0][0] * j[1][1] - j[0][1] * j[1][0];
  const double disc = tr * tr - 4.0 * det;
  double* __restrict__ iv = p.inv + 4 * idx;
  iv[0] = tr;
  iv[1] = det;
  iv[2] = disc;
  iv[3] = 0.0;
  p.cls[idx] = (unsigned char)classify2(tr, det, disc);
  p.cell[idx] = cellidx;
  p.simplex[idx] = (unsigned char)t;
  p.vmax[idx] = (float)(sqrt(vmax2) * sc);
}

// grid: (row blocks of one step, steps of this launch)
template <int ND>
__global__ __launch_bounds__(NT) void critical_emit_kernel(const EP p) {
  constexpr int NC = Geo<ND>::NC;
  const Field& g = p.g;
  const int lane = threadIdx.x & 63;
  const int rows_per_step = g.D * g.H;
  const int rin = (int)blockIdx.x * kRows + (int)(threadIdx.x >> 6);
  if (rin >= rows_per_step) return;  // (the whole wave)
  const int ks = (int)blockIdx.y;    // uniform: the scale is read from the launch's arguments
  const long long k = (long long)p.k0 + ks;
  const long long row = k * rows_per_step + rin;
  const long long n0 = p.off[row], nr = p.off[row + 1] - n0;
  if (nr == 0) return;  // (most rows end here)
  const double sc = p.scale[ks];
  const int y = rin % g.H, z = rin / g.H;
  const bool cells = y + 1 < g.H && (ND == 2 || z + 1 < g.D);
  const float* __restrict__ r00 = g.flows + k * g.sstride + ((size_t)z * g.H + y) * g.W;
  const size_t sy = (size_t)g.W, sz = (size_t)g.W * g.H;
  const unsigned char* __restrict__ mrow = p.mask + (size_t)row * g.W;
  long long carry = n0;
  bool ok = cells && n0 >= 0 && nr > 0 && n0 + nr <= p.N;
  for (int x0 = 0; x0 < g.W; x0 += 64) {
    const int x = x0 + lane;
    unsigned m = x < g.W ? mrow[x] & 0x3fu : 0u;
    // a mask that is not this field's could flag a cell that leaves it: nothing is read out there
    if (m && !(cells && x + 1 < g.W)) {
      ok = false;
      m = 0;
    }
    int total;
    const int pre = wave_prefix3(__popc(m), total);
    long long idx = carry + pre;
    carry += total;
    if (m && ok && idx >= n0 && idx + __popc(m) <= n0 + nr) {
      float f[NC][ND];
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        const size_t at = (c & 2 ? sy : 0) + (c & 4 ? sz : 0) + (size_t)(x + (c & 1));
#pragma unroll
        for (int q = 0; q < ND; ++q) f[c][q] = r00[(size_t)q * g.P + at];
      }
      const int i[3] = {x, y, z};
      const int cellidx = (z * g.H + y) * g.W + x;
      while (m) {
        const int t = __builtin_ctz(m);
        m &= m - 1u;
        double v[ND + 1][ND], s[ND + 1];
        gather(f, t, v);
        signed_minors(v, s);  // (the bits the count pass saw)
        emit_point(p, v, s, max_speed2<ND>(v), t, i, sc, cellidx, idx);
        ++idx;
      }
    } else if (m) {
      ok = false;
    }
  }
  // the masks must add up to what the offsets say this row owns
  ok = ok && carry - n0 == nr;
  if (__ballot(!ok) != 0ull && lane == 0) atomicOr(p.status, 1);
}

// FS_OK, or what is wrong with the fields' geometry
int check_fields(int nd, int K, int C, int D, int H, int W, long long sstride) {
  if (K < 1 || C != nd || D < (nd == 3 ? 2 : 1) || H < 2 || W < 2) return FS_ERR_SHAPE;
  const long long P = (long long)D * H * W;
  if (P >= 0x7fffffffLL || sstride < (long long)C * P) return FS_ERR_SHAPE;
  if ((long long)K * D * H > 0x7fffffffLL) return FS_ERR_SHAPE;
  return FS_OK;
}

inline long long counts_bytes(int K, int D, int H) { return (2LL * K * D * H * 4 + 15) / 16 * 16; }

inline bool vmin_ok(double vmin) { return vmin >= 0.0 && vmin < HUGE_VAL && (double)(float)vmin < HUGE_VAL; }

Field make_field(const float* flows, int K, int D, int H, int W, long long sstride, double vmin) {
  Field g;
  g.flows = flows; g.sstride = sstride; g.rows = (long long)K * D * H; g.P = (long long)D * H * W;
  g.W = W; g.H = H; g.D = D;
  const double vm = (double)(float)vmin;
  g.vmin2 = vm * vm;
  return g;
}

long long ws_bytes(int nd, int K, int D, int H, int W) {
  const int rc = check_fields(nd, K, nd, D, H, W, (long long)nd * D * H * W);
  if (rc != FS_OK) return -rc;
  return counts_bytes(K, D, H) + (long long)K * D * H * W;
}

int count(int nd, const float* flows, int K, int C, int D, int H, int W, long long sstride, double vmin, unsigned char* ws,
          fs_stream_t stream) {
  FS_ENTER();
  FS_REQUIRE_PTR(flows); FS_REQUIRE_PTR(ws);
  const int rc = check_fields(nd, K, C, D, H, W, sstride);
  if (rc != FS_OK) return rc;
  if (!vmin_ok(vmin) || ((uintptr_t)ws & 15u)) return FS_ERR_ARG;
  const Field g = make_field(flows, K, D, H, W, sstride, vmin);
  int* np = reinterpret_cast<int*>(ws);
  const dim3 grid((unsigned)((g.rows + kRows - 1) / kRows));
  if (nd == 3)
    hipLaunchKernelGGL(critical_count_kernel<3>, grid, dim3(NT), 0, (hipStream_t)stream, g, ws + counts_bytes(K, D, H), np,
                       np + g.rows);
  else
    hipLaunchKernelGGL(critical_count_kernel<2>, grid, dim3(NT), 0, (hipStream_t)stream, g, ws + counts_bytes(K, D, H), np,
                       np + g.rows);
  FS_LAUNCH_CHECK();
  return FS_OK;
}

int emit(int nd, const float* flows, int K, int C, int D, int H, int W, long long sstride, const double* inv_h,
         const double* scale, double vmin, const unsigned char* ws, const long long* row_offsets, long long N, int* cell,
         unsigned char* simplex, float* pos, double* jac, double* inv, unsigned char* cls, float* vmax, int* status,
         fs_stream_t stream) {
  FS_ENTER();
  FS_REQUIRE_PTR(flows); FS_REQUIRE_PTR(inv_h); FS_REQUIRE_PTR(scale); FS_REQUIRE_PTR(ws); FS_REQUIRE_PTR(row_offsets);
  FS_REQUIRE_PTR(status);
  if (N > 0) {
    FS_REQUIRE_PTR(cell); FS_REQUIRE_PTR(simplex); FS_REQUIRE_PTR(pos); FS_REQUIRE_PTR(jac); FS_REQUIRE_PTR(inv);
    FS_REQUIRE_PTR(cls); FS_REQUIRE_PTR(vmax);
  }
  const int rc = check_fields(nd, K, C, D, H, W, sstride);
  if (rc != FS_OK) return rc;
  if (!vmin_ok(vmin) || N < 0 || ((uintptr_t)ws & 15u)) return FS_ERR_ARG;
  EP p;
  for (int a = 0; a < 3; ++a) {
    p.inv_h[a] = a < nd ? inv_h[a] : 1.0;
    if (!fs::pos_finite(p.inv_h[a])) return FS_ERR_ARG;
  }
  for (int k = 0; k < K; ++k)
    if (!fs::pos_finite(scale[k])) return FS_ERR_ARG;
  if (N == 0) return FS_OK;  // nothing to write: nothing launched
  p.g = make_field(flows, K, D, H, W, sstride, vmin);
  p.mask = ws + counts_bytes(K, D, H);
  p.off = row_offsets;
  p.cell = cell; p.simplex = simplex; p.pos = pos; p.jac = jac; p.inv = inv; p.cls = cls; p.vmax = vmax;
  p.status = status; p.N = N;
  const unsigned bx = (unsigned)((D * H + kRows - 1) / kRows);
  for (int k0 = 0; k0 < K; k0 += kSteps) {
    const int kc = K - k0 < kSteps ? K - k0 : kSteps;
    p.k0 = k0;
    for (int k = 0; k < kSteps; ++k) p.scale[k] = k < kc ? scale[k0 + k] : 0.0;
    if (nd == 3)
      hipLaunchKernelGGL(critical_emit_kernel<3>, dim3(bx, (unsigned)kc), dim3(NT), 0, (hipStream_t)stream, p);
    else
      hipLaunchKernelGGL(critical_emit_kernel<2>, dim3(bx, (unsigned)kc), dim3(NT), 0, (hipStream_t)stream, p);
    FS_LAUNCH_CHECK();
  }
  return FS_OK;
}

}  // namespace

extern "C" long long fs_critical2d_ws_bytes(int K, int H, int W) { return ws_bytes(2, K, 1, H, W); }

extern "C" long long fs_critical3d_ws_bytes(int K, int D, int H, int W) { return ws_bytes(3, K, D, H, W); }

extern "C" int fs_critical_count2d(const float* flows, int K, int C, int H, int W, long long flow_sstride, double vmin,
                                   unsigned char* ws, fs_stream_t stream) {
  return count(2, flows, K, C, 1, H, W, flow_sstride, vmin, ws, stream);
}

extern "C" int fs_critical_count3d(const float* flows, int K, int C, int D, int H, int W, long long flow_sstride,
                                   double vmin, unsigned char* ws, fs_stream_t stream) {
  return count(3, flows, K, C, D, H, W, flow_sstride, vmin, ws, stream);
}

extern "C" int fs_critical_emit2d(const float* flows, int K, int C, int H, int W, long long flow_sstride,
                                  const double* inv_h, const double* scale, double vmin, const unsigned char* ws,
                                  const long long* row_offsets, long long N, int* cell, unsigned char* simplex, float* pos,
                                  double* jac, double* inv, unsigned char* cls, float* vmax, int* status,
                                  fs_stream_t stream) {
  return emit(2, flows, K, C, 1, H, W, flow_sstride, inv_h, scale, vmin, ws, row_offsets, N, cell, simplex, pos, jac, inv,
              cls, vmax, status, stream);
}

extern "C" int fs_critical_emit3d(const float* flows, int K, int C, int D, int H, int W, long long flow_sstride,
                                  const double* inv_h, const double* scale, double vmin, const unsigned char* ws,
                                  const long long* row_offsets, long long N, int* cell, unsigned char* simplex, float* pos,
                                  double* jac, double* inv, unsigned char* cls, float* vmax, int* status,
                                  fs_stream_t stream) {
  return emit(3, flows, K, C, D, H, W, flow_sstride, inv_h, scale, vmin, ws, row_offsets, N, cell, simplex, pos, jac, inv,
              cls, vmax, status, stream);
}
