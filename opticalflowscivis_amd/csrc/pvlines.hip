// pvlines.hip -- vortex core lines by the parallel-vectors operator: the segments of the locus v || w on the Kuhn split
// of every cell of K steps (fs_pv_count3d, fs_pv_emit3d).  include/flowsci_hip.h states the definition;
// tests/pv_ref.py restates it.
//
// The unit of work is a triangular FACE, not a tetrahedron: a point of the locus lies on a face, and the two tetrahedra
// that share the face must see the same point.  Every face has one owner -- the node that is its lowest corner, 12 slots
// per node -- and is only ever solved in the owner's frame by one function, solve_face: whoever solves it, in whichever
// pass, runs the same operations on the same nodes in the same order.
//   count: two kernels on the stream.
//          faces: one wave per row (k, z, y), one lane per node.  A lane loads the 8 corners of its cell (v, w, aux: 7
//                 values each, neighbours from the vector cache), and screens its 12 owned faces in registers: finite,
//                 not quiet, and the Bernstein test of step 2 -- multiplications and compares only, branch-free,
//                 unrolled over constant corner numbers.  Almost every face ends there.  A lane with survivors takes
//                 them one per trip: it re-reads the face's 18 values by slot (from the cache: the 56 screening
//                 registers are dead by then), forms the pencil's cubic and brackets its roots.  The accepted points
//                 of a slot, 0..3, go to two bits of the node's word in ws; nothing else is kept.
//          tets:  one lane per cell reads the words of its 8 corners (4 of them own its faces, all 8 say "finite"),
//                 adds up each tetrahedron's four faces and writes one mask byte per cell and four int32 per row.
//   emit:  a row without a segment ends after reading its two offsets.  Otherwise the in-row prefix is recomputed from
//          the mask bytes and a lane takes one (tetrahedron, face) pair per trip: the faces of its flagged tetrahedra
//          whose count is not 0, re-solved in the owner's frame, their endpoints written in (face, rank) order.  No atomic decides a value or an order.
// The cost is fp64 VALU work: ~1100 operations of screening per node against 28 bytes read, and 64 bisections of a
// cubic per surviving face on the few lanes that have one, the rest of the wave idle.  Two things are done about that
// divergence: the trip loops keep it to one solve_face body per wave -- lanes with survivors run it together, however
// their slots (in the emit pass: their tetrahedra) differ, instead of once per slot -- and the three intervals of a
// face are bisected side by side, three independent chains in one loop.  profiles/pv.txt has the times and what is
// and is not known about the bound.  No LDS, no scratch: corners are picked by constants in the screening and
// by address arithmetic in load_face, never by a runtime index into registers.
#include "common.hpp"

#pragma clang fp contract(off)

namespace {

constexpr int NT = 256;
constexpr int kRows = NT / 64;  // rows per workgroup
constexpr int kBisections = 64, kNewtons = 2;

// Slot s of a node: the face with the corners 0 < mid(s) < hi(s) of the cell the node is the origin of (corner c at
// the offset (dz, dy, dx) = (c >> 2 & 1, c >> 1 & 1, c & 1)).  mid: 1 1 2 2 4 4 3 5 6 1 2 4, hi: 3 5 3 6 5 6 7 7 7 7 7 7.
__host__ __device__ constexpr int slot_mid(int s) { return (int)(0x421653442211ull >> (4 * s)) & 15; }
__host__ __device__ constexpr int slot_hi(int s) { return (int)(0x777777656353ull >> (4 * s)) & 15; }
// Face f of tetrahedron t: the corner of the cell whose node owns it, and its slot there.
__host__ __device__ constexpr int tet_c1(int t) { return t < 2 ? 1 : t < 4 ? 2 : 4; }
__host__ __device__ constexpr int face_owner(int t, int f) { return f == 0 ? tet_c1(t) : 0; }
__host__ __device__ constexpr int face_slot(int t, int f) {
  return f == 0 ? (int)(0x204153u >> (4 * t)) & 15 : f == 1 ? 6 + ((int)(0x212010u >> (4 * t)) & 15) : f == 2 ? 9 + (t >> 1) : t;
}

struct Fields {
  const float* v;
  const float* w;
  const float* aux;         // or nullptr
  long long vs, wst, as;    // step strides in elements
  long long rows;           // K * D * H
  long long P;              // D * H * W
  int W, H, D;
  double vmin2, wmin2;  // ((double)(float)vmin)^2, likewise wmin
};

struct Face {
  double v[3][3], w[3][3];  // [corner][component]
};

__device__ __forceinline__ double det3(const double (&a)[3], const double (&b)[3], const double (&c)[3]) {
  return (a[0] * (b[1] * c[2] - b[2] * c[1]) - a[1] * (b[0] * c[2] - b[2] * c[0])) + a[2] * (b[0] * c[1] - b[1] * c[0]);
}

__device__ __forceinline__ double sumsq(const double (&a)[3]) { return (a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]; }

// Step 1 for one corner.
__device__ __forceinline__ bool quiet(const double (&v)[3], const double (&w)[3], double vmin2, double wmin2) {
  return sumsq(v) <= vmin2 || sumsq(w) <= wmin2;
}

// Step 2 on a face with finite corners: some component of v x w has one sign on the whole face.  The six numbers are
// finite (products of three fp32 values do not overflow fp64), so "all > 0" is "the smallest > 0": two compares per
// component instead of twelve, which keeps the screening of twelve faces out of the scalar registers.
__device__ __forceinline__ bool rejected(const double (&v)[3][3], const double (&w)[3][3]) {
  bool out = false;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int j = (k + 1) % 3, l = (k + 2) % 3;
    double six[6];
#pragma unroll
    for (int i = 0; i < 3; ++i) six[i] = v[i][j] * w[i][l] - v[i][l] * w[i][j];
    six[3] = (v[0][j] * w[1][l] - v[0][l] * w[1][j]) + (v[1][j] * w[0][l] - v[1][l] * w[0][j]);
    six[4] = (v[0][j] * w[2][l] - v[0][l] * w[2][j]) + (v[2][j] * w[0][l] - v[2][l] * w[0][j]);
    six[5] = (v[1][j] * w[2][l] - v[1][l] * w[2][j]) + (v[2][j] * w[1][l] - v[2][l] * w[1][j]);
    const double mn = fmin(fmin(fmin(six[0], six[1]), fmin(six[2], six[3])), fmin(six[4], six[5]));
    const double mx = fmax(fmax(fmax(six[0], six[1]), fmax(six[2], six[3])), fmax(six[4], six[5]));
    out = out || mn > 0.0 || mx < 0.0;
  }
  return out;
}

enum { kAccMask = 3, kDegenerate = 4 };

// Steps 3-5 on a face that passed steps 1 and 2.  sink(r, lambda, swapped, l0, l1, l2) is called for every accepted
// root in interval order, r its rank among the face's roots.  Returns the number of accepted roots, or kDegenerate.
template <class Sink>
__device__ __forceinline__ int solve_face(const Face& f, Sink&& sink) {
  const double dV = det3(f.v[0], f.v[1], f.v[2]), dW = det3(f.w[0], f.w[1], f.w[2]);
  const bool swapped = !(fabs(dW) >= fabs(dV));
  double A[3][3], B[3][3];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      A[i][r] = swapped ? f.v[i][r] : f.w[i][r];
      B[i][r] = swapped ? f.w[i][r] : f.v[i][r];
    }
  const double dA = swapped ? dV : dW, dB = swapped ? dW : dV;
  if (dA == 0.0 || !isfinite(dA)) return kDegenerate;
  const double m1 = (det3(A[0], B[1], B[2]) + det3(B[0], A[1], B[2])) + det3(B[0], B[1], A[2]);
  const double m2 = (det3(A[0], A[1], B[2]) + det3(A[0], B[1], A[2])) + det3(B[0], A[1], A[2]);
  const double a = -(m2 / dA), b = m1 / dA, c = -(dB / dA);
  double mx = fabs(a);
  if (fabs(b) > mx) mx = fabs(b);
  if (fabs(c) > mx) mx = fabs(c);
  const double R = 1.0 + mx;
  const double disc = a * a - 3.0 * b;
  double k1 = -R, k2 = -R;
  if (disc > 0.0) {
    const double sq = sqrt(disc);
    k1 = (-a - sq) / 3.0;
    k2 = (-a + sq) / 3.0;
  }
  auto p = [&](double x) { return ((x + a) * x + b) * x + c; };
  auto dp = [&](double x) { return (3.0 * x + 2.0 * a) * x + b; };
  // The three intervals are bisected side by side: three independent chains of dependent fp64 operations in one loop of
  // 64 trips instead of three loops one after the other (the lane waits on latency, not on issue).  An interval
  // without a root is bisected along and ignored: every interval's arithmetic is what it would be on its own.
  double los[3] = {-R, k1, k2}, his[3] = {k1, k2, R};
  bool sls[3];
  unsigned has = 0;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    sls[i] = p(los[i]) < 0.0;
    has |= (los[i] < his[i] && sls[i] != (p(his[i]) < 0.0) ? 1u : 0u) << i;
  }
  if (!has) return 0;
#pragma unroll 1
  for (int it = 0; it < kBisections; ++it) {
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const double m = 0.5 * (los[i] + his[i]);
      const bool left = (p(m) < 0.0) == sls[i];
      los[i] = left ? m : los[i];
      his[i] = left ? his[i] : m;
    }
  }
  int nroots = 0, nacc = 0;
#pragma unroll 1
  for (int iv = 0; iv < 3; ++iv) {  // (selects among values: the brackets stay in registers)
    if (!(has >> iv & 1u)) continue;
    const double lo = iv == 0 ? los[0] : iv == 1 ? los[1] : los[2];
    const double hi = iv == 0 ? his[0] : iv == 1 ? his[1] : his[2];
    double x = 0.5 * (lo + hi);
#pragma unroll
    for (int it = 0; it < kNewtons; ++it) {
      const double xn = x - p(x) / dp(x);
      if (isfinite(xn) && xn >= lo && xn <= hi) x = xn;
    }
    double N[3][3];  // [component][corner]
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int i = 0; i < 3; ++i) N[r][i] = B[i][r] - x * A[i][r];
    double n[3], best;
    {
      const double (&u)[3] = N[0];
      const double (&q)[3] = N[1];
      n[0] = u[1] * q[2] - u[2] * q[1];
      n[1] = u[2] * q[0] - u[0] * q[2];
      n[2] = u[0] * q[1] - u[1] * q[0];
      best = sumsq(n);
    }
#pragma unroll
    for (int pr = 0; pr < 2; ++pr) {
      const double (&u)[3] = N[pr];  // the pairs (0, 2) and (1, 2)
      const double (&q)[3] = N[2];
      double n2[3];
      n2[0] = u[1] * q[2] - u[2] * q[1];
      n2[1] = u[2] * q[0] - u[0] * q[2];
      n2[2] = u[0] * q[1] - u[1] * q[0];
      const double s2 = sumsq(n2);
      if (s2 > best) {
        best = s2;
        n[0] = n2[0];
        n[1] = n2[1];
        n[2] = n2[2];
      }
    }
    if ((n[0] > 0.0 && n[1] > 0.0 && n[2] > 0.0) || (n[0] < 0.0 && n[1] < 0.0 && n[2] < 0.0)) {
      const double S = (n[0] + n[1]) + n[2];
      sink(nroots, x, swapped, n[0] / S, n[1] / S, n[2] / S);
      ++nacc;
    }
    ++nroots;
  }
  return nacc;
}

struct Row {
  long long k;
  int z, y;
};

__device__ __forceinline__ Row row_of(const Fields& g, long long row) {
  Row r;
  const unsigned u = (unsigned)row;  // (rows <= 2^31 - 1: 32-bit divisions)
  r.y = (int)(u % (unsigned)g.H);
  const unsigned kz = u / (unsigned)g.H;
  r.z = (int)(kz % (unsigned)g.D);
  r.k = (long long)(kz / (unsigned)g.D);
  return r;
}

// The face in slot s of the node (ox, oy, oz) of the step whose planes start at vb, wb (and ab, or nullptr), widened, and its corners' aux (0 without aux).  False, and
// nothing read, when a corner is no node of the grid.
__device__ __forceinline__ bool load_face(const Fields& g, const float* __restrict__ vb, const float* __restrict__ wb,
                                          const float* __restrict__ ab, int ox, int oy, int oz, int s, Face& f,
                                          double (&ax)[3]) {
  const int cs[3] = {0, slot_mid(s), slot_hi(s)};
  bool ok = true;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const int cx = ox + (cs[i] & 1), cy = oy + (cs[i] >> 1 & 1), cz = oz + (cs[i] >> 2 & 1);
    ok = ok && cx >= 0 && cy >= 0 && cz >= 0 && cx < g.W && cy < g.H && cz < g.D;
  }
  if (!ok) return false;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const int cx = ox + (cs[i] & 1), cy = oy + (cs[i] >> 1 & 1), cz = oz + (cs[i] >> 2 & 1);
    const size_t at = ((size_t)cz * g.H + cy) * g.W + cx;
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      f.v[i][q] = (double)vb[(size_t)q * g.P + at];
      f.w[i][q] = (double)wb[(size_t)q * g.P + at];
    }
    ax[i] = ab ? (double)ab[at] : 0.0;
  }
  return true;
}

__global__ __launch_bounds__(NT) void pv_face_kernel(const Fields g, unsigned* __restrict__ fbits, int* __restrict__ ndeg) {
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * kRows + (threadIdx.x >> 6);
  if (row >= g.rows) return;  // (the whole wave)
  const Row r = row_of(g, row);
  // seven plane pointers at the row's first node, uniform; a corner adds a 32-bit lane offset (below D*H*W < 2^31)
  const float* __restrict__ vb = g.v + r.k * g.vs;
  const float* __restrict__ wb = g.w + r.k * g.wst;
  const float* __restrict__ ab = g.aux ? g.aux + r.k * g.as : nullptr;
  const size_t rowbase = ((size_t)r.z * g.H + r.y) * g.W;
  const float* __restrict__ pl[7];
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    pl[q] = vb + (size_t)q * g.P + rowbase;
    pl[3 + q] = wb + (size_t)q * g.P + rowbase;
  }
  pl[6] = ab ? ab + rowbase : nullptr;
  unsigned* __restrict__ frow = fbits + (size_t)row * g.W;
  const unsigned sy = (unsigned)g.W, sz = (unsigned)g.W * (unsigned)g.H;
  int cd = 0;
  for (int x0 = 0; x0 < g.W; x0 += 64) {
    const int x = x0 + lane;
    const bool in = x < g.W;
    float f[8][7];
    unsigned okc = 0;  // bit c: corner c is a node, and every value at it is finite
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      const bool ok = in && x + (c & 1) < g.W && r.y + (c >> 1 & 1) < g.H && r.z + (c >> 2 & 1) < g.D;
      const unsigned at = ok ? (c & 2 ? sy : 0u) + (c & 4 ? sz : 0u) + (unsigned)(x + (c & 1)) : 0u;
      bool fin = ok;
#pragma unroll
      for (int q = 0; q < 6; ++q) {
        f[c][q] = ok ? pl[q][at] : 0.f;
        fin = fin && isfinite(f[c][q]);
      }
      f[c][6] = ok && pl[6] ? pl[6][at] : 0.f;
      fin = fin && isfinite(f[c][6]);
      okc |= (fin ? 1u : 0u) << c;
    }
    unsigned bits = in && !(okc & 1u) ? 1u << 24 : 0u;  // this node has a value that is not finite
    unsigned qc = 0;  // bit c: corner c is quiet
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      const double v[3] = {(double)f[c][0], (double)f[c][1], (double)f[c][2]};
      const double w[3] = {(double)f[c][3], (double)f[c][4], (double)f[c][5]};
      qc |= (quiet(v, w, g.vmin2, g.wmin2) ? 1u : 0u) << c;
    }
    unsigned todo = 0;
#pragma unroll
    for (int s = 0; s < 12; ++s) {
      constexpr unsigned one = 1u;
      const int cs[3] = {0, slot_mid(s), slot_hi(s)};
      const unsigned need = one | one << cs[1] | one << cs[2];
      double v[3][3], w[3][3];
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int q = 0; q < 3; ++q) {
          v[i][q] = (double)f[cs[i]][q];
          w[i][q] = (double)f[cs[i]][3 + q];
        }
      const bool rej = rejected(v, w);
      todo |= ((okc & need) == need && (qc & need) != need && !rej ? 1u : 0u) << s;
    }
    while (todo) {  // (a lane's trips: its surviving faces, usually none)
      const int s = __builtin_ctz(todo);
      todo &= todo - 1u;
      Face fc;
      double ax[3];
      if (!load_face(g, vb, wb, ab, x, r.y, r.z, s, fc, ax)) continue;
      const int res = solve_face(fc, [](int, double, bool, double, double, double) {});
      bits |= (unsigned)(res & kAccMask) << (2 * s);
      cd += res >> 2;
    }
    if (in) frow[x] = bits;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) cd += __shfl_xor(cd, o, 64);
  if (lane == 0) ndeg[row] = cd;
}

__device__ __forceinline__ int face_count(const unsigned (&b)[8], int t, int f) {
  return (int)(b[face_owner(t, f)] >> (2 * face_slot(t, f))) & 3;
}

enum { kMaskAmbiguous = 64, kMaskNonfinite = 128 };

__global__ __launch_bounds__(NT) void pv_tet_kernel(const Fields g, const unsigned* __restrict__ fbits,
                                                    unsigned char* __restrict__ tmask, int* __restrict__ nseg,
                                                    int* __restrict__ namb, int* __restrict__ nnf) {
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * kRows + (threadIdx.x >> 6);
  if (row >= g.rows) return;  // (the whole wave)
  const Row r = row_of(g, row);
  const bool cells = r.y + 1 < g.H && r.z + 1 < g.D;
  const unsigned* __restrict__ frow = fbits + (size_t)row * g.W;
  unsigned char* __restrict__ mrow = tmask + (size_t)row * g.W;
  const size_t sy = (size_t)g.W, sz = (size_t)g.W * g.H;
  int cs = 0, ca = 0, cn = 0;
  for (int x0 = 0; x0 < g.W; x0 += 64) {
    const int x = x0 + lane;
    unsigned m = 0;
    if (cells && x + 1 < g.W) {
      unsigned b[8];
      unsigned any = 0;
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        b[c] = frow[(c & 2 ? sy : 0) + (c & 4 ? sz : 0) + (size_t)(x + (c & 1))];
        any |= b[c];
      }
      if (any >> 24 & 1u) {
        m = kMaskNonfinite;
        ++cn;
      } else {
#pragma unroll
        for (int t = 0; t < 6; ++t) {
          const int n = (face_count(b, t, 0) + face_count(b, t, 1)) + (face_count(b, t, 2) + face_count(b, t, 3));
          if (n == 2) {
            m |= 1u << t;
            ++cs;
          } else if (n != 0) {
            m |= kMaskAmbiguous;
            ++ca;
          }
        }
      }
    }
    if (x < g.W) mrow[x] = (unsigned char)m;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    cs += __shfl_xor(cs, o, 64);
    ca += __shfl_xor(ca, o, 64);
    cn += __shfl_xor(cn, o, 64);
  }
  if (lane == 0) {
    nseg[row] = cs;
    namb[row] = ca;
    nnf[row] = cn;
  }
}

struct EP {
  Fields g;
  const unsigned* fbits;
  const unsigned char* tmask;
  const long long* off;  // [rows + 1]
  int* cell;
  unsigned char* simplex;
  unsigned char* face;
  long long* key;
  float* pos;
  double* mu;
  float* vel;
  float* aux;
  long long N;
  int* status;
  double inv_h[3];
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

// Endpoint e (0 or 1) of segment idx: the accepted root of rank r of the face in slot s of the node (o[0], o[1], o[2]).
__device__ __forceinline__ void write_end(const EP& p, long long idx, int e, int fnum, long long node, const int (&o)[3],
                                          int s, const Face& fc, const double (&ax)[3], int r, double lam, bool swapped,
                                          double l0, double l1, double l2) {
  const long long at = 2 * idx + e;
  const int mid = slot_mid(s), hi = slot_hi(s);
  p.face[at] = (unsigned char)fnum;
  p.key[at] = 4 * (node * 12 + s) + r;
  p.mu[at] = swapped ? lam : 1.0 / lam;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    double c = (double)o[a];
    if (mid >> a & 1) c = c + l1;
    if (hi >> a & 1) c = c + l2;
    p.pos[3 * at + a] = (float)(c / p.inv_h[a]);
    p.vel[3 * at + a] = (float)((l0 * fc.v[0][a] + l1 * fc.v[1][a]) + l2 * fc.v[2][a]);
  }
  if (p.aux) p.aux[at] = (float)((l0 * ax[0] + l1 * ax[1]) + l2 * ax[2]);
}

__global__ __launch_bounds__(NT) void pv_emit_kernel(const EP p) {
  const Fields& g = p.g;
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * kRows + (threadIdx.x >> 6);
  if (row >= g.rows) return;  // (the whole wave)
  const long long n0 = p.off[row], nr = p.off[row + 1] - n0;
  if (nr == 0) return;  // (most rows end here)
  const Row r = row_of(g, row);
  const bool cells = r.y + 1 < g.H && r.z + 1 < g.D;
  const float* __restrict__ vb = g.v + r.k * g.vs;
  const float* __restrict__ wb = g.w + r.k * g.wst;
  const float* __restrict__ ab = g.aux ? g.aux + r.k * g.as : nullptr;
  const unsigned char* __restrict__ mrow = p.tmask + (size_t)row * g.W;
  const unsigned* __restrict__ frow = p.fbits + (size_t)row * g.W;
  const size_t sy = (size_t)g.W, sz = (size_t)g.W * g.H;
  long long carry = n0;
  bool ok = cells && n0 >= 0 && nr > 0 && n0 + nr <= p.N;
  for (int x0 = 0; x0 < g.W; x0 += 64) {
    const int x = x0 + lane;
    unsigned m = x < g.W ? mrow[x] & 0x3fu : 0u;
    // a mask that is not these fields' could flag a cell that leaves them: nothing is read out there
    if (m && !(cells && x + 1 < g.W)) {
      ok = false;
      m = 0;
    }
    int total;
    const int pre = wave_prefix3(__popc(m), total);
    long long idx = carry + pre;
    carry += total;
    if (m && ok && idx >= n0 && idx + __popc(m) <= n0 + nr) {
      const int cellidx = (r.z * g.H + r.y) * g.W + x;
      // One trip per (tetrahedron, face) with points, not a loop of faces inside a loop of tetrahedra: the lanes of a
      // wave meet in one solve_face however their tetrahedra differ.  Bit 4 t + f of `work`; the endpoints written so
      // far by tetrahedron t in bits 4 t .. 4 t + 3 of `ends`.
      unsigned word[8];
#pragma unroll
      for (int c = 0; c < 8; ++c)
        word[c] = c == 0 || c == 1 || c == 2 || c == 4 ? frow[(c & 2 ? sy : 0) + (c & 4 ? sz : 0) + (size_t)(x + (c & 1))] : 0u;
      unsigned work = 0, ends = 0, want = 0;
#pragma unroll
      for (int t = 0; t < 6; ++t) {
        if (!(m >> t & 1u)) continue;
        want |= 2u << (4 * t);
        const long long seg = idx + __popc(m & ((1u << t) - 1u));
        p.cell[seg] = cellidx;
        p.simplex[seg] = (unsigned char)t;
#pragma unroll
        for (int f = 0; f < 4; ++f)
          work |= (word[face_owner(t, f)] >> (2 * face_slot(t, f)) & 3u ? 1u : 0u) << (4 * t + f);
      }
      while (work) {
        const int tf = __builtin_ctz(work);
        work &= work - 1u;
        const int t = tf >> 2, f = tf & 3;
        const long long seg = idx + __popc(m & ((1u << t) - 1u));
        const int oc = face_owner(t, f), s = face_slot(t, f);
        const int o[3] = {x + (oc & 1), r.y + (oc >> 1 & 1), r.z + (oc >> 2 & 1)};
        Face fc;
        double ax[3];
        if (!load_face(g, vb, wb, ab, o[0], o[1], o[2], s, fc, ax)) continue;
        const long long node = ((long long)o[2] * g.H + o[1]) * g.W + o[0];
        int e = (int)(ends >> (4 * t)) & 15;
        solve_face(fc, [&](int rk, double lam, bool swapped, double l0, double l1, double l2) {
          if (e < 2) write_end(p, seg, e, f, node, o, s, fc, ax, rk, lam, swapped, l0, l1, l2);
          ++e;
        });
        ends = (ends & ~(15u << (4 * t))) | (unsigned)e << (4 * t);
      }
      if (ends != want) ok = false;  // (the passes disagree: the rows are written, and are not a table)
    } else if (m) {
      ok = false;
    }
  }
  // the masks must add up to what the offsets say this row owns
  ok = ok && carry - n0 == nr;
  if (__ballot(!ok) != 0ull && lane == 0) atomicOr(p.status, 1);
}

// FS_OK, or what is wrong with the fields' geometry
int check_fields(int K, int D, int H, int W, long long vs, long long wst, bool with_aux, long long as) {
  if (K < 1 || D < 2 || H < 2 || W < 2) return FS_ERR_SHAPE;
  const long long P = (long long)D * H * W;
  if (P >= 0x7fffffffLL || vs < 3 * P || wst < 3 * P || (with_aux && as < P)) return FS_ERR_SHAPE;
  if ((long long)K * D * H > 0x7fffffffLL) return FS_ERR_SHAPE;
  return FS_OK;
}

inline long long counts_bytes(int K, int D, int H) { return (4LL * K * D * H * 4 + 15) / 16 * 16; }

inline bool min_ok(double m) { return m >= 0.0 && m < HUGE_VAL && (double)(float)m < HUGE_VAL; }

Fields make_fields(const float* v, long long vs, const float* w, long long wst, const float* aux, long long as, int K, int D,
                   int H, int W, double vmin, double wmin) {
  Fields g;
  g.v = v; g.w = w; g.aux = aux; g.vs = vs; g.wst = wst; g.as = aux ? as : 0;
  g.rows = (long long)K * D * H; g.P = (long long)D * H * W;
  g.W = W; g.H = H; g.D = D;
  const double vm = (double)(float)vmin, wm = (double)(float)wmin;
  g.vmin2 = vm * vm;
  g.wmin2 = wm * wm;
  return g;
}

}  // namespace

extern "C" long long fs_pv3d_ws_bytes(int K, int D, int H, int W) {
  const long long P = (long long)D * H * W;
  const int rc = check_fields(K, D, H, W, 3 * P, 3 * P, false, 0);
  if (rc != FS_OK) return -rc;
  return counts_bytes(K, D, H) + 5LL * K * P;
}

extern "C" int fs_pv_count3d(const float* v, long long v_sstride, const float* w, long long w_sstride, const float* aux,
                             long long aux_sstride, int K, int D, int H, int W, double vmin, double wmin, unsigned char* ws,
                             fs_stream_t stream) {
  FS_ENTER();
  FS_REQUIRE_PTR(v); FS_REQUIRE_PTR(w); FS_REQUIRE_PTR(ws);
  const int rc = check_fields(K, D, H, W, v_sstride, w_sstride, aux != nullptr, aux_sstride);
  if (rc != FS_OK) return rc;
  if (!min_ok(vmin) || !min_ok(wmin) || ((uintptr_t)ws & 15u)) return FS_ERR_ARG;
  const Fields g = make_fields(v, v_sstride, w, w_sstride, aux, aux_sstride, K, D, H, W, vmin, wmin);
  int* cnt = reinterpret_cast<int*>(ws);
  unsigned* fbits = reinterpret_cast<unsigned*>(ws + counts_bytes(K, D, H));
  unsigned char* tmask = ws + counts_bytes(K, D, H) + 4LL * K * g.P;
  const dim3 grid((unsigned)((g.rows + kRows - 1) / kRows));
  hipLaunchKernelGGL(pv_face_kernel, grid, dim3(NT), 0, (hipStream_t)stream, g, fbits, cnt + 2 * g.rows);
  FS_LAUNCH_CHECK();
  hipLaunchKernelGGL(pv_tet_kernel, grid, dim3(NT), 0, (hipStream_t)stream, g, fbits, tmask, cnt, cnt + g.rows,
                     cnt + 3 * g.rows);
  FS_LAUNCH_CHECK();
  return FS_OK;
}

extern "C" int fs_pv_emit3d(const float* v, long long v_sstride, const float* w, long long w_sstride, const float* aux,
                            long long aux_sstride, int K, int D, int H, int W, const double* inv_h, double vmin, double wmin,
                            const unsigned char* ws, const long long* row_offsets, long long N, int* cell,
                            unsigned char* simplex, unsigned char* face, long long* key, float* pos, double* mu, float* vel,
                            float* aux_out, int* status, fs_stream_t stream) {
  FS_ENTER();
  FS_REQUIRE_PTR(v); FS_REQUIRE_PTR(w); FS_REQUIRE_PTR(inv_h); FS_REQUIRE_PTR(ws); FS_REQUIRE_PTR(row_offsets);
  FS_REQUIRE_PTR(status);
  if (N > 0) {
    FS_REQUIRE_PTR(cell); FS_REQUIRE_PTR(simplex); FS_REQUIRE_PTR(face); FS_REQUIRE_PTR(key); FS_REQUIRE_PTR(pos);
    FS_REQUIRE_PTR(mu); FS_REQUIRE_PTR(vel);
    if (aux) FS_REQUIRE_PTR(aux_out);
  }
  const int rc = check_fields(K, D, H, W, v_sstride, w_sstride, aux != nullptr, aux_sstride);
  if (rc != FS_OK) return rc;
  if (!min_ok(vmin) || !min_ok(wmin) || N < 0 || ((uintptr_t)ws & 15u)) return FS_ERR_ARG;
  EP p;
  for (int a = 0; a < 3; ++a) {
    p.inv_h[a] = inv_h[a];
    if (!fs::pos_finite(p.inv_h[a])) return FS_ERR_ARG;
  }
  if (N == 0) return FS_OK;  // nothing to write: nothing launched
  p.g = make_fields(v, v_sstride, w, w_sstride, aux, aux_sstride, K, D, H, W, vmin, wmin);
  p.fbits = reinterpret_cast<const unsigned*>(ws + counts_bytes(K, D, H));
  p.tmask = ws + counts_bytes(K, D, H) + 4LL * K * p.g.P;
  p.off = row_offsets;
  p.cell = cell; p.simplex = simplex; p.face = face; p.key = key; p.pos = pos; p.mu = mu; p.vel = vel;
  p.aux = aux ? aux_out : nullptr;
  p.N = N; p.status = status;
  const dim3 grid((unsigned)((p.g.rows + kRows - 1) / kRows));
  hipLaunchKernelGGL(pv_emit_kernel, grid, dim3(NT), 0, (hipStream_t)stream, p);
  FS_LAUNCH_CHECK();
  return FS_OK;
}
