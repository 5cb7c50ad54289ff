// advect.hip -- pathlines: P particles moved through K consecutive displacement fields in one launch
// (fs_advect2d / fs_advect3d).  Field k is the displacement of one time step on that step's grid, so a particle at p
// moves to p + scale * F_k(p) (Euler), or by the RK2 / RK4 update of the same steady field, in `substeps` equal parts.
//
// Per particle (fp64, contraction off: a numpy fp64 restatement with the same operations in the same order reproduces
// every position bit, every status and every count -- tests/advect_ref.py):
//   sample(k, q) and classify(p): the rule trilinear64.hpp states (a non-finite q samples NaN with no index formed, any
//     other q is clamped to the grid; p is NONFINITE, OUT (border inclusive) or ALIVE).  They are their OWN copy of
//     those lines and do not include the header: on it the 3-D Euler kernel measured 0.9 % slower on 10^4 scattered
//     seeds in three sessions, outside the parent's spread (profiles/trilinear64.txt) -- a change to the rule is made
//     there and here
//   step k: the fp32 position (pos_in, later the previous step's result) is widened; an ALIVE particle is classified
//     (a seed outside the box or a NaN seed ends here without moving); while ALIVE, each substep forms p' (stage points
//     are clamped by sample, never classified) and classifies it: NONFINITE keeps p, OUT and ALIVE take p'; `steps`
//     counts the steps a particle is still ALIVE after; the position is rounded to fp32 once per step and stored in
//     slot k, and the next step starts from the rounded value: K steps in one launch == K launches of one step.
//     A particle that is not ALIVE copies its position to every remaining slot.
//
// One thread per particle, component-major positions (a wave's loads and stores are contiguous), plain global gathers
// for the 2^C x C corner reads per stage: grid seeds are neighbours in the field, so a wave's corners share cache
// lines as they do in flowconsist.hip.  A thread touches only its own particle's pos_in / traj / status / steps
// elements and reads pos_in before it stores anything: traj's last slot may be pos_in's memory.
#include "common.hpp"

namespace {

constexpr int NT = 256;

struct AP {
  long long P;         // particles
  long long fss;       // step stride of flows (elements)
  long long plane;     // D*H*W
  long long pcs;       // component stride of pos_in
  long long tss, tcs;  // step and component strides of traj (tss = 0: every step overwrites the one slot)
  int K, S;            // steps, substeps
  int D, H, W;
  double hs, hh, h6;  // scale / S, 0.5 hs, hs / 6: formed on the host, the device divides nothing
};

template <int C>
__device__ __forceinline__ int classify(const double (&p)[3], const AP& a) {
  const int S[3] = {a.W, a.H, a.D};
  bool fin = true, out = false;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    fin = fin && isfinite(p[c]);
    out = out || p[c] < 0.0 || p[c] > (double)(S[c] - 1);
  }
  return !fin ? FS_ADV_NONFINITE : out ? FS_ADV_OUT : FS_ADV_ALIVE;
}

// v = field fk sampled at q.  Every index comes from a finite value clamped to [0, S_c - 1].
template <int C>
__device__ __forceinline__ void sample(const float* __restrict__ fk, const AP& a, const double (&q)[3],
                                       double (&v)[3]) {
#pragma clang fp contract(off)
  bool fin = true;
#pragma unroll
  for (int c = 0; c < C; ++c) fin = fin && isfinite(q[c]);
  if (!fin) {
#pragma unroll
    for (int c = 0; c < C; ++c) v[c] = __builtin_nan("");
    return;
  }
  const int S[3] = {a.W, a.H, a.D};
  const size_t st[3] = {(size_t)1, (size_t)a.W, (size_t)a.W * (size_t)a.H};
  double fr[3], gr[3];
  size_t o0[3], o1[3];
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const double hi = (double)(S[c] - 1);
    double qc = q[c] < 0.0 ? 0.0 : q[c];
    qc = qc > hi ? hi : qc;
    const double fl = floor(qc);
    const int i0 = (int)fl;
    const int i1 = i0 + 1 < S[c] ? i0 + 1 : S[c] - 1;
    fr[c] = qc - fl;
    gr[c] = 1.0 - fr[c];
    o0[c] = (size_t)i0 * st[c];
    o1[c] = (size_t)i1 * st[c];
  }
  double s[3] = {0.0, 0.0, 0.0};
#pragma unroll
  for (int k = 0; k < (1 << C); ++k) {
    const int bx = k & 1, by = (k >> 1) & 1, bz = (k >> 2) & 1;
    double wt;
    size_t o;
    if (C == 3) {
      wt = ((bz ? fr[2] : gr[2]) * (by ? fr[1] : gr[1])) * (bx ? fr[0] : gr[0]);
      o = (bz ? o1[2] : o0[2]) + (by ? o1[1] : o0[1]) + (bx ? o1[0] : o0[0]);
    } else {
      wt = (by ? fr[1] : gr[1]) * (bx ? fr[0] : gr[0]);
      o = (by ? o1[1] : o0[1]) + (bx ? o1[0] : o0[0]);
    }
#pragma unroll
    for (int c = 0; c < C; ++c) s[c] = s[c] + wt * (double)fk[(size_t)c * a.plane + o];
  }
#pragma unroll
  for (int c = 0; c < C; ++c) v[c] = s[c];
}

// q = p + h * v
template <int C>
__device__ __forceinline__ void axpy(const double (&p)[3], double h, const double (&v)[3], double (&q)[3]) {
#pragma clang fp contract(off)
#pragma unroll
  for (int c = 0; c < C; ++c) q[c] = p[c] + h * v[c];
}

// pos_in and traj carry no __restrict__: traj's last slot may be pos_in
template <int C, int M>
__global__ __launch_bounds__(NT) void advect_kernel(const float* __restrict__ flows, const float* pos_in, float* traj,
                                                    unsigned char* __restrict__ status, int* __restrict__ steps,
                                                    AP a) {
#pragma clang fp contract(off)
  const long long i = (long long)blockIdx.x * NT + threadIdx.x;
  if (i >= a.P) return;
  float pf[3] = {0.f, 0.f, 0.f};
#pragma unroll
  for (int c = 0; c < C; ++c) pf[c] = pos_in[(size_t)c * a.pcs + i];
  int st = status[i];
  int n = steps ? steps[i] : 0;
  for (int k = 0; k < a.K; ++k) {
    if (st == FS_ADV_ALIVE) {
      double p[3] = {0.0, 0.0, 0.0};
#pragma unroll
      for (int c = 0; c < C; ++c) p[c] = (double)pf[c];
      st = classify<C>(p, a);
      if (st == FS_ADV_ALIVE) {
        const float* fk = flows + (size_t)k * a.fss;
        for (int s = 0; s < a.S && st == FS_ADV_ALIVE; ++s) {
          double k1[3], pn[3] = {0.0, 0.0, 0.0};
          sample<C>(fk, a, p, k1);
          if (M == FS_ADV_EULER) {
            axpy<C>(p, a.hs, k1, pn);
          } else if (M == FS_ADV_RK2) {
            double q[3], k2[3];
            axpy<C>(p, a.hh, k1, q);
            sample<C>(fk, a, q, k2);
            axpy<C>(p, a.hs, k2, pn);
          } else {
            double q[3], k2[3], k3[3], k4[3], sm[3];
            axpy<C>(p, a.hh, k1, q);
            sample<C>(fk, a, q, k2);
            axpy<C>(p, a.hh, k2, q);
            sample<C>(fk, a, q, k3);
            axpy<C>(p, a.hs, k3, q);
            sample<C>(fk, a, q, k4);
#pragma unroll
            for (int c = 0; c < C; ++c) sm[c] = ((k1[c] + 2.0 * k2[c]) + 2.0 * k3[c]) + k4[c];
            axpy<C>(p, a.h6, sm, pn);
          }
          st = classify<C>(pn, a);
          if (st != FS_ADV_NONFINITE) {
#pragma unroll
            for (int c = 0; c < C; ++c) p[c] = pn[c];
          }
        }
        if (st == FS_ADV_ALIVE) n += 1;
#pragma unroll
        for (int c = 0; c < C; ++c) pf[c] = (float)p[c];
      }
    }
#pragma unroll
    for (int c = 0; c < C; ++c) traj[(size_t)k * a.tss + (size_t)c * a.tcs + i] = pf[c];
  }
  status[i] = (unsigned char)st;
  if (steps) steps[i] = n;
}

int launch(bool is3d, const float* flows, int K, int C, int D, int H, int W, long long fss, const float* pos_in,
           long long pcs, long long P, float* traj, long long tss, long long tcs, unsigned char* status, int* steps,
           int method, int substeps, double scale, fs_stream_t stream) {
  FS_ENTER();
  FS_REQUIRE_PTR(flows); FS_REQUIRE_PTR(pos_in); FS_REQUIRE_PTR(traj); FS_REQUIRE_PTR(status);
  if (K < 1 || P < 1 || C != (is3d ? 3 : 2) || D < 1 || H < 1 || W < 1) return FS_ERR_SHAPE;
  const long long plane = (long long)D * H * W;
  if (plane > (1LL << 40) / C) return FS_ERR_SHAPE;
  if (K > 1 && (fss < C * plane || (tss != 0 && tss < P))) return FS_ERR_SHAPE;
  if (pcs < P || tcs < P) return FS_ERR_SHAPE;
  const long long blocks = (P + NT - 1) / NT;
  if (blocks > 0x7fffffffLL) return FS_ERR_SHAPE;
  if (substeps < 1 || !(scale > -HUGE_VAL && scale < HUGE_VAL)) return FS_ERR_ARG;
  if (method != FS_ADV_EULER && method != FS_ADV_RK2 && method != FS_ADV_RK4) return FS_ERR_ARG;
  AP a;
  a.P = P; a.fss = fss; a.plane = plane; a.pcs = pcs; a.tss = tss; a.tcs = tcs;
  a.K = K; a.S = substeps; a.D = D; a.H = H; a.W = W;
  a.hs = scale / (double)substeps;
  a.hh = 0.5 * a.hs;
  a.h6 = a.hs / 6.0;
  const hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)blocks), blk(NT);
#define FS_ADV_LAUNCH(CC, MM) \
  hipLaunchKernelGGL((advect_kernel<CC, MM>), grid, blk, 0, s, flows, pos_in, traj, status, steps, a)
#define FS_ADV_LAUNCH_C(CC)                                           \
  do {                                                                \
    if (method == FS_ADV_EULER) FS_ADV_LAUNCH(CC, FS_ADV_EULER);      \
    else if (method == FS_ADV_RK2) FS_ADV_LAUNCH(CC, FS_ADV_RK2);     \
    else FS_ADV_LAUNCH(CC, FS_ADV_RK4);                               \
  } while (0)
  if (is3d) FS_ADV_LAUNCH_C(3); else FS_ADV_LAUNCH_C(2);
#undef FS_ADV_LAUNCH_C
#undef FS_ADV_LAUNCH
  FS_LAUNCH_CHECK();
  return FS_OK;
}

}  // namespace

extern "C" int fs_advect2d(const float* flows, int K, int C, int H, int W, long long flow_sstride, const float* pos_in,
                           long long pos_cstride, long long P, float* traj, long long traj_sstride,
                           long long traj_cstride, unsigned char* status, int* steps, int method, int substeps,
                           double scale, fs_stream_t stream) {
  return launch(false, flows, K, C, 1, H, W, flow_sstride, pos_in, pos_cstride, P, traj, traj_sstride, traj_cstride,
                status, steps, method, substeps, scale, stream);
}

extern "C" int fs_advect3d(const float* flows, int K, int C, int D, int H, int W, long long flow_sstride,
                           const float* pos_in, long long pos_cstride, long long P, float* traj,
                           long long traj_sstride, long long traj_cstride, unsigned char* status, int* steps,
                           int method, int substeps, double scale, fs_stream_t stream) {
  return launch(true, flows, K, C, D, H, W, flow_sstride, pos_in, pos_cstride, P, traj, traj_sstride, traj_cstride,
                status, steps, method, substeps, scale, stream);
}
