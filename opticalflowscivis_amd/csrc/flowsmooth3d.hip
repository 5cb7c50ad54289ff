// flowsmooth3d.hip -- first-order flow smoothness on volumes for gfx950: the term the reference's Flow-3D update
// holds commented out (Flow-3D/model/RIFE.py:147-167), with differences taken only between voxels that both exist and
// the optional edge-aware weight of UPFlow's smoothness term.
//   S1 = sum over b, c, voxel p, axis a in {D,H,W} with p + e_a inside of
//        w_a(p) * ((flow[b,c,p+e_a] - flow[b,c,p])^2 + eps^2)^q,   w_a(p) = exp(-kappa |guide[b,0,p+e_a] - guide[b,0,p]|)
// One thread owns one voxel and walks its C channels (the three weights are formed once per voxel); the forward and the
// diagonal neighbours come out of the caches, so each way is one pass over the flow.  Reduction as fs_robust_sum:
// per-workgroup partials, fixed-order finish in fp64, no float atomics.
#include <float.h>
#include "common.hpp"

namespace {

struct SMP {
  long long nv;   // B*D*H*W voxels
  long long DHW;
  int C, D, H, W;
  float q, eps2, kappa;
};

// (d^2 + eps^2)^q through v_log / v_exp: d^2 + eps^2 >= eps^2 is a normal number (checked on the host side of the
// entry points), so the hardware forms need no range handling
__device__ __forceinline__ float pen(float d, float q, float eps2) {
  return __builtin_amdgcn_exp2f(q * __builtin_amdgcn_logf(d * d + eps2));
}
// d/dd (d^2 + eps^2)^q = 2 q d (d^2 + eps^2)^(q-1)
__device__ __forceinline__ float dpen(float d, float q, float eps2) {
  return 2.f * q * d * __builtin_amdgcn_exp2f((q - 1.f) * __builtin_amdgcn_logf(d * d + eps2));
}

__device__ __forceinline__ float edge_w(const float* __restrict__ g, long long a, long long b, float kappa) {
  return expf(-kappa * fabsf(g[b] - g[a]));
}

__device__ __forceinline__ void voxel_of(long long v, const SMP& p, long long& b, int& z, int& y, int& x) {
  b = v / p.DHW;
  long long r = v - b * p.DHW;
  const int HW = p.H * p.W;
  z = (int)(r / HW);
  const int r2 = (int)(r - (long long)z * HW);
  y = r2 / p.W;
  x = r2 - y * p.W;
}

__global__ __launch_bounds__(256) void flow_smooth3d_fwd_kernel(const float* __restrict__ flow,
                                                                const float* __restrict__ guide,
                                                                float* __restrict__ ws, SMP p) {
  float s1 = 0.f, s2 = 0.f;
  const long long sW = 1, sH = p.W, sD = (long long)p.H * p.W;
  for (long long v = (long long)blockIdx.x * 256 + threadIdx.x; v < p.nv; v += (long long)gridDim.x * 256) {
    long long b;
    int z, y, x;
    voxel_of(v, p, b, z, y, x);
    const bool hz = z + 1 < p.D, hy = y + 1 < p.H, hx = x + 1 < p.W;
    float wz = 1.f, wy = 1.f, wx = 1.f;
    if (guide) {
      if (hz) wz = edge_w(guide, v, v + sD, p.kappa);
      if (hy) wy = edge_w(guide, v, v + sH, p.kappa);
      if (hx) wx = edge_w(guide, v, v + sW, p.kappa);
    }
    const float* f = flow + b * p.C * p.DHW + (v - b * p.DHW);
    for (int c = 0; c < p.C; ++c, f += p.DHW) {
      const float f0 = f[0];
      if (hz) s1 += wz * pen(f[sD] - f0, p.q, p.eps2);
      if (hy) s1 += wy * pen(f[sH] - f0, p.q, p.eps2);
      if (hx) s1 += wx * pen(f[sW] - f0, p.q, p.eps2);
    }
    s2 += (float)(p.C * ((int)hz + (int)hy + (int)hx));  // pairs counted: exact per workgroup, summed in fp64
  }
  fs::block_pair_to_ws(s1, s2, ws);
}

__global__ __launch_bounds__(256) void flow_smooth3d_bwd_kernel(const float* __restrict__ flow,
                                                                const float* __restrict__ guide,
                                                                const float* __restrict__ coef,
                                                                float* __restrict__ gflow, SMP p) {
  const float k = coef[0];
  const long long sW = 1, sH = p.W, sD = (long long)p.H * p.W;
  for (long long v = (long long)blockIdx.x * 256 + threadIdx.x; v < p.nv; v += (long long)gridDim.x * 256) {
    long long b;
    int z, y, x;
    voxel_of(v, p, b, z, y, x);
    // the up to six differences this voxel is part of: towards p + e_a (weight w_a(p)) and from p - e_a (w_a(p - e_a))
    const bool hz = z + 1 < p.D, hy = y + 1 < p.H, hx = x + 1 < p.W, lz = z > 0, ly = y > 0, lx = x > 0;
    float wzp = 1.f, wyp = 1.f, wxp = 1.f, wzm = 1.f, wym = 1.f, wxm = 1.f;
    if (guide) {
      if (hz) wzp = edge_w(guide, v, v + sD, p.kappa);
      if (hy) wyp = edge_w(guide, v, v + sH, p.kappa);
      if (hx) wxp = edge_w(guide, v, v + sW, p.kappa);
      if (lz) wzm = edge_w(guide, v - sD, v, p.kappa);
      if (ly) wym = edge_w(guide, v - sH, v, p.kappa);
      if (lx) wxm = edge_w(guide, v - sW, v, p.kappa);
    }
    const long long at = b * p.C * p.DHW + (v - b * p.DHW);
    const float* f = flow + at;
    float* g = gflow + at;
    for (int c = 0; c < p.C; ++c, f += p.DHW, g += p.DHW) {
      const float f0 = f[0];
      float a = 0.f;
      if (hz) a -= wzp * dpen(f[sD] - f0, p.q, p.eps2);
      if (lz) a += wzm * dpen(f0 - f[-sD], p.q, p.eps2);
      if (hy) a -= wyp * dpen(f[sH] - f0, p.q, p.eps2);
      if (ly) a += wym * dpen(f0 - f[-sH], p.q, p.eps2);
      if (hx) a -= wxp * dpen(f[sW] - f0, p.q, p.eps2);
      if (lx) a += wxm * dpen(f0 - f[-sW], p.q, p.eps2);
      g[0] = k * a;
    }
  }
}

int make_smp(SMP& p, int B, int C, int D, int H, int W, float q, float eps, float kappa) {
  if (B < 1 || C < 1 || D < 1 || H < 1 || W < 1 || (long long)H * W > 0x7fffffffLL) return FS_ERR_SHAPE;
  const float eps2 = eps * eps;
  // eps^2 must be a normal fp32 number (eps = 0 would make the gradient of a zero difference 0 * inf); q > 0; the
  // weight is a decay
  if (!(eps2 >= FLT_MIN) || !(eps2 <= FLT_MAX) || !(q > 0.f) || !(q <= FLT_MAX) || !(kappa >= 0.f) || !(kappa <= FLT_MAX))
    return FS_ERR_ARG;
  p.DHW = (long long)D * H * W;
  p.nv = (long long)B * p.DHW;
  p.C = C; p.D = D; p.H = H; p.W = W;
  p.q = q; p.eps2 = eps2; p.kappa = kappa;
  return FS_OK;
}

}  // namespace

extern "C" int fs_flow_smooth3d_fwd(const float* flow, const float* guide, float* sums, float* ws, int B, int C,
                                    int D, int H, int W, float q, float eps, float kappa, fs_stream_t stream) {
  FS_ENTER();
  FS_REQUIRE_PTR(flow); FS_REQUIRE_PTR(sums); FS_REQUIRE_PTR(ws);
  SMP p;
  const int rc = make_smp(p, B, C, D, H, W, q, eps, kappa);
  if (rc != FS_OK) return rc;
  if (kappa == 0.f) guide = nullptr;  // w = 1
  const long long want = (p.nv + 255) / 256;
  const int nb = (int)(want < FS_REDUCE_BLOCKS ? want : FS_REDUCE_BLOCKS);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(flow_smooth3d_fwd_kernel, dim3(nb), dim3(256), 0, st, flow, guide, ws, p);
  hipLaunchKernelGGL(fs::reduce_final_kernel, dim3(1), dim3(256), 0, st, ws, nb, sums);
  FS_LAUNCH_CHECK();
  return FS_OK;
}

extern "C" int fs_flow_smooth3d_bwd(const float* flow, const float* guide, const float* coef, float* grad_flow,
                                    int B, int C, int D, int H, int W, float q, float eps, float kappa,
                                    fs_stream_t stream) {
  FS_ENTER();
  FS_REQUIRE_PTR(flow); FS_REQUIRE_PTR(coef); FS_REQUIRE_PTR(grad_flow);
  SMP p;
  const int rc = make_smp(p, B, C, D, H, W, q, eps, kappa);
  if (rc != FS_OK) return rc;
  if (kappa == 0.f) guide = nullptr;
  const long long want = (p.nv + 255) / 256;
  const int nb = (int)(want < 16384 ? want : 16384);
  hipLaunchKernelGGL(flow_smooth3d_bwd_kernel, dim3(nb), dim3(256), 0, (hipStream_t)stream, flow, guide, coef,
                     grad_flow, p);
  FS_LAUNCH_CHECK();
  return FS_OK;
}
