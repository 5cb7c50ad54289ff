// census3d.hip -- the census (soft ternary) distance of UPFlow/utils/loss.py:59-71 on volumes, for gfx950.
//
// The arithmetic is the 2-D kernel's (losses.hip) without the grey conversion: zero-padded (2r+1)^3 neighbourhood,
// u = v[n] - v[c], t = u / sqrt(0.81 + u^2), dist[c] = sum over the taps of (t1 - t2)^2 / (0.1 + (t1 - t2)^2).
// One workgroup of 512 threads owns a brick of 8 x 16 x 32 voxels (z, y, x); both volumes -- and grad_dist in the
// backward pass -- sit in LDS with an r-voxel halo.  A thread owns the 8 voxels of one z-column: for each of the
// (2r+1)^2 in-plane offsets it reads the column of 8 + 2r values once and uses every value for up to 2r+1 of its voxels,
// so a tap costs (8 + 2r) / (8 (2r+1)) LDS reads per volume instead of one (r = 3: 1/4), and the lanes of a wave read
// consecutive x (conflict-free ds_read_b32 without padding).  DESIGN.md "3-D census" has the brick's derivation.
// Backward: gather-formulated, no atomics; the pair symmetry of census_pair.hpp makes it one evaluation per tap.
#include "common.hpp"
#include "census_pair.hpp"

namespace {

constexpr int BX = 32, BY = 16, BZ = 8, NT = BX * BY;

template <int R>
struct Brick {
  static constexpr int P = 2 * R + 1, SX = BX + 2 * R, SY = BY + 2 * R, SZ = BZ + 2 * R, PL = SX * SY, N = PL * SZ;
};

// origin of this workgroup's brick; blockIdx.z = b * nbz + z-brick
struct Origin {
  int b, z0, y0, x0;
};
__device__ __forceinline__ Origin brick_origin(int nbz) {
  Origin o;
  o.b = blockIdx.z / nbz;
  o.z0 = (blockIdx.z - o.b * nbz) * BZ;
  o.y0 = blockIdx.y * BY;
  o.x0 = blockIdx.x * BX;
  return o;
}

// global offset of halo element i of the brick, or -1 outside the volume (zero padding, loss.py:64)
template <int R>
__device__ __forceinline__ long long halo_offset(int i, const Origin& o, int D, int H, int W) {
  using K = Brick<R>;
  const int z = i / K::PL, rem = i - z * K::PL, y = rem / K::SX, x = rem - y * K::SX;
  const int gz = o.z0 + z - R, gy = o.y0 + y - R, gx = o.x0 + x - R;
  if (gz < 0 || gz >= D || gy < 0 || gy >= H || gx < 0 || gx >= W) return -1;
  return ((long long)gz * H + gy) * W + gx;
}

template <int R>
__global__ __launch_bounds__(NT) void census3d_fwd_kernel(const float* __restrict__ vol1,
                                                          const float* __restrict__ vol2,
                                                          float* __restrict__ dist, int D, int H, int W, int nbz) {
  using K = Brick<R>;
  __shared__ float s1[K::N], s2[K::N];
  const Origin o = brick_origin(nbz);
  const long long DHW = (long long)D * H * W;
  const float* v1 = vol1 + o.b * DHW;
  const float* v2 = vol2 + o.b * DHW;
  for (int i = threadIdx.x; i < K::N; i += NT) {
    const long long g = halo_offset<R>(i, o, D, H, W);
    s1[i] = g >= 0 ? v1[g] : 0.f;
    s2[i] = g >= 0 ? v2[g] : 0.f;
  }
  __syncthreads();
  const int tx = threadIdx.x % BX, ty = threadIdx.x / BX;
  const int y = o.y0 + ty, x = o.x0 + tx;
  if (y >= H || x >= W) return;
  float c1[BZ], c2[BZ], acc[BZ];
  const int ctr = (R * K::SY + ty + R) * K::SX + tx + R;
#pragma unroll
  for (int j = 0; j < BZ; ++j) {
    c1[j] = s1[ctr + j * K::PL];
    c2[j] = s2[ctr + j * K::PL];
    acc[j] = 0.f;
  }
#pragma unroll 1
  for (int t = 0; t < K::P * K::P; ++t) {
    const int dy = t / K::P, dx = t - dy * K::P;
    const int col = (ty + dy) * K::SX + tx + dx;
    float a1[K::SZ], a2[K::SZ];
#pragma unroll
    for (int k = 0; k < K::SZ; ++k) {
      a1[k] = s1[col + k * K::PL];
      a2[k] = s2[col + k * K::PL];
    }
#pragma unroll
    for (int j = 0; j < BZ; ++j) {
      // The 2r+1 taps of the column are summed first and reach the voxel's sum in one addition: a partial sum is rounded
      // (2r+1)^2 + 2r times, not (2r+1)^3 times.  Near a border most taps are the same padding term, and adding it 300
      // times to one running sum rounds the same way each time (up to 342 * 2^-24 = 2e-5 of the value at r = 3).
      float part = 0.f;
#pragma unroll
      for (int dz = 0; dz < K::P; ++dz) {
        const float u1 = a1[j + dz] - c1[j], u2 = a2[j + dz] - c2[j];
        // v_rsq / v_rcp (1 ulp) as in the 2-D kernel: the kernel is VALU-bound from r = 2 on
        const float e = census_ternary_diff(u1, census_rnorm(u1), u2, census_rnorm(u2));
        const float d = e * e;
        const float term = d * __builtin_amdgcn_rcpf(0.1f + d);
        part = dz == 0 ? term : part + term;
      }
      acc[j] += part;
    }
  }
  float* out = dist + o.b * DHW + ((long long)o.z0 * H + y) * W + x;
#pragma unroll
  for (int j = 0; j < BZ; ++j)
    if (o.z0 + j < D) out[(long long)j * H * W] = acc[j];
}

template <int R>
__global__ __launch_bounds__(NT) void census3d_bwd_kernel(const float* __restrict__ vol1,
                                                          const float* __restrict__ vol2,
                                                          const float* __restrict__ gdist,
                                                          float* __restrict__ gvol1, float* __restrict__ gvol2,
                                                          int D, int H, int W, int nbz) {
  using K = Brick<R>;
  __shared__ float s1[K::N], s2[K::N], sk[K::N];
  const Origin o = brick_origin(nbz);
  const long long DHW = (long long)D * H * W;
  const float* v1 = vol1 + o.b * DHW;
  const float* v2 = vol2 + o.b * DHW;
  const float* gd = gdist + o.b * DHW;
  for (int i = threadIdx.x; i < K::N; i += NT) {
    const long long g = halo_offset<R>(i, o, D, H, W);
    s1[i] = g >= 0 ? v1[g] : 0.f;
    s2[i] = g >= 0 ? v2[g] : 0.f;
    sk[i] = g >= 0 ? gd[g] : 0.f;  // k = 0 outside: such centres do not exist
  }
  __syncthreads();
  const int tx = threadIdx.x % BX, ty = threadIdx.x / BX;
  const int y = o.y0 + ty, x = o.x0 + tx;
  if (y >= H || x >= W) return;
  float c1[BZ], c2[BZ], ck[BZ], g1[BZ], g2[BZ];
  const int ctr = (R * K::SY + ty + R) * K::SX + tx + R;
#pragma unroll
  for (int j = 0; j < BZ; ++j) {
    c1[j] = s1[ctr + j * K::PL];
    c2[j] = s2[ctr + j * K::PL];
    ck[j] = sk[ctr + j * K::PL];
    g1[j] = g2[j] = 0.f;
  }
#pragma unroll 1
  for (int t = 0; t < K::P * K::P; ++t) {
    const int dy = t / K::P, dx = t - dy * K::P;
    const int col = (ty + dy) * K::SX + tx + dx;
    float a1[K::SZ], a2[K::SZ], ak[K::SZ];
#pragma unroll
    for (int k = 0; k < K::SZ; ++k) {
      a1[k] = s1[col + k * K::PL];
      a2[k] = s2[col + k * K::PL];
      ak[k] = sk[col + k * K::PL];
    }
#pragma unroll
    for (int j = 0; j < BZ; ++j)
#pragma unroll
      for (int dz = 0; dz < K::P; ++dz)
        // the pair (q, q + delta): q as the centre (zero-padded volume outside) and as the neighbour of the centre
        // q + delta (k = 0 where no such centre exists)
        census_pair_grad(a1[j + dz] - c1[j], a2[j + dz] - c2[j], ck[j] + ak[j + dz], g1[j], g2[j]);
  }
  const long long at = o.b * DHW + ((long long)o.z0 * H + y) * W + x;
#pragma unroll
  for (int j = 0; j < BZ; ++j)
    if (o.z0 + j < D) {
      if (gvol1) gvol1[at + (long long)j * H * W] = g1[j];
      if (gvol2) gvol2[at + (long long)j * H * W] = g2[j];
    }
}

int census3d_grid(int B, int D, int H, int W, int radius, dim3& grid, int& nbz) {
  if (B < 1 || D < 1 || H < 1 || W < 1) return FS_ERR_SHAPE;
  if (radius < 1 || radius > 3) return FS_ERR_ARG;
  nbz = fs::cdiv(D, BZ);
  if ((long long)B * nbz > 65535 || fs::cdiv(H, BY) > 65535) return FS_ERR_SHAPE;
  grid = dim3(fs::cdiv(W, BX), fs::cdiv(H, BY), B * nbz);
  return FS_OK;
}

}  // namespace

extern "C" int fs_census3d_dist_fwd(const float* vol1, const float* vol2, float* dist, int B, int D, int H,
                                    int W, int radius, fs_stream_t stream) {
  FS_ENTER();
  FS_REQUIRE_PTR(vol1); FS_REQUIRE_PTR(vol2); FS_REQUIRE_PTR(dist);
  dim3 grid;
  int nbz;
  const int rc = census3d_grid(B, D, H, W, radius, grid, nbz);
  if (rc != FS_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (radius == 1)
    hipLaunchKernelGGL(census3d_fwd_kernel<1>, grid, dim3(NT), 0, st, vol1, vol2, dist, D, H, W, nbz);
  else if (radius == 2)
    hipLaunchKernelGGL(census3d_fwd_kernel<2>, grid, dim3(NT), 0, st, vol1, vol2, dist, D, H, W, nbz);
  else
    hipLaunchKernelGGL(census3d_fwd_kernel<3>, grid, dim3(NT), 0, st, vol1, vol2, dist, D, H, W, nbz);
  FS_LAUNCH_CHECK();
  return FS_OK;
}

extern "C" int fs_census3d_dist_bwd(const float* vol1, const float* vol2, const float* grad_dist,
                                    float* grad_vol1, float* grad_vol2, int B, int D, int H, int W, int radius,
                                    fs_stream_t stream) {
  FS_ENTER();
  FS_REQUIRE_PTR(vol1); FS_REQUIRE_PTR(vol2); FS_REQUIRE_PTR(grad_dist);
  if (grad_vol1 == nullptr && grad_vol2 == nullptr) return FS_ERR_NULLPTR;
  dim3 grid;
  int nbz;
  const int rc = census3d_grid(B, D, H, W, radius, grid, nbz);
  if (rc != FS_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (radius == 1)
    hipLaunchKernelGGL(census3d_bwd_kernel<1>, grid, dim3(NT), 0, st, vol1, vol2, grad_dist, grad_vol1, grad_vol2,
                       D, H, W, nbz);
  else if (radius == 2)
    hipLaunchKernelGGL(census3d_bwd_kernel<2>, grid, dim3(NT), 0, st, vol1, vol2, grad_dist, grad_vol1, grad_vol2,
                       D, H, W, nbz);
  else
    hipLaunchKernelGGL(census3d_bwd_kernel<3>, grid, dim3(NT), 0, st, vol1, vol2, grad_dist, grad_vol1, grad_vol2,
                       D, H, W, nbz);
  FS_LAUNCH_CHECK();
  return FS_OK;
}
