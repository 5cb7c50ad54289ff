/*
 * flowsci_hip.h -- C-ABI of libflowsci_hip.so: the MI355X (gfx950) hot path of
 * HamidGadirov/OpticalFlowSciVis (backward warps, local-window correlation,
 * photometric / census losses), as hand-written HIP kernels.
 *
 * Conventions (every entry point):
 *   - plain pointers to DEVICE memory, fp32, contiguous NCHW / NCDHW; sizes as int;
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream);
 *   - returns FS_OK (0) or an FS_ERR_* code; never throws, never allocates,
 *     never synchronises; the caller owns all memory;
 *   - stateless and re-entrant (the reference's module-level grid cache,
 *     Flow-2D/model/warplayer.py:5, has no equivalent: grids are computed in-kernel).
 *
 * Each declaration cites the reference interface it replaces (paths relative to the
 * reference tree).  The Python binding a maintainer would add is in INTEGRATION.md.
 */
#ifndef FLOWSCI_HIP_H
#define FLOWSCI_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

typedef void* fs_stream_t; /* hipStream_t */

enum {
  FS_OK = 0,
  FS_ERR_NULLPTR = 1, /* a required pointer is NULL */
  FS_ERR_SHAPE = 2,   /* a size is out of the supported range */
  FS_ERR_ARG = 3,     /* an option / mode value is invalid */
  FS_ERR_LAUNCH = 4,  /* hipGetLastError() != hipSuccess after the launch */
  FS_ERR_UNSUPPORTED = 5 /* a fused entry point has no kernel for this shape / alignment: use the unfused ones */
};

/* ABI version of this header (major*10000 + minor*100 + patch).  ANY change to the argument list of an existing
 * entry point bumps it, and a binding must refuse a library whose fs_version() differs from the header it was
 * written against -- a stale .so would otherwise run with shifted arguments instead of failing.
 *   100  round 1.
 *   300  round 2 inserted `const int* in_hw` into fs_warp2d_{fwd,bwd} and fs_warp2d_pair_{fwd,bwd} (without bumping
 *        the number: fixed in round 3) and added the f1-f4 / conv3d entry points.
 *   310  round 3: fs_conv3d_fwd* / fs_conv3d_tr* accept w = NULL ("ws is prepared"), fs_conv3d_*_wprep_jobs,
 *        fs_conv3d_wprep_batch.
 *   320  round 4: fs_conv3d_wrw_kernel_id (which weight-gradient kernel a call dispatches to; nothing launched);
 *        fs_conv3d_wrw_det / fs_conv3d_wrw_det_ws_floats (workspace form without float atomics).
 *        The library reads no environment variable any more (measurement switches live in the -DFS_ABLATION build).
 *   330  round 5: fs_warp3d_kernel_id (which kernel a trilinear-warp call dispatches to; nothing launched).
 *   340  fs_frame_metrics2d / fs_frame_metrics3d and their _ws_bytes queries (sequence evaluation: PSNR / SSIM).
 *   350  fs_flow_metrics2d / fs_flow_metrics3d and their _ws_bytes queries (flow accuracy: EPE, Fl, angular error).
 *   360  fs_triplet_gather, fs_series_stats / fs_series_stats_ws_bytes (training batches from a device-resident series).
 *   370  fs_census3d_dist_{fwd,bwd}, fs_flow_smooth3d_{fwd,bwd} (unsupervised flow-side loss terms of Flow-3D).
 *   380  fs_flow_consistency2d / fs_flow_consistency3d and their _ws_bytes queries (label-free flow quality:
 *        forward-backward residual, occlusion / outgoing / consistent classes, photometric error of the warp).
 *   390  fs_series_encode / fs_series_encode_ws_bytes (padded fp32 planes back to a stored type: the inverse of the
 *        gather's decode, for writing rebuilt series and flows).
 *   400  fs_advect2d / fs_advect3d (pathlines: particles advected through consecutive displacement fields).
 *   410  fs_ftle2d / fs_ftle3d and their _ws_bytes queries (finite-time Lyapunov exponents of a lattice flow map).
 *   420  fs_velgrad2d / fs_velgrad3d and their _ws_bytes queries (divergence, vorticity, Q and lambda2 of step flows).
 *   430  fs_label_regions2d / fs_label_regions3d and their _ws_bytes queries, fs_region_stats2d / fs_region_stats3d,
 *        fs_region_follow2d / fs_region_follow3d (connected regions of flag maps, their table, where the flow carries them).
 *   440  fs_raycast3d / fs_raycast3d_ws_bytes, fs_brick_range3d (volumes to images: emission / absorption and maximum
 *        intensity through a transfer function, with per-brick value ranges to jump over empty space).
 *   450  fs_iso_count3d / fs_iso_emit3d / fs_iso3d_ws_bytes (volumes to indexed triangle meshes: marching tetrahedra).
 *   460  fs_lic2d / fs_lic3d and their _ws_bytes queries (line integral convolution: a texture averaged along the
 *        streamlines of step flows).
 *   470  fs_critical_count{2,3}d / fs_critical_emit{2,3}d and their _ws_bytes queries (critical points of step flows:
 *        where the piecewise-linear field vanishes, with its Jacobian, invariants and class).
 *   480  fs_streamlines2d / fs_streamlines3d (streamlines of step flows as geometry: every vertex kept, lines ended by
 *        the border, stagnation, a capturing cell or their length -- what separatrices are traced with).
 *   490  fs_pv_count3d / fs_pv_emit3d / fs_pv3d_ws_bytes (parallel vectors: the segments of the locus v || w on the Kuhn
 *        split -- vortex core lines after Sujudi-Haimes (w = J v) and Levy et al. (w = vorticity)).
 *        Added without a new number (no existing argument list changed): fs_ridge_nodes3d / fs_ridge_count3d /
 *        fs_ridge_emit3d / fs_ridge3d_ws_bytes (height-ridge surfaces of scalar volumes: Marching Ridges on the Kuhn
 *        split).  A binding that needs them fails on a library without them when it resolves the symbols. */
#define FS_ABI_VERSION 490
int fs_version(void);
/* Static string for an FS_* code. */
const char* fs_error_string(int code);

/* ------------------------------------------------------------------------------------
 * a2. Flow-3D trilinear backward warp -- Flow-3D/model/warplayer.py:9-41 `warp`.
 *   in   [B,C,D,H,W], flow [B,3,D,H,W] -> out [B,C,D,H,W].
 *   grid = (linspace(H) , linspace(D), linspace(W)) + flow/((dim-1)/2)   (:15-26)
 *   5-D grid_sample(bilinear, border, align_corners=True)               (:36)
 *   i.e. the axis-rotating sampling  out[d,h,w] = in[(w+F2)(D-1)/(W-1), (d+F1)(H-1)/(D-1),
 *   (h+F0)(W-1)/(H-1)]  with border clamp.  D,H,W >= 2.
 *   D,H,W are the extent of the FLOW (= of the output).  The reference builds its grid from
 *   the flow's shape and its divisors from the input's (:11-26), so the sampled volume may
 *   have a different extent: `in_dhw` = {Din,Hin,Win} (HOST pointer to 3 ints) or NULL when
 *   the input has the flow's extent.  (IFNet-3D hits this for sizes that are not multiples
 *   of 16: Flow-3D/model/IFNet.py:151-191.)
 * bwd: grad_in (nullable; must be zero-filled by the caller, accumulated with float
 *   atomics) and grad_flow (nullable; fully overwritten).
 */
int fs_warp3d_fwd(const float* in, const float* flow, float* out,
                  int B, int C, const int* in_dhw, int D, int H, int W, fs_stream_t stream);
int fs_warp3d_bwd(const float* in, const float* flow, const float* grad_out,
                  float* grad_in, float* grad_flow,
                  int B, int C, const int* in_dhw, int D, int H, int W, fs_stream_t stream);

/* The IFNet call site warps BOTH frames with the two halves of one 6-channel flow:
 *   warped_img0 = warp(img0, flow[:, :3]); warped_img1 = warp(img1, flow[:, 3:6])
 *   (Flow-3D/model/IFNet.py:190-191, 233-234).  One launch serves both and uses flow6 /
 * grad_flow6 [B,6,D,H,W] in place (no slice copies).  grad_img0/grad_img1: both or neither.
 */
int fs_warp3d_pair_fwd(const float* img0, const float* img1, const float* flow6,
                       float* out0, float* out1,
                       int B, int C, const int* in_dhw, int D, int H, int W, fs_stream_t stream);
int fs_warp3d_pair_bwd(const float* img0, const float* img1, const float* flow6,
                       const float* grad_out0, const float* grad_out1,
                       float* grad_img0, float* grad_img1, float* grad_flow6,
                       int B, int C, const int* in_dhw, int D, int H, int W, fs_stream_t stream);
/* The same with the gradient that reaches the flow from its OTHER consumers summed in by the launch:
 * grad_flow6 = d(warps)/d(flow) + grad_flow_add (nullable; may BE grad_flow6 -- in-place accumulation).
 * An IFNet block's flow feeds the warp, the next block's input and accumulation, and the distillation
 * term (Flow-3D/model/IFNet.py:190-191, 210-214, 261); autograd would add the warp's share to the others'
 * in a separate pass over 805 MB tensors. */
int fs_warp3d_pair_bwd_acc(const float* img0, const float* img1, const float* flow6,
                           const float* grad_out0, const float* grad_out1,
                           float* grad_img0, float* grad_img1,
                           const float* grad_flow_add, float* grad_flow6,
                           int B, int C, const int* in_dhw, int D, int H, int W, fs_stream_t stream);

/* f1: "upsample flow x scale -> warp" in ONE kernel -- Flow-3D/model/IFNet.py:118
 *   flow = F.interpolate(flow_d, scale_factor=s, mode="trilinear", align_corners=False) * s   (+ the running
 *   flow of :213-214) followed by :190-191 warp(img0, flow[:, :3]), warp(img1, flow[:, 3:6]).
 * delta [B,6,Ds,Hs,Ws] is the head's output at the block's working resolution; prev_flow (nullable),
 * flow_out, out0, out1 live at factor x that extent (factor 2 or 4).  flow_out = prev_flow + scale *
 * upsample(delta) is formed per tile in registers, written once (it has three more consumers) and
 * handed to the warp without a second trip through HBM; values are bit-identical to
 * fs_upsample3d_scale_add + fs_warp3d_pair_fwd.
 * bwd: grad_flow_total = d(warps)/d(flow_out) + grad_flow_add (gradient reaching flow_out from its other
 * consumers; nullable; may alias grad_flow_total) -- also the gradient of prev_flow -- and
 * grad_delta = scale * adjoint_upsample(grad_flow_total).  ws: B*6*(D*H*Ws + D*Hs*Ws) floats. */
int fs_upsample_warp3d_pair_fwd(const float* img0, const float* img1, const float* delta,
                                const float* prev_flow, float* flow_out, float* out0, float* out1,
                                int B, int C, const int* in_dhw, int Ds, int Hs, int Ws, int factor,
                                float scale, fs_stream_t stream);
int fs_upsample_warp3d_pair_bwd(const float* img0, const float* img1, const float* flow6,
                                const float* grad_out0, const float* grad_out1,
                                const float* grad_flow_add, float* grad_flow_total, float* grad_delta,
                                float* ws, int B, int C, const int* in_dhw, int Ds, int Hs, int Ws,
                                int factor, float scale, fs_stream_t stream);
/* fs_warp3d_pair_bwd_acc / fs_upsample_warp3d_pair_bwd with up to THREE gradients reaching the flow from its
 * other consumers (Flow-3D/model/IFNet.py: the flow of a block feeds :190-191 the warps, :183 the next block's
 * input `torch.cat`, :213 the running-flow accumulation and :262 the distillation term).  Each add* (nullable)
 * is a [B,6,D,H,W] tensor or a 6-channel slice of a wider one: batch_stride* = its batch stride in floats
 * (>= 6*D*H*W), channel stride D*H*W.  add0 may alias grad_flow6 / grad_flow_total.  The gradients of the two
 * warped frames may be channel slices too (they are channels 2 and 3 of the next block's input gradient):
 * gout_batch_stride* = their batch stride in floats, 0 = dense (C*D*H*W). */
int fs_warp3d_pair_bwd_acc3(const float* img0, const float* img1, const float* flow6,
                            const float* grad_out0, long long gout_batch_stride0, const float* grad_out1,
                            long long gout_batch_stride1, float* grad_img0, float* grad_img1,
                            const float* add0, long long batch_stride0, const float* add1, long long batch_stride1,
                            const float* add2, long long batch_stride2, float* grad_flow6,
                            int B, int C, const int* in_dhw, int D, int H, int W, fs_stream_t stream);
int fs_upsample_warp3d_pair_bwd3(const float* img0, const float* img1, const float* flow6,
                                 const float* grad_out0, long long gout_batch_stride0, const float* grad_out1,
                                 long long gout_batch_stride1, const float* add0, long long batch_stride0, const float* add1, long long batch_stride1,
                                 const float* add2, long long batch_stride2, float* grad_flow_total, float* grad_delta,
                                 float* ws, int B, int C, const int* in_dhw, int Ds, int Hs, int Ws,
                                 int factor, float scale, fs_stream_t stream);

/* Which kernel the trilinear-warp entry points above dispatch a call of this geometry to (nothing is launched; the
 * pointers are inspected for alignment only, `in0` / `in1` = the sampled volumes, in1 NULL for a single warp):
 *   FS_W3_KERNEL_GATHER (0)  the global-gather kernels (rounds 1-4: warp3d_fwd_ring_kernel / warp3d_bwd_kernel)
 *   FS_W3_KERNEL_RC     (1)  round 5: ring pipeline with the gather source in an LDS row cache (warp3d_rc_kernel;
 *                            C == 1, W_in % 4 == 0, the 37-plane x 72-column window fits the sampled volume, 16-byte
 *                            aligned tensors, flow gradient only)
 * `backward` != 0: fs_warp3d*_bwd* with `with_grad_in` saying whether grad_in / grad_img* are asked for; a negative
 * return value is -FS_ERR_*.  (bench.py names the kernel symbol of its roofline records with it.)
 * The query sees in0, in1 and flow only.  A raw-ABI call whose out / grad_out / grad_flow / addend is not 16-byte
 * aligned, or whose addend / grad_out batch stride is not a multiple of 4 floats, runs the scalar gather kernels even
 * where the query answers FS_W3_KERNEL_RC (tests/mem_ledger.py, rows with plan None); the binding never makes such a
 * call: it allocates those tensors, and its slices are channel slices of W % 4 == 0 tensors. */
enum { FS_W3_KERNEL_GATHER = 0, FS_W3_KERNEL_RC = 1 };
int fs_warp3d_kernel_id(const float* in0, const float* in1, const float* flow, int B, int C, const int* in_dhw,
                        int D, int H, int W, int backward, int with_grad_in);

/* ------------------------------------------------------------------------------------
 * 2-D bilinear backward warps.  in [B,C,H,W], flow [B,2,H,W] (ch0 = x, ch1 = y),
 * out [B,C,H,W].  `mode` selects the reference call site whose coordinate convention is
 * reproduced:
 *   FS_WARP2D_RIFE    a1  Flow-2D/model/warplayer.py:7-26  border pad, align_corners=True,
 *                         samples at (x+u, y+v).
 *   FS_WARP2D_PWC     a5/a6 UPFlow/model/pwc_modules.py:184-207 (WarpingLayer_no_div) and
 *                         UPFlow/utils/tools.py:1317-1361 (torch_warp): vgrid = 2(x+u)/(W-1)-1,
 *                         zeros pad, align_corners=False.
 *   FS_WARP2D_PHOTO   a11 Flow-2D/model/RIFE.py:244-262 (`backwrd_warp`): grid = (x+u)*2/W-1,
 *                         zeros pad, align_corners=False => samples at (x+u-0.5, y+v-0.5).
 *   FS_WARP2D_DILATED a7  UPFlow/utils/tools.py:412-541 (boundary_dilated_warp.warp_im):
 *                         samples at (x+start_x+u, y+start_y+v), indices clamped, weights from
 *                         clamped corners vs unclamped coordinate.  `start` = [B,2] device
 *                         floats (x,y) or NULL for zeros.
 * `with_mask` (FS_WARP2D_PWC only): multiply by (sum of in-bounds weights >= 1.0), the
 *   validity mask of pwc_modules.py:200-207.
 * bwd: grad_in nullable (caller zero-fills; float atomics), grad_flow nullable (overwritten).
 */
enum { FS_WARP2D_RIFE = 0, FS_WARP2D_PWC = 1, FS_WARP2D_PHOTO = 2, FS_WARP2D_DILATED = 3 };

/* H, W = extent of the flow (= of the output).  `in_hw` = {Hin, Win} (HOST pointer to 2 ints) or NULL
 * when the image has the flow's extent; only FS_WARP2D_RIFE defines the other case (the reference builds
 * its grid from the flow's shape and its divisors from the input's, warplayer.py:10-20; IFNet-2D hits it
 * for extents where its blocks return fewer rows than the frames have, e.g. H = 146). */
int fs_warp2d_fwd(const float* in, const float* flow, const float* start, float* out,
                  int B, int C, const int* in_hw, int H, int W, int mode, int with_mask,
                  fs_stream_t stream);
int fs_warp2d_bwd(const float* in, const float* flow, const float* start,
                  const float* grad_out, float* grad_in, float* grad_flow,
                  int B, int C, const int* in_hw, int H, int W, int mode, int with_mask,
                  fs_stream_t stream);

/* Pair form for the IFNet call site (Flow-2D/model/IFNet.py:191-192, 230-231):
 *   warp(img0, flow[:, :2]); warp(img1, flow[:, 2:4])  with flow4 [B,4,H,W] used in place.
 * No mask, no start.  * Aliasing: grad_in / grad_img0 / grad_img1 are accumulated INTO (zero-fill them first).  Planes of <= 48 KB are added
 * by plane-owning workgroups with plain read-modify-writes, which needs every grad_img of a pair launch to be present and
 * the two to be different tensors; a pair launch whose grad_img0 == grad_img1 (or with one of them NULL where that is
 * allowed) takes the float-atomic kernel instead, which tolerates the aliasing. */
int fs_warp2d_pair_fwd(const float* img0, const float* img1, const float* flow4,
                       float* out0, float* out1,
                       int B, int C, const int* in_hw, int H, int W, int mode, fs_stream_t stream);
int fs_warp2d_pair_bwd(const float* img0, const float* img1, const float* flow4,
                       const float* grad_out0, const float* grad_out1,
                       float* grad_img0, float* grad_img1, float* grad_flow4,
                       int B, int C, const int* in_hw, int H, int W, int mode, fs_stream_t stream);

/* ------------------------------------------------------------------------------------
 * f2. Forward-backward occlusion check + outgoing mask, fused.
 *   UPFlow/utils/tools.py:560-590 (occ_check_model.__call__ dispatch), :592-630
 *   (_forward_backward_occ_check with length_sq_v0 = sum_c |x_c| and two torch_warp calls),
 *   :683-709 (torch_outgoing_occ_check), :711-719 (torch_get_obj_occ_check).
 *   flow_f, flow_b [B,2,H,W] -> occ_f, occ_b [B,1,H,W] in {0,1} (0 = occluded / ignore).
 *   alpha1, alpha2_over_scale: occ_thresh = alpha1 * (|flow_f|_1 + |flow_b|_1) + alpha2/scale.
 *   mode FS_OCC_ALL: the consistency masks; FS_OCC_OUT: the outgoing masks only;
 *   FS_OCC_OBJ: (consistent == 1) or (outgoing == 0) -- the reference's 'obj' setting.
 *   No gradient: the reference's masks are bool -> float.
 */
enum { FS_OCC_ALL = 0, FS_OCC_OBJ = 1, FS_OCC_OUT = 2 };
int fs_occ_check2d(const float* flow_f, const float* flow_b, float* occ_f, float* occ_b,
                   int B, int H, int W, float alpha1, float alpha2_over_scale, int mode,
                   fs_stream_t stream);

/* ------------------------------------------------------------------------------------
 * a3/a4. Local-window correlation (cost volume) -- replaces the `correlation_cuda` torch
 * extension bound at UPFlow/model/correlation_package/correlation.py:4,26-27,42-43
 * (sources absent from the reference tree; semantics pinned by Corr_pyTorch,
 * UPFlow/utils/pytorch_correlation.py:27-50) for the only configuration the reference uses:
 * pad_size = max_displacement = md, kernel_size = 1, stride1 = stride2 = 1, corr_multiply = 1
 * (UPFlow/model/upflow.py:649,652: md = 4).
 *   f1, f2 [B,C,H,W] -> out [B,(2md+1)^2,H,W],
 *   out[b,(dy+md)(2md+1)+(dx+md),y,x] = (1/C) sum_c f1[b,c,y,x] f2[b,c,y+dy,x+dx], zero pad.
 * md in 1..4.  bwd: grad_f1 / grad_f2 nullable (at least one), fully overwritten; no atomics,
 * bitwise reproducible.  The reference's rbot1/rbot2 scratch tensors have no equivalent.
 * Sizes: B*C*H*W and (2md+1)^2*H*W below 2^29 floats (32-bit byte offsets inside a tensor / a sample's
 * cost volume), FS_ERR_SHAPE otherwise; any alignment of rows (W need not be a multiple of 4).
 */
int fs_corr2d_fwd(const float* f1, const float* f2, float* out,
                  int B, int C, int H, int W, int max_displacement, fs_stream_t stream);
int fs_corr2d_bwd(const float* f1, const float* f2, const float* grad_out,
                  float* grad_f1, float* grad_f2,
                  int B, int C, int H, int W, int max_displacement, fs_stream_t stream);

/* f4. normalize_features folded into the cost volume: UPFlow/model/upflow.py:96-138
 * with normalize = center = True, moments_across_channels = moments_across_images = False (the
 * configuration UPFlow_net.demo() / C3 uses, upflow.py:635-641): every (b, c) plane of each feature map
 * is centred and scaled by its own mean / sqrt(unbiased var + 1e-16) immediately before
 * correlation.py:26.  The normalised maps are never materialised:
 *   fs_plane_moments   : stats[plane] = (mean, 1/sqrt(var + 1e-16)) for `planes` planes of S floats (S >= 2);
 *   fs_corr2d_norm_fwd : fs_corr2d_fwd of the normalised maps, normalisation applied as tiles are
 *                        staged (the zero padding of f2 applies AFTER normalisation, as in the reference);
 *   fs_corr2d_norm_bwd : gradients w.r.t. the NORMALISED maps (either may be NULL);
 *   fs_plane_norm_bwd  : chains one of them through the normalisation,
 *                        grad_f = r (grad_n - mean(grad_n) - n sum(grad_n n)/(S-1)).
 */
int fs_plane_moments(const float* f, float* stats, int planes, int S, fs_stream_t stream);
int fs_plane_norm_bwd(const float* f, const float* stats, const float* grad_n, float* grad_f,
                      int planes, int S, fs_stream_t stream);
int fs_corr2d_norm_fwd(const float* f1, const float* f2, const float* stats1, const float* stats2,
                       float* out, int B, int C, int H, int W, int max_displacement,
                       fs_stream_t stream);
int fs_corr2d_norm_bwd(const float* f1, const float* f2, const float* stats1, const float* stats2,
                       const float* grad_out, float* grad_n1, float* grad_n2,
                       int B, int C, int H, int W, int max_displacement, fs_stream_t stream);

/* Both directions of one pyramid level in ONE launch (UPFlow/model/upflow.py:649 and :652 correlate
 * (x1, x2_warp) and (x2, x1_warp) at every level): set a = (f1a, f2a) -> outa, set b = (f1b, f2b) -> outb,
 * identical shapes.  `stats` (nullable) = [4][B*C][2] (mean, rstd) tables of (f1a, f2a, f1b, f2b) as
 * fs_plane_moments4 writes them: the normalize_features-folded variant; with it, the bwd gradients are
 * w.r.t. the NORMALISED maps (chain them with fs_plane_norm_bwd4; a NULL grad_f skips that tensor).
 * The five levels of a step cannot share a launch: level l's features are warped with the flow estimated at
 * level l-1 (upflow.py:621-633). */
int fs_corr2d_pair_fwd(const float* f1a, const float* f2a, const float* f1b, const float* f2b,
                       const float* stats, float* outa, float* outb,
                       int B, int C, int H, int W, int max_displacement, fs_stream_t stream);
int fs_corr2d_pair_bwd(const float* f1a, const float* f2a, const float* f1b, const float* f2b,
                       const float* stats, const float* grad_outa, const float* grad_outb,
                       float* grad_f1a, float* grad_f2a, float* grad_f1b, float* grad_f2b,
                       int B, int C, int H, int W, int max_displacement, fs_stream_t stream);
int fs_plane_moments4(const float* fa, const float* fb, const float* fc, const float* fd, float* stats,
                      int planes, int S, fs_stream_t stream);
int fs_plane_norm_bwd4(const float* fa, const float* fb, const float* fc, const float* fd,
                       const float* stats, const float* grad_na, const float* grad_nb,
                       const float* grad_nc, const float* grad_nd, float* grad_fa, float* grad_fb,
                       float* grad_fc, float* grad_fd, int planes, int S, fs_stream_t stream);

/* 3-D correlation: NEW capability named by BASELINE.json (config 4); the reference has no 3-D cost
 * volume, so this generalises the 2-D layer above (dz-major, then dy, dx; channel mean; zero pad):
 *   f1, f2 [B,C,D,H,W] -> out [B,(2md+1)^3,D,H,W].  Pinned to the reference only through D = 1.
 * Sizes: B*C*D*H*W and (2md+1)^3*D*H*W below 2^29 floats, FS_ERR_SHAPE otherwise.
 */
int fs_corr3d_fwd(const float* f1, const float* f2, float* out,
                  int B, int C, int D, int H, int W, int max_displacement, fs_stream_t stream);
int fs_corr3d_bwd(const float* f1, const float* f2, const float* grad_out,
                  float* grad_f1, float* grad_f2,
                  int B, int C, int D, int H, int W, int max_displacement, fs_stream_t stream);

/* ------------------------------------------------------------------------------------
 * a9/a10. Robust penalty + (masked) reduction -- the arithmetic of
 *   loss_functions.photo_loss_function   UPFlow/utils/loss.py:17-48   (tail of the census loss)
 *   network_tools.photo_loss_multi_type  UPFlow/model/upflow.py:267-289
 *   torch.nn.functional.l1_loss          Flow-3D/model/RIFE.py:132-134 (FS_PEN_L1)
 * in one pass:  S1 = sum_e pen(x[e] - y[e]) * w,  S2 = sum w   (w broadcast over C; S2 counts
 * each pixel once).  x, y [B,C,S] (y NULL => pen(x)), w [B,1,S] or NULL (then S2 = 0).
 * pen: ABS_ROBUST (|v|+0.01)^q | CHARBONNIER (v^2+eps)^q | L1_EPS |v+1e-6| | L1 |v|.
 * `border` > 0 (needs S == H*W): weights within `border` px of the image edge are zeroed --
 * the inner mask of census_loss_torch (loss.py:74-88, max_distance = 3).
 * sums: 2 device floats.  ws: device scratch, 2*FS_REDUCE_BLOCKS floats (caller-owned).
 * The caller turns (S1, S2) into the reference's mean / ratio forms.  Deterministic.
 * bwd: grad_x[e] = coef[0] * pen'(x-y) * w ; grad_y = -grad_x.  coef = device scalar
 * (upstream gradient times d loss / d S1).
 */
enum { FS_PEN_ABS_ROBUST = 0, FS_PEN_CHARBONNIER = 1, FS_PEN_L1_EPS = 2, FS_PEN_L1 = 3 };
#define FS_REDUCE_BLOCKS 1024

int fs_robust_sum(const float* x, const float* y, const float* w, float* sums, float* ws,
                  int B, int C, int S, int H, int W, int border, int mode, float q, float eps,
                  fs_stream_t stream);
int fs_robust_sum_bwd(const float* x, const float* y, const float* w, const float* coef,
                      float* grad_x, float* grad_y,
                      int B, int C, int S, int H, int W, int border, int mode, float q, float eps,
                      fs_stream_t stream);

/* a9, 'SSIM' branch: network_tools.weighted_ssim (UPFlow/model/upflow.py:141-196, c1 = inf,
 * c2 = 9e-6, weight_epsilon = 0.01, 3x3 valid average pools) fused with the reduction of
 * photo_loss_multi_type (:285-289):  sums[0] = sum ld * (use_occ ? avgpool(weight) : 1),
 * sums[1] = sum avgpool(weight);  x, y [B,C,H,W], weight [B,1,H,W], H, W >= 3.
 * loss = sums[0]/(sums[1]+1e-6) (use_occ) or sums[0]/(B*C*(H-2)*(W-2)).  ws as for fs_robust_sum.
 * bwd: grad_x / grad_y (nullable) = coef[0] * d sums[0] / d x, y  (the weight carries no gradient).
 */
int fs_wssim_fwd(const float* x, const float* y, const float* weight, float* sums, float* ws,
                 int B, int C, int H, int W, int use_occ, fs_stream_t stream);
int fs_wssim_bwd(const float* x, const float* y, const float* weight, const float* coef,
                 float* grad_x, float* grad_y, int B, int C, int H, int W, int use_occ,
                 fs_stream_t stream);

/* ------------------------------------------------------------------------------------
 * a8. Census (soft ternary) distance -- loss_functions.census_loss_torch,
 * UPFlow/utils/loss.py:51-72: grey = .2989R+.5870G+.1140B; 7x7 zero-padded neighbourhood
 * differences t = d/sqrt(0.81+d^2); dist = sum_49 (t1-t2)^2/(0.1+(t1-t2)^2).
 *   img1, img2 [B,3,H,W] -> dist [B,1,H,W].  max_distance must be 3.
 * The loss is fs_robust_sum(dist, w = occ mask, border = 3, ...).
 * bwd: grad_dist [B,1,H,W] -> grad_img1 / grad_img2 [B,3,H,W] (nullable, overwritten);
 * gather-formulated, no atomics.
 */
int fs_census_dist_fwd(const float* img1, const float* img2, float* dist,
                       int B, int H, int W, int max_distance, fs_stream_t stream);
int fs_census_dist_bwd(const float* img1, const float* img2, const float* grad_dist,
                       float* grad_img1, float* grad_img2,
                       int B, int H, int W, int max_distance, fs_stream_t stream);

/* ------------------------------------------------------------------------------------
 * a12. IFNet epilogues (Flow-2D/model/IFNet.py:239-248, Flow-3D/model/IFNet.py:241-267).
 * merge:   merged[B,C,S] = w0 * sigmoid(m) + w1 * (1 - sigmoid(m)),  m [B,1,S];
 *          sigmoid_out [B,1,S] nullable (the reference keeps it as mask_list[i]).
 * distill: sums[0] = sum_voxels sqrt(mean_c (flow_tea - flow_i)^2) * loss_mask,
 *          sums[1] = sum loss_mask,  loss_mask = mean_c|merged_i-gt| > mean_c|merged_tea-gt| + 0.01;
 *          merged_*, gt [B,C,S]; flow_* [B,F,S].  The term of loss_distill is sums[0] / (B*S).
 *          bwd: grad_flow_i only (teacher flow and mask are detached in the reference).
 */
int fs_merge_fwd(const float* w0, const float* w1, const float* mask_logit,
                 float* merged, float* sigmoid_out, int B, int C, int S, fs_stream_t stream);
int fs_merge_bwd(const float* w0, const float* w1, const float* mask_logit,
                 const float* grad_merged, const float* grad_sigmoid,
                 float* grad_w0, float* grad_w1, float* grad_mask_logit,
                 int B, int C, int S, fs_stream_t stream);
int fs_distill_fwd(const float* merged_i, const float* merged_tea, const float* gt,
                   const float* flow_i, const float* flow_tea, float* sums, float* ws,
                   int B, int C, int F, int S, fs_stream_t stream);
int fs_distill_bwd(const float* merged_i, const float* merged_tea, const float* gt,
                   const float* flow_i, const float* flow_tea, const float* coef,
                   float* grad_flow_i, int B, int C, int F, int S, fs_stream_t stream);
/* The three student terms of loss_distill (one per block, all against the same teacher: Flow-3D/model/
 * IFNet.py:259-262, Flow-2D/model/IFNet.py:244-248) in one launch each way: the teacher's flow / merged frame
 * and the ground truth are read once instead of three times.  sums[0..2] = the per-term sums of
 * sqrt(mean_c dflow^2) * mask (divide by B*S for the means; sums[3] is scratch: pass 4 floats);
 * ws: 4 * FS_REDUCE_BLOCKS floats.  bwd: coef = device scalar d(objective)/d(sum), shared by the terms. */
int fs_distill3_fwd(const float* merged0, const float* merged1, const float* merged2,
                    const float* merged_tea, const float* gt, const float* flow0, const float* flow1,
                    const float* flow2, const float* flow_tea, float* sums, float* ws,
                    int B, int C, int F, int S, fs_stream_t stream);
int fs_distill3_bwd(const float* merged0, const float* merged1, const float* merged2,
                    const float* merged_tea, const float* gt, const float* flow0, const float* flow1,
                    const float* flow2, const float* flow_tea, const float* coef,
                    float* grad_flow0, float* grad_flow1, float* grad_flow2,
                    int B, int C, int F, int S, fs_stream_t stream);

/* ------------------------------------------------------------------------------------
 * §8f.1  Backward of the trilinear resizes inside IFBlock (Flow-3D/model/IFNet.py:85,88,118-119):
 * F.interpolate(mode="trilinear", align_corners=False, scale_factor = `factor` (upsample = 1) or
 * 1/`factor` (upsample = 0)), factor in {2, 4}.  grad_out [B,C,Dout,Hout,Wout] ->
 * grad_in [B,C,Din,Hin,Win], with out = in*factor (up) or in/factor (down, floor).
 * Gather-formulated adjoint (ATen scatters with atomics): no atomics, reproducible.
 * ws: device scratch for the up-sampling case, B*C*(Dout*Hout*Win + Dout*Hin*Win) floats (the
 * adjoint then runs as three separable 1-D passes); NULL selects the single-pass kernel.
 */
int fs_interp3d_bwd(const float* grad_out, float* grad_in, float* ws, int B, int C,
                    int Din, int Hin, int Win, int Dout, int Hout, int Wout,
                    int factor, int upsample, fs_stream_t stream);
/* grad_in = scale * adjoint(grad_out): the `* scale` of `F.interpolate(flow_d, ...) * scale` (IFNet.py:118)
 * folded into the last separable pass.  scale != 1 needs upsample = 1 and ws != NULL (FS_ERR_ARG otherwise). */
int fs_interp3d_bwd_scaled(const float* grad_out, float* grad_in, float* ws, int B, int C,
                           int Din, int Hin, int Win, int Dout, int Hout, int Wout,
                           int factor, int upsample, float scale, fs_stream_t stream);

/* Forward of the down-scaling side (Flow-3D/model/IFNet.py:85, 88):
 *   out = scale * F.interpolate(in, scale_factor = 1/factor, mode="trilinear", align_corners=False)
 * in [B,C,Din,Hin,Win] -> out [B,C,Din/factor,...] (floor), factor in {2, 4}; `scale` carries the flow's
 * `* 1. / scale` (:88).  ATen's arithmetic and summation order (every lambda is 1/2: bit-identical to ATen).  Adjoint: fs_interp3d_bwd
 * with upsample = 0. */
int fs_downsample3d_fwd(const float* in, float* out, int B, int C, int Din, int Hin, int Win,
                        int factor, float scale, fs_stream_t stream);
/* the same over an input whose C <= 12 channels are planes of different tensors (IFBlock's `torch.cat` in front of its
 * down-sampling, Flow-3D/model/IFNet.py:183 + :85): src[c] = channel c of sample 0, batch_strides[c] = that tensor's
 * batch stride in floats (host arrays, read at launch). */
int fs_downsample3d_fwd_ms(const float* const* src, const long long* batch_strides, float* out, int B, int C,
                           int Din, int Hin, int Win, int factor, float scale, fs_stream_t stream);

/* The 2-D pair (Flow-2D/model/IFNet.py:89, 92, 115-116): out = scale * F.interpolate(in, scale_factor =
 * factor (upsample = 1) or 1/factor (upsample = 0), mode="bilinear", align_corners=False), factor in {2, 4},
 * in [B,C,Hin,Win] -> out [B,C,Hout,Wout] with out = in*factor or floor(in/factor); ATen's arithmetic.
 * bwd: grad_in = scale * adjoint(grad_out), a gather per input pixel (no atomics, reproducible). */
int fs_resize2d_fwd(const float* in, float* out, int B, int C, int Hin, int Win, int Hout, int Wout,
                    int factor, int upsample, float scale, fs_stream_t stream);
int fs_resize2d_bwd(const float* grad_out, float* grad_in, int B, int C, int Hin, int Win, int Hout,
                    int Wout, int factor, int upsample, float scale, fs_stream_t stream);

/* Forward companion for the up-sampling side (Flow-3D/model/IFNet.py:118-119 followed by the
 * accumulation at :213-214 / :228-229):
 *   out = prev + scale * interpolate(small, scale_factor = factor, trilinear, align_corners=False)
 * small [B,C,Din,Hin,Win] -> out [B,C,factor*Din,...]; prev (same shape as out) may be NULL (= 0);
 * factor in {2, 4}.  ATen's index / weight arithmetic and summation order.  The adjoint of the
 * interpolation is fs_interp3d_bwd (times scale); d out / d prev is the identity. */
int fs_upsample3d_scale_add(const float* small, const float* prev, float* out, int B, int C,
                            int Din, int Hin, int Win, int factor, float scale, fs_stream_t stream);

/* ------------------------------------------------------------------------------------
 * f3. Laplacian-pyramid L1 loss of Flow-2D: Flow-2D/model/laplacian.py:10-88
 * (gauss_kernel :10-19, downsample :21-22, upsample :24-36, conv_gauss :38-47,
 * laplacian_pyramid :49-74, LapLoss.forward :81-88).
 *   loss = sum_{l < levels} mean | pyr_l(input) - pyr_l(target) |  computed as ONE pyramid of
 *   (input - target) -- every pyramid step is linear.
 * input, target [N,H,W] (N = B*C; the 5x5 filter is depthwise), target may be NULL (= zeros).
 * Every level needs extent >= 3 (reflect padding by 2; torch raises there too) -> FS_ERR_SHAPE.
 * fs_laploss2d_sizes: host-only; element counts of the three caller-owned fp32 buffers.
 *   sgn  : sign(pyr_l) / numel_l for every level, written by fwd, read by bwd (save it);
 *   ws   : scratch (fwd: ws_fwd_floats, bwd: ws_bwd_floats), contents need not survive.
 * fwd : loss[0] = the loss (loss[1] is scratch; pass 2 floats).
 * bwd : grad_loss = device pointer to d(objective)/d(loss) (1 float);
 *       grad_diff [N,H,W] = d/d(input) = -d/d(target).  Gathers only, deterministic.
 */
int fs_laploss2d_sizes(int N, int H, int W, int levels, long long* sgn_floats,
                       long long* ws_fwd_floats, long long* ws_bwd_floats);
int fs_laploss2d_fwd(const float* input, const float* target, float* sgn, float* ws, float* loss,
                     int N, int H, int W, int levels, fs_stream_t stream);
int fs_laploss2d_bwd(const float* sgn, const float* grad_loss, float* ws, float* grad_diff,
                     int N, int H, int W, int levels, fs_stream_t stream);

/* f3, second half: the 3-D Laplacian-pyramid L1 loss.  PARITY UNPINNED: Flow-3D/model/laplacian.py:37-91 is
 * dead code in the reference (commented out of Model.update, Flow-3D/model/RIFE.py:126,132) whose conv_gauss
 * (:44-58) ignores its kernel, round-trips through scipy.ndimage.gaussian_filter on the CPU over all five
 * axes and detaches the result.  Built here: the 3-D analogue of the 2-D loss above -- filtered = G3(reflect
 * pad 2)(cur) with G3 = g (x) g (x) g, g = [1,4,6,4,1]/16; down = filtered[::2,::2,::2]; up = (8 G3)(reflect
 * pad 2)(zero-interleave(down)) (the reference's `x_up * 8`, laplacian.py:41); pyr = cur - up; loss =
 * sum_l mean |pyr_l(input) - pyr_l(target)|.  Same buffer protocol as fs_laploss2d_*; input, target
 * [N,D,H,W] (N = B*C); every level needs extent >= 3 per axis. */
int fs_laploss3d_sizes(int N, int D, int H, int W, int levels, long long* sgn_floats,
                       long long* ws_fwd_floats, long long* ws_bwd_floats);
int fs_laploss3d_fwd(const float* input, const float* target, float* sgn, float* ws, float* loss,
                     int N, int D, int H, int W, int levels, fs_stream_t stream);
int fs_laploss3d_bwd(const float* sgn, const float* grad_loss, float* ws, float* grad_diff,
                     int N, int D, int H, int W, int levels, fs_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Forward pass of the IFNet-3D convolutions as an implicit GEMM on the fp32 matrix cores
 * (companion of fs_conv3d_wrw; `conv()` / IFBlock.conv0 / convblock in Flow-3D/model/IFNet.py:13-29,
 * 31-76: Conv3d(k=3,s=1,p=1) and Conv3d(k=4,s=2,p=1), NCDHW fp32).
 *   y[b,co,o] = bias[co] + sum_{ci,k} W[co,ci,k] * x[b,ci, o*stride + k - pad]   (zero padding)
 * x [B,Cin,Di,Hi,Wi] -> y [B,Cout,Do,Ho,Wo], Do = (Di + 2 pad - kernel)/stride + 1 (checked).
 * (kernel,stride) in {(3,1),(4,2)}.  bias may be NULL.
 * wmode 0: w is [Cout][Cin][k^3] (Conv3d forward; also the INPUT GRADIENT of a ConvTranspose3d, whose
 *          weight tensor [Cin_t][Cout_t][k^3] already reads as [out][in] of that convolution);
 * wmode 1: w is [Cin][Cout][k^3] and is applied flipped (tap k^3-1-k): the INPUT GRADIENT of a
 *          stride-1 "same" Conv3d is this convolution of grad_out with the layer's own weight.
 * ws: device scratch of fs_conv3d_fwd_ws_floats(Cin, Cout, kernel) floats (re-laid-out weights).
 * Alignment: y, and z / addend / residual / grad_act_y / act_y of the variants below, must be 16-byte aligned (the
 * epilogues move 16 bytes at a time); FS_ERR_ARG otherwise, before anything is launched.  The same holds for y, z and
 * addend of fs_conv3d_tr*.  x and ws may have any 4-byte alignment (a misaligned one only selects a slower kernel).
 */
long long fs_conv3d_fwd_ws_floats(int Cin, int Cout, int kernel);
int fs_conv3d_fwd(const float* x, const float* w, const float* bias, float* y, float* ws,
                  int B, int Cin, int Cout, int Di, int Hi, int Wi, int Do, int Ho, int Wo,
                  int kernel, int stride, int pad, int wmode, fs_stream_t stream);

/* ------------------------------------------------------------------------------------
 * ConvTranspose3d(k=4, s=2, p=1) forward -- the IFNet-3D heads (`conv1` / `conv2` of IFBlock,
 * Flow-3D/model/IFNet.py:62-75) -- which is also the INPUT GRADIENT of Conv3d(k=4, s=2, p=1)
 * (IFBlock.conv0, Flow-3D/model/IFNet.py:34-37) applied to grad_out.
 *   y[b,co,o] = bias[co] + sum_{ci,k : (o + 1 - k) even} x[b,ci,(o + 1 - k)/2] * w[ci,co,k]
 * x [B,Cin,Di,Hi,Wi], w [Cin][Cout][4*4*4] (a ConvTranspose3d weight as stored; a Conv3d weight
 * [Cout_conv][Cin_conv][64] reads the same way for its input gradient), bias may be NULL,
 * y [B,Cout,Dout,Hout,Wout] with out = 2*in per axis (or 2*in + 1: input gradient of a convolution
 * with an odd input extent -- its last plane is read by tap 3 of the last output, so it is not zero).
 * Cout <= 32 (FS_ERR_ARG otherwise).  ws: fs_conv3d_tr_ws_floats(Cin, Cout) floats of device scratch
 * (0 for Cout <= 6: those run on the vector ALUs with scalar-loaded weights).
 */
/* fs_conv3d_fwd_prelu / fs_conv3d_tr_prelu: the same convolutions with the PReLU that follows every one of
 * them in IFNet (`conv()` / `deconv()`, Flow-3D/model/IFNet.py:13-29) applied in the epilogue:
 * y = conv(x) + bias (kept: the PReLU backward needs it) and z = y > 0 ? y : prelu_weight[c] * y are written
 * in the same pass (num_prelu_weights = 1 or Cout).  fwd_prelu is wmode 0 only; its `residual` (may be
 * NULL, z's shape) is added to z: the `convblock(x) + x` of IFBlock.forward (Flow-3D/model/IFNet.py:101-104).
 * fs_conv3d_fwd_add: y = conv(x) + bias + addend (y's shape) -- with wmode 1 the input gradient of such a
 * residual unit, whose skip branch contributes grad_out itself. */
int fs_conv3d_fwd_add(const float* x, const float* w, const float* bias, const float* addend, float* y,
                      float* ws, int B, int Cin, int Cout, int Di, int Hi, int Wi, int Do, int Ho, int Wo,
                      int kernel, int stride, int pad, int wmode, fs_stream_t stream);
/* The backward counterpart for the heads (Flow-3D/model/IFNet.py:66-77: deconv -> PReLU -> deconv): the input gradient
 * of the SECOND deconvolution (a strided convolution of its grad_out, weight read as [out][in], wmode 0) with the PReLU
 * backward of the layer in between folded into the epilogue -- grad_act_y = conv(x) * prelu'(act_y), plus the PReLU
 * weight gradient and the first deconvolution's bias gradient (deterministic: per-wave partials in `part`,
 * fs_conv3d_fwd_dprelu_part_floats floats, summed in a fixed order).  FS_ERR_UNSUPPORTED: no such kernel for this
 * shape / alignment -- use fs_conv3d_fwd followed by fs_prelu_bwd.
 * kernel 3 (stride 1, pad 1): the same for the INNER PReLU of an IFBlock residual unit (Flow-3D/model/IFNet.py:101-104,
 * `convblock(x) + x` with convblock = conv, PReLU, conv, PReLU): x = grad w.r.t. the second convolution's output,
 * w = that convolution's weight as stored (read flipped + transposed, as fs_conv3d_fwd wmode 1), act_y = the first
 * convolution's output. */
long long fs_conv3d_fwd_dprelu_part_floats(int B, int Cout, int Do, int Ho, int Wo);    /* kernel 4 */
long long fs_conv3d_fwd_dprelu_part_floats_k3(int B, int Cout, int Do, int Ho, int Wo); /* kernel 3 */
int fs_conv3d_fwd_dprelu(const float* x, const float* w, const float* act_y, const float* prelu_weight,
                         int num_prelu_weights, float* grad_act_y, float* grad_prelu_weight, float* grad_bias,
                         float* part, float* ws, int B, int Cin, int Cout, int Di, int Hi, int Wi, int Do, int Ho, int Wo,
                         int kernel, int stride, int pad, fs_stream_t stream);
int fs_conv3d_fwd_prelu(const float* x, const float* w, const float* bias, const float* prelu_weight,
                        const float* residual, float* y, float* z, float* ws,
                        int B, int Cin, int Cout, int Di, int Hi, int Wi, int Do, int Ho, int Wo,
                        int kernel, int stride, int pad, int num_prelu_weights, fs_stream_t stream);
int fs_conv3d_tr_prelu(const float* x, const float* w, const float* bias, const float* prelu_weight,
                       float* y, float* z, float* ws,
                       int B, int Cin, int Cout, int Di, int Hi, int Wi, int Dout, int Hout, int Wout,
                       int num_prelu_weights, fs_stream_t stream);
/* fs_conv3d_tr_add: y = conv_transpose(x) + bias + addend (addend has y's shape): the head's flow / mask
 * delta accumulated onto the running flow / mask (Flow-3D/model/IFNet.py:213-214, 228-229) in the epilogue. */
int fs_conv3d_tr_add(const float* x, const float* w, const float* bias, const float* addend, float* y,
                     float* ws, int B, int Cin, int Cout, int Di, int Hi, int Wi,
                     int Dout, int Hout, int Wout, fs_stream_t stream);
long long fs_conv3d_tr_ws_floats(int Cin, int Cout);
int fs_conv3d_tr(const float* x, const float* w, const float* bias, float* y, float* ws,
                 int B, int Cin, int Cout, int Di, int Hi, int Wi, int Dout, int Hout, int Wout,
                 fs_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Backward of torch.nn.PReLU(num_parameters = C or 1) as used after every IFNet convolution
 * (`conv()` in Flow-2D/model/IFNet.py and Flow-3D/model/IFNet.py):  y = x > 0 ? x : a[c] x.
 *   grad_x[e] = x > 0 ? g : a[c] g ;  grad_weight[c] = sum_{b,spatial} (x > 0 ? 0 : x g).
 * x, grad_out, grad_x [B,C,S]; weight, grad_weight [num_weights]; ws: device scratch of
 * B*C*FS_PRELU_MAX_CHUNKS floats.  One pass + a tiny deterministic finishing kernel.
 * grad_bias (may be NULL) [C]: additionally sum_{b,spatial} grad_x per channel -- the bias gradient
 * of the convolution that produced x, for free in the same pass (ws must then hold
 * 2*B*C*FS_PRELU_MAX_CHUNKS floats).
 */
#define FS_PRELU_MAX_CHUNKS 64
int fs_prelu_bwd(const float* x, const float* grad_out, const float* weight,
                 float* grad_x, float* grad_weight, float* grad_bias, float* ws,
                 int B, int C, int S, int num_weights, fs_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Weight gradient of the IFNet-3D convolutions (callers of the hot path; MIOpen's own weight-gradient
 * solvers have no gfx950 tuning) as an implicit GEMM on the fp32 matrix cores:
 *   dw[g, c, kz,ky,kx] += sum_{b,o} g[b,g,o] * src[b,c, o*stride + k - pad]     (zero outside src)
 * g [B,Cg,Do,Ho,Wo], src [B,Cs,Di,Hi,Wi], dw [Cg,Cs,k,k,k] (caller zero-fills; float atomics).
 *   torch.nn.Conv3d:          g = grad_output, src = input        -> dw = weight.grad [Cout,Cin,k,k,k]
 *   torch.nn.ConvTranspose3d: g = input,       src = grad_output  -> dw = weight.grad [Cin,Cout,k,k,k]
 * (kernel, stride) in {(3,1), (4,2)} -- the IFBlock layers (Flow-3D/model/IFNet.py:33-78).
 */
int fs_conv3d_wrw(const float* g, const float* src, float* dw, int B, int Cg, int Cs,
                  int Do, int Ho, int Wo, int Di, int Hi, int Wi,
                  int kernel, int stride, int pad, fs_stream_t stream);
/* Which kernel fs_conv3d_wrw runs for these arguments (its own dispatch, nothing launched, pointers only inspected
 * for alignment; `dw` is not needed): FS_WRW_KERNEL_* >= 0, or -(FS_ERR_*) for arguments it would refuse.  For flop
 * accounting (the Winograd form executes half the direct form's multiply-adds) and for tests that must know which
 * kernel they exercised. */
enum { FS_WRW_KERNEL_BRICK = 0,   /* register-staged position bricks (any shape) */
       FS_WRW_KERNEL_DMA = 1,     /* loader-wave form, direct implicit GEMM */
       FS_WRW_KERNEL_WINO23 = 2,  /* Winograd F(2,3) along x (ablation build only) */
       FS_WRW_KERNEL_WINO43 = 3,  /* Winograd F(4,3) along x: the 64 -> 64 k3 trunk layers */
       FS_WRW_KERNEL_S3 = 4       /* loader-wave form on split-bf16 matrix cores: the k = 4 layers with >= 3 source channels */ };
int fs_conv3d_wrw_kernel_id(const float* g, const float* src, int B, int Cg, int Cs,
                            int Do, int Ho, int Wo, int Di, int Hi, int Wi, int kernel, int stride, int pad);

/* IFBlock's first convolution without its `torch.cat` (Flow-3D/model/IFNet.py:183 `x = torch.cat((x, flow), 1)`
 * over `torch.cat((img0, img1, warped_img0, warped_img1, mask), 1)`, :190-191): the Cin <= 12 input channels are
 * planes of the tensors they already live in.  src[c] = device pointer to channel c of sample 0 (16-byte aligned),
 * batch_strides[c] = the batch stride of its tensor in floats (a multiple of 4, >= D*H*W); both are HOST arrays of
 * Cin entries, read at launch.  fs_conv3d_fwd_prelu_ms == fs_conv3d_fwd_prelu without `residual`;
 * fs_conv3d_wrw_ms == fs_conv3d_wrw with that source.  FS_ERR_UNSUPPORTED when the shape has no loader-wave
 * kernel (k = 4, <= 32 output / gradient channels, W % 4 == 0, enough bricks): concatenate and use the plain
 * entry points. */
int fs_conv3d_fwd_prelu_ms(const float* const* src, const long long* batch_strides, const float* w, const float* bias,
                           const float* prelu_weight, float* y, float* z, float* ws,
                           int B, int Cin, int Cout, int Di, int Hi, int Wi, int Do, int Ho, int Wo,
                           int kernel, int stride, int pad, int num_prelu_weights, fs_stream_t stream);
int fs_conv3d_wrw_ms(const float* g, const float* const* src, const long long* batch_strides, float* dw,
                     int B, int Cg, int Cs, int Do, int Ho, int Wo, int Di, int Hi, int Wi,
                     int kernel, int stride, int pad, fs_stream_t stream);

/* Deterministic weight gradient (round 4).  fs_conv3d_wrw / _ms split the positions into runs whose partial tiles
 * meet in dw through float atomics: the order of arrival decides the last bits.  Here every run STORES its partial
 * tile into its own copy of dw inside a caller-owned workspace and one more launch adds the copies in run order:
 * same kernels, same dispatch, bitwise reproducible from run to run; dw is overwritten (no zero fill).
 *   fs_conv3d_wrw_det_ws_floats: floats of workspace this call needs (runs x Cg*Cs*k^3; its own dispatch, nothing
 *   launched), or -(FS_ERR_*).  src_planes / batch_strides both NULL: one `src` tensor; both non-NULL: the
 *   multi-source form of fs_conv3d_wrw_ms (`src` ignored).
 * The Python binding takes this path when torch.are_deterministic_algorithms_enabled(). */
long long fs_conv3d_wrw_det_ws_floats(const float* g, const float* src, const float* const* src_planes,
                                      const long long* batch_strides, int B, int Cg, int Cs,
                                      int Do, int Ho, int Wo, int Di, int Hi, int Wi, int kernel, int stride, int pad);
int fs_conv3d_wrw_det(const float* g, const float* src, const float* const* src_planes, const long long* batch_strides,
                      float* dw, float* ws, long long ws_floats, int B, int Cg, int Cs,
                      int Do, int Ho, int Wo, int Di, int Hi, int Wi, int kernel, int stride, int pad,
                      fs_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Weight preparation in one launch per optimiser step.  fs_conv3d_fwd* / fs_conv3d_tr* re-lay their weights into
 * `ws` with a small launch in front of every convolution (~110 launches of ~5 us per 256^3 Flow-3D step).  A caller
 * that keeps one `ws` per (layer, use) alive can instead (1) ask each entry point ONCE which re-layout it would run
 * for its shape -- fs_conv3d_fwd_wprep_jobs / fs_conv3d_tr_wprep_jobs take the arguments of fs_conv3d_fwd /
 * fs_conv3d_tr (the same dispatch code runs, nothing is launched) and write FsWprepJob records to a HOST array,
 * returning their number (0: this shape reads `w` directly; < 0: -FS_ERR_*; more than `cap`: array too small);
 * (2) after every weight update run all jobs with ONE fs_conv3d_wprep_batch launch (`jobs` in DEVICE memory);
 * (3) call the convolutions with w = NULL: "`ws` is already prepared".  Passing w != NULL keeps the classic
 * behaviour.  The fused variants (_add, _prelu, _prelu_ms, _dprelu) use the layout of their plain entry point
 * (fs_conv3d_fwd_dprelu: wmode = kernel == 3).  `x` is only inspected for its alignment; `has_prelu_out`: the
 * fs_conv3d_tr_prelu form (its two outputs rule out the all-parities kernel). */
typedef struct FsWprepJob {
  const float* w; /* source weights (device) */
  float* ws;      /* destination slab (device) */
  int kind;       /* layout, private to the library */
  int total;      /* floats written */
  int p[6];       /* layout parameters, private to the library */
} FsWprepJob;
int fs_conv3d_fwd_wprep_jobs(FsWprepJob* jobs_host, int cap, const float* x, const float* w, float* ws,
                             int B, int Cin, int Cout, int Di, int Hi, int Wi, int Do, int Ho, int Wo,
                             int kernel, int stride, int pad, int wmode);
int fs_conv3d_tr_wprep_jobs(FsWprepJob* jobs_host, int cap, const float* x, const float* w, float* ws, int B, int Cin,
                            int Cout, int Di, int Hi, int Wi, int Dout, int Hout, int Wout, int has_prelu_out);
int fs_conv3d_wprep_batch(const FsWprepJob* jobs_dev, int njobs, fs_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Sequence evaluation metrics -- error.py:27-56 calculate_psnr / ssim, per frame, N frames per launch.
 *   x, y [N,C,H,W] (2-D) or [N,C,D,H,W] (3-D), fp32, any value range L (`L` = data range: 255 for the reference's
 *   bytes, 1 for [0,1] data).  For every frame n:
 *     out_sse[n]      = sum over all C*H*W (C*D*H*W) elements of (x - y)^2                       (fp64)
 *     out_ssim_sum[n] = sum over the C channels and the VALID region of the SSIM map             (fp64)
 *   SSIM map: separable 11-tap Gaussian window g = cv2.getGaussianKernel(11, 1.5) along each axis, valid region
 *   (H-10) x (W-10) (2-D) or (D-10)(H-10)(W-10) (3-D), sigma^2 = E[x^2] - mu^2, C1 = (0.01 L)^2, C2 = (0.03 L)^2,
 *   ssim = ((2 mx my + C1)(2 sxy + C2)) / ((mx^2 + my^2 + C1)(sxx + syy + C2)).  PSNR = 10 log10(L^2 / mse) with
 *   mse = out_sse / (C*H*W), the mean SSIM = out_ssim_sum / (C * valid region); for C = 3 the mean over channels is
 *   what error.py:68-72 returns.  The reference has no working 3-D form (calculate_ssim returns None for volumes,
 *   error.py:67-74): the 3-D window is the same construction along a third axis, pinned by this project's fp64
 *   restatement only.
 *   fp32 inputs, fp64 window sums, fp64 partials per workgroup in `ws` (fs_frame_metrics{2,3}d_ws_bytes bytes, 8-byte aligned),
 *   summed by a second launch in a fixed order: bitwise reproducible, no atomics.
 *   FS_ERR_SHAPE: N or C < 1, a filtered extent below 11, or a grid beyond 2^24 workgroups; FS_ERR_ARG: L <= 0.
 *   The _ws_bytes queries launch nothing and return the byte count or -(FS_ERR_*).
 */
long long fs_frame_metrics2d_ws_bytes(int N, int C, int H, int W);
long long fs_frame_metrics3d_ws_bytes(int N, int C, int D, int H, int W);
int fs_frame_metrics2d(const float* x, const float* y, int N, int C, int H, int W, double L, double* ws,
                       double* out_sse, double* out_ssim_sum, fs_stream_t stream);
int fs_frame_metrics3d(const float* x, const float* y, int N, int C, int D, int H, int W, double L, double* ws,
                       double* out_sse, double* out_ssim_sum, fs_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Flow accuracy -- end-point error, RMSE, angular error and the KITTI outlier rate Fl of N predicted flows against N
 * ground-truth displacements, one launch.
 *   pred, gt: N flows of C fp32 planes of D*H*W (2-D: D = 1, C = 2; 3-D: C = 3) elements each; the planes of one flow
 *     are contiguous ([C, D, H, W]), flow n starts at pred + n * pred_bstride (gt + n * gt_bstride) elements, so the
 *     channel slice flow[:, C:2C] of an [N, 2C, ...] tensor is passed without a copy (bstride >= C*D*H*W when N > 1).
 *     Channel 0 is the displacement along W, 1 along H, 2 along D, in elements.
 *   valid, noc: uint8 [N, D, H, W] (contiguous, nonzero = set) or NULL.  valid NULL: every element is valid.  noc NULL:
 *     no occlusion split (the noc sums stay 0).  noc only counts where valid is set.
 *   convention (3-D only): FS_FLOW_DISP, or FS_FLOW_RIFE3D: pred is a Flow-3D (rife3d) flow, whose warp rotates axes
 *     (out[d,h,w] samples the input at ix = (h+F0)(W-1)/(H-1), iy = (d+F1)(H-1)/(D-1), iz = (w+F2)(D-1)/(W-1)); the
 *     kernel converts it to the displacement x = ix - w, y = iy - h, z = iz - d (fp64, not clamped) first.  gt is
 *     always a displacement.  RIFE3D needs D, H, W >= 2 (FS_ERR_SHAPE).
 *   Per element: e2 = |p - g|^2 and epe = sqrt(e2) in fp64; ae = atan2(|a x b|, a.b) with a = (p, 1), b = (g, 1), its
 *     arguments in fp64 and the atan2 in fp32 (radians); outlier = e2 > tau_abs^2 && e2 > tau_rel^2 |g|^2 (fp64; KITTI
 *     Fl: epe > 3 px and > 5 % of |g|).  An element whose pred or gt has a non-finite component counts in n, in
 *     n_outlier and in n_nonfinite, and in none of the sums or the max.
 *   epe_map: fp32 [N, D, H, W] (contiguous) or NULL: epe at EVERY element, valid or not; NaN where pred or gt is not
 *     finite.
 *   out: fp64 [N][FS_FLOW_METRICS_K], per flow, in this order (the noc entries over valid AND noc):
 *     0 n_valid   1 sum epe   2 sum epe^2   3 sum ae   4 n_outlier   5 max epe (-inf when no finite valid element)
 *     6 n_noc     7 sum epe   8 sum epe^2   9 sum ae  10 n_outlier
 *    11 n_nonfinite (valid)  12 n_nonfinite (valid and noc)
 *     Means are over the finite elements (n - n_nonfinite), Fl = n_outlier / n; occluded = valid minus noc.
 *   Per-workgroup fp64 partials in `ws` (fs_flow_metrics{2,3}d_ws_bytes bytes, 8-byte aligned), summed by a second
 *   launch in a fixed order: bitwise reproducible, no atomics.
 *   FS_ERR_SHAPE: N < 1, C other than 2 (2-D) / 3 (3-D), an extent < 1 (< 2 under RIFE3D), a batch stride below
 *   C*D*H*W; FS_ERR_ARG: an unknown convention, tau_abs or tau_rel negative or not finite.
 *   The _ws_bytes queries launch nothing and return the byte count or -(FS_ERR_*).
 */
#define FS_FLOW_METRICS_K 13
#define FS_FM_MAX_EPE 5
enum { FS_FLOW_DISP = 0, FS_FLOW_RIFE3D = 1 };
long long fs_flow_metrics2d_ws_bytes(int N, int C, int H, int W);
long long fs_flow_metrics3d_ws_bytes(int N, int C, int D, int H, int W, int convention);
int fs_flow_metrics2d(const float* pred, const float* gt, int N, int C, int H, int W, long long pred_bstride,
                      long long gt_bstride, const unsigned char* valid, const unsigned char* noc, float tau_abs,
                      float tau_rel, float* epe_map, double* ws, double* out, fs_stream_t stream);
int fs_flow_metrics3d(const float* pred, const float* gt, int N, int C, int D, int H, int W, long long pred_bstride,
                      long long gt_bstride, const unsigned char* valid, const unsigned char* noc, int convention,
                      float tau_abs, float tau_rel, float* epe_map, double* ws, double* out, fs_stream_t stream);

/* ------------------------------------------------------------------------------------
 * The fp64 sample of a step flow -- the one rule by which fs_flow_consistency*, fs_advect* and fs_lic* read a field (or
 * an image or texture plane) at a point and decide whether a point is on the grid (csrc/trilinear64.hpp); fs_streamlines*
 * samples by it too.  S = (W, H, D)
 * nodes per axis (2-D: D = 1), points of C components (x, y[, z]) in elements; fp64 without fused multiply-adds:
 *   classify(p): any p_c not finite: non-finite.  Else p_c < 0 or p_c > S_c - 1 for some c: outside (the border is
 *     inclusive; an extent of 1 is legal).  Else on the grid.
 *   sample(q): any q_c not finite -> every value NaN (no index is formed).  Else q_c = min(max(q_c, 0), S_c - 1) (nothing
 *     to do for a point that classify found on the grid), i0 = floor(q_c), f_c = q_c - i0, g_c = 1 - f_c,
 *     i1 = min(i0 + 1, S_c - 1); the corner with bits (bz, by, bx) weighs (tz * ty) * tx (2-D: ty * tx), t = f where the
 *     bit is set, else g; the sum over the corners in ascending 4 bz + 2 by + bx, from 0.0, of weight * plane[corner],
 *     every product formed (a non-finite corner of weight 0 gives NaN).
 */

/* ------------------------------------------------------------------------------------
 * Forward-backward consistency -- the label-free quality measure of a flow: N pairs of displacements, one launch.
 *   flow_f, flow_b: N flows of C fp32 planes of D*H*W (2-D: D = 1, C = 2; 3-D: C = 3) elements each, laid out and
 *     strided exactly as fs_flow_metrics*'s operands (planes of one flow contiguous, flow n at + n * bstride elements,
 *     bstride >= C*D*H*W when N > 1; channel 0 along W, 1 along H, 2 along D, in elements).  flow_f maps frame a to
 *     frame b on a's grid, flow_b maps b to a on b's grid.
 *   img0, img1: fp32 [N, D, H, W] (contiguous) frames a and b, both or neither (NULL).
 *   valid: uint8 [N, D, H, W] (contiguous, nonzero = set) or NULL = every element is valid.
 *   Per element x, in fp64 without fused multiply-adds (a restatement with the same operations in the same order
 *   reproduces every count exactly):
 *     p_c = x_c + flow_f_c(x).  A non-finite flow_f_c(x): NONFINITE.  Else classify(p) outside: OUTGOING.  Else
 *     Fbw_c = sample(p) of flow_b_c and I1w = sample(p) of img1 ("The fp64 sample of a step flow" above).
 *     r2 = sum_c (flow_f_c + Fbw_c)^2, m2 = sum_c flow_f_c^2 + sum_c Fbw_c^2 (each sum in ascending c from 0.0),
 *     r = sqrt(r2), e = I1w - img0(x).  Fbw, or with images img0(x) or I1w, not finite: NONFINITE.  Else
 *     OCCLUDED when r2 > alpha1 * m2 + alpha2 (UnFlow: 0.01, 0.5), CONSISTENT otherwise.  inside = OCCLUDED + CONSISTENT.
 *   out: fp64 [N][FS_FLOW_CONSISTENCY_K], over the elements with `valid` set:
 *     0 n_valid   1 n_nonfinite   2 n_outgoing   3 n_occluded   4 n_consistent
 *     5 sum r (inside)   6 sum r2 (inside)   7 max r (inside; -inf when none)   8 sum r (consistent)
 *     9 sum |e| (inside)  10 sum e^2 (inside)  11 sum |e| (consistent)  12 sum e^2 (consistent)   (9-12: 0 without images)
 *   class_map: uint8 [N, D, H, W] or NULL: 0 where valid is not set, else the FS_FC_* class.
 *   res_map: fp32 [N, D, H, W] or NULL: r at EVERY element, valid or not; NaN where it is outgoing or nonfinite.
 *   Per-workgroup fp64 partials in `ws` (fs_flow_consistency{2,3}d_ws_bytes bytes, 8-byte aligned), summed by a second
 *   launch in a fixed order: bitwise reproducible, no atomics.
 *   FS_ERR_NULLPTR: flow_f, flow_b, ws or out NULL.  FS_ERR_SHAPE: N < 1, C other than 2 (2-D) / 3 (3-D), an extent
 *   < 1, a batch stride below C*D*H*W.  FS_ERR_ARG: alpha1 or alpha2 negative or not finite, exactly one image given.
 *   All of them are returned before anything is launched.  The _ws_bytes queries launch nothing and return the byte
 *   count or -(FS_ERR_*).
 */
#define FS_FLOW_CONSISTENCY_K 13
#define FS_FC_MAX_R 7
enum { FS_FC_NOT_VALID = 0, FS_FC_CONSISTENT = 1, FS_FC_OCCLUDED = 2, FS_FC_OUTGOING = 3, FS_FC_NONFINITE = 4 };
long long fs_flow_consistency2d_ws_bytes(int N, int C, int H, int W);
long long fs_flow_consistency3d_ws_bytes(int N, int C, int D, int H, int W);
int fs_flow_consistency2d(const float* flow_f, const float* flow_b, int N, int C, int H, int W, long long f_bstride,
                          long long b_bstride, const float* img0, const float* img1, const unsigned char* valid,
                          double alpha1, double alpha2, unsigned char* class_map, float* res_map, double* ws,
                          double* out, fs_stream_t stream);
int fs_flow_consistency3d(const float* flow_f, const float* flow_b, int N, int C, int D, int H, int W,
                          long long f_bstride, long long b_bstride, const float* img0, const float* img1,
                          const unsigned char* valid, double alpha1, double alpha2, unsigned char* class_map,
                          float* res_map, double* ws, double* out, fs_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Pathlines -- P particles moved through K consecutive displacement fields, one launch.
 *   flows: K fields of C fp32 planes of D*H*W elements (2-D: D = 1, C = 2; 3-D: C = 3), planes of one field contiguous,
 *     field k at + k * flow_sstride elements (flow_sstride >= C*D*H*W when K > 1); channel 0 along W, 1 along H, 2 along
 *     D, in elements.  Field k is the displacement over time step k on that step's grid.
 *   pos_in: fp32 [C][P], component c at + c * pos_cstride (>= P); component 0 is x (along W).
 *   traj: fp32 [K][C][P], step k at + k * traj_sstride (>= P when K > 1), component c at + c * traj_cstride (>= P): the
 *     position after step k goes to slot k.  traj_sstride = 0 keeps the last position only (a particle's stores go out
 *     in step order to the one slot).  Slot K-1 may be pos_in's memory (same pointer and component stride): a
 *     particle's pos_in is read once, before any store, and no thread touches another particle's elements.
 *   status: uint8 [P], in / out, FS_ADV_ALIVE / FS_ADV_OUT / FS_ADV_NONFINITE.  steps: int32 [P], in / out, or NULL: the
 *     number of steps after which the particle was still ALIVE is added.
 *   method: FS_ADV_EULER, FS_ADV_RK2 (midpoint) or FS_ADV_RK4; substeps S >= 1; hs = scale / S, 0.5 * hs and hs / 6.0
 *     are formed on the host in fp64 (scale = -1 with the opposite flows traces backward in time).
 *   Per particle, in fp64 without fused multiply-adds (a restatement with the same operations in the same order
 *   reproduces every output bit, status and count):
 *     sample(k, q): the sample of "The fp64 sample of a step flow" above on the C planes of field k, the clamp included.
 *     classify(p): that section's: non-finite is NONFINITE, outside is OUT (the border is inside), on the grid is ALIVE.
 *     Step k: the fp32 position (pos_in at k = 0, the previous step's result later) is widened; an ALIVE particle is
 *       classified (a seed outside the box or a non-finite seed ends here without moving).  For s in 0..S-1 while ALIVE,
 *       with k1 = sample(k, p): Euler p' = p + hs k1; RK2 k2 = sample(p + (0.5 hs) k1), p' = p + hs k2; RK4 the classical
 *       stages k2 = sample(p + (0.5 hs) k1), k3 = sample(p + (0.5 hs) k2), k4 = sample(p + hs k3),
 *       p' = p + (hs / 6) (((k1 + 2 k2) + 2 k3) + k4).  Stage points are clamped by sample and never classified.
 *       classify(p'): NONFINITE keeps p; OUT takes p' (the exit point); ALIVE takes p'.  After the substeps an ALIVE
 *       particle's `steps` grows by one; the position is rounded to fp32 once and stored in slot k; the next step starts
 *       from the rounded value, so K steps in one launch equal K launches of one step bit for bit.  A particle that is
 *       not ALIVE (on entry too) copies its position to every remaining slot.
 *   FS_ERR_NULLPTR: flows, pos_in, traj or status NULL.  FS_ERR_SHAPE: K < 1, P < 1, C other than 2 (2-D) / 3 (3-D), an
 *   extent < 1, a stride below its minimum.  FS_ERR_ARG: substeps < 1, an unknown method, scale not finite.  All of them
 *   are returned before anything is launched.
 */
enum { FS_ADV_ALIVE = 0, FS_ADV_OUT = 1, FS_ADV_NONFINITE = 2 };
enum { FS_ADV_EULER = 0, FS_ADV_RK2 = 1, FS_ADV_RK4 = 2 };
int fs_advect2d(const float* flows, int K, int C, int H, int W, long long flow_sstride, const float* pos_in,
                long long pos_cstride, long long P, float* traj, long long traj_sstride, long long traj_cstride,
                unsigned char* status, int* steps, int method, int substeps, double scale, fs_stream_t stream);
int fs_advect3d(const float* flows, int K, int C, int D, int H, int W, long long flow_sstride, const float* pos_in,
                long long pos_cstride, long long P, float* traj, long long traj_sstride, long long traj_cstride,
                unsigned char* status, int* steps, int method, int substeps, double scale, fs_stream_t stream);

/* ------------------------------------------------------------------------------------
 * FTLE -- the finite-time Lyapunov exponent of a flow map sampled on a lattice, one launch (plus the summary's).
 *   map: fp32 [C][Gd*Gh*Gw], component c at + c * map_cstride (>= Gd*Gh*Gw) elements, node (z, y, x) at
 *     (z * Gh + y) * Gw + x (x fastest): the end positions fs_advect* returns for lattice seeds.  2-D: Gd = 1, C = 2;
 *     3-D: C = 3.  Component 0 and axis 0 run along x.
 *   status: uint8 [Gd*Gh*Gw], the FS_ADV_* of fs_advect*.  valid: uint8 [Gd*Gh*Gw] (nonzero = set) or NULL = every node.
 *   inv_h, inv_2h: HOST arrays of C doubles, 1 / h_c and 1 / (2 h_c) with h_c the seed spacing along axis c in elements;
 *     inv_T = 1 / |integration time|.  The host forms them in fp64; the device divides nothing by them.
 *   Per node, in fp64 without fused multiply-adds up to and including G (a restatement with the same operations in the
 *   same order reproduces every class and every bit of cg):
 *     usable(j): status[j] == FS_ADV_ALIVE, or FS_ADV_OUT when accept_out != 0 (the exit point stands for the end
 *       position).
 *     The difference along axis c at index i is the first that applies of: central, i-1 and i+1 exist and are usable
 *       (the node's own state does not matter): (phi(i+1) - phi(i-1)) * inv_2h[c]; forward, i and i+1 usable:
 *       (phi(i+1) - phi(i)) * inv_h[c]; backward, i and i-1 usable: (phi(i) - phi(i-1)) * inv_h[c].  None along some axis:
 *       FS_FTLE_ENDED.  Map values are widened to fp64 before the subtraction; nothing is read from a node that is not
 *       usable (its map values may be anything).
 *     J[r][c] = the difference of component r along axis c.  Any J[r][c] not finite (a used map value was not):
 *       FS_FTLE_NONFINITE.
 *     G[a][b] = (J[0][a] J[0][b] + J[1][a] J[1][b]) + J[2][a] J[2][b] (2-D: the first two terms), the Cauchy-Green tensor.
 *     lambda = its largest eigenvalue: in 2-D 0.5 (G00 + G11) + sqrt((0.5 (G00 - G11))^2 + G01^2), in 3-D by cyclic
 *       Jacobi rotations on G scaled by a power of two, until the off-diagonal entries sum to less than 2^-45 of the
 *       scaled trace's upper bound (relative error of lambda below 2e-13; a diagonal G gives its largest entry exactly).
 *     lambda == 0: FS_FTLE_COLLAPSED (the lattice cell mapped to a point).  Else e = (0.5 * log(lambda)) * inv_T, rounded
 *       to fp32 once; e not finite: FS_FTLE_NONFINITE; else FS_FTLE_OK.
 *   ftle: fp32 [Gd*Gh*Gw]: e where the class is FS_FTLE_OK, NaN elsewhere.  cls: uint8 [Gd*Gh*Gw]: FS_FTLE_NOT_VALID where
 *     valid is not set, else the class.
 *   cg: fp32 [C(C+1)/2][Gd*Gh*Gw] or NULL: G's entries in the plane order xx, xy, yy, xz, yz, zz, each rounded once; NaN at
 *     nodes that are neither OK nor COLLAPSED.
 *   out: fp64 [FS_FTLE_K] or NULL: 0-4 the number of nodes of class 0-4; 5 the sum, 6 the sum of squares, 7 the minimum
 *     (+inf when none) and 8 the maximum (-inf when none) of the STORED fp32 ftle over the OK nodes.  Per-workgroup fp64
 *     partials in `ws` (fs_ftle{2,3}d_ws_bytes bytes, 8-byte aligned; needed only with out), combined by a second launch
 *     in a fixed order: bitwise reproducible, no atomics.
 *   FS_ERR_NULLPTR: map, status, inv_h, inv_2h, ftle or cls NULL, or out without ws.  FS_ERR_SHAPE: C other than 2 (2-D) /
 *   3 (3-D), a lattice extent below 2 along an axis C covers, more than 2^31 - 1 nodes, map_cstride below the node count.
 *   FS_ERR_ARG: an inv_h[c], inv_2h[c] or inv_T that is not finite or not positive.  All of them are returned before
 *   anything is launched.  The _ws_bytes queries launch nothing and return the byte count or -(FS_ERR_*).
 */
#define FS_FTLE_K 9
#define FS_FTLE_MIN 7
#define FS_FTLE_MAX 8
enum { FS_FTLE_NOT_VALID = 0, FS_FTLE_OK = 1, FS_FTLE_ENDED = 2, FS_FTLE_NONFINITE = 3, FS_FTLE_COLLAPSED = 4 };
long long fs_ftle2d_ws_bytes(int C, int Gh, int Gw);
long long fs_ftle3d_ws_bytes(int C, int Gd, int Gh, int Gw);
int fs_ftle2d(const float* map, long long map_cstride, const unsigned char* status, const unsigned char* valid, int C,
              int Gh, int Gw, const double* inv_h, const double* inv_2h, double inv_T, int accept_out, float* ftle,
              unsigned char* cls, float* cg, double* ws, double* out, fs_stream_t stream);
int fs_ftle3d(const float* map, long long map_cstride, const unsigned char* status, const unsigned char* valid, int C,
              int Gd, int Gh, int Gw, const double* inv_h, const double* inv_2h, double inv_T, int accept_out,
              float* ftle, unsigned char* cls, float* cg, double* ws, double* out, fs_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Velocity gradient -- divergence, vorticity, the Q criterion and lambda2 of K step flows, one launch (plus the
 * summary's).
 *   flows: K fields of C fp32 planes of D*H*W elements (2-D: D = 1, C = 2; 3-D: C = 3), planes of one field contiguous,
 *     field k at + k * flow_sstride elements (>= C*D*H*W: every other field of a stack is read in place), node (z, y, x)
 *     at (z * H + y) * W + x; displacements in elements, component 0 and axis 0 along x (W), 1 along y, 2 along z.
 *   inv_h, inv_2h: HOST arrays of C doubles, 1 / h_c and 1 / (2 h_c) with h_c the node spacing along axis c.  scale: HOST
 *     array of K doubles, the reciprocal of the time step k spans: velocity = displacement * scale[k].  The host forms
 *     them in fp64 and the device divides nothing by them; the scales travel in the launch's arguments (steps beyond
 *     FS_VG_STEPS_PER_LAUNCH = 256 go out in further launches of the same call).
 *   fields: a bitmask of FS_VG_DIV, FS_VG_VORT, FS_VG_VMAG, FS_VG_Q, FS_VG_L2, FS_VG_J; NP = the number of planes it
 *     selects, in this order: div (1), vort (2-D: 1, 3-D: 3), vmag (1), q (1), l2 (1), J (C*C, plane r * C + c).
 *   Per node, in fp64 without fused multiply-adds (a restatement with the same operations in the same order reproduces
 *   every bit of div, vort, q and J; tests/velgrad_ref.py):
 *     The difference along axis c at index i: central where i-1 and i+1 exist, lo = i-1, hi = i+1, w = inv_2h[c]; else
 *       forward where i+1 exists, lo = i, hi = i+1, w = inv_h[c]; else backward, lo = i-1, hi = i, w = inv_h[c].
 *     J[r][c] = (((double)u_r[hi] - (double)u_r[lo]) * w) * scale[k]     (all C*C entries, whatever is selected)
 *     div = (J00 + J11) + J22                                              (2-D: J00 + J11)
 *     vort = (J21 - J12, J02 - J20, J10 - J01)                             (2-D: the scalar J10 - J01)
 *     vmag = sqrt((vort0^2 + vort1^2) + vort2^2)                           (2-D: |vort|)
 *     s_aa = J_aa; for a < b: s_ab = 0.5 (J_ab + J_ba), o_ab = 0.5 (J_ab - J_ba)      (S and Omega)
 *     nS = ((s00^2 + s11^2) + s22^2) + 2 ((s01^2 + s02^2) + s12^2)          (2-D: (s00^2 + s11^2) + 2 s01^2)
 *     nO = 2 ((o01^2 + o02^2) + o12^2)                                      (2-D: 2 o01^2)
 *     q = 0.5 (nO - nS)
 *     M = S^2 + Omega^2 (symmetric):
 *       m00 = ((s00^2 + s01^2) + s02^2) - (o01^2 + o02^2)     m01 = ((s00 s01 + s01 s11) + s02 s12) - o02 o12
 *       m11 = ((s01^2 + s11^2) + s12^2) - (o01^2 + o12^2)     m02 = ((s00 s02 + s01 s12) + s02 s22) + o01 o12
 *       m22 = ((s02^2 + s12^2) + s22^2) - (o02^2 + o12^2)     m12 = ((s01 s02 + s11 s12) + s12 s22) - o01 o02
 *       (2-D: m00 = (s00^2 + s01^2) - o01^2, m11 = (s01^2 + s11^2) - o01^2, m01 = s00 s01 + s01 s11)
 *     l2 = the median eigenvalue of M.  3-D: cyclic Jacobi rotations on M scaled by the power of two that brings its
 *       largest entry magnitude into [0.5, 1), until the off-diagonal entries sum to at most 2^-45 (at most 10 sweeps),
 *       then the median of the three diagonal entries, scaled back: every eigenvalue is within 2^-44 ||M||_F of one of
 *       them, and a diagonal M comes back untouched (a constant field gives exactly 0, a rigid rotation exactly
 *       -|rate|^2).  2-D: the median of 0 and the two eigenvalues 0.5 (m00 + m11) -+ sqrt((0.5 (m00 - m11))^2 + m01^2) --
 *       the planar field embedded in 3-D.  trace M = -2 q.
 *     Each selected value is rounded to fp32 once.  The node is NOT FINITE when an entry of J or a selected value (after
 *     its rounding) is not finite; every selected plane of the node is then NaN.
 *   out: fp32 [K][NP][D*H*W], contiguous.
 *   flags: uint8 [K][D*H*W] or NULL.  bit 0: q is selected and the stored q > 0; bit 1: l2 is selected and the stored
 *     l2 < 0; bit 7: the node is not finite (bits 0-1 are then clear).
 *   summary: fp64 [K][FS_VG_K] or NULL, per step: 0 the nodes that are not finite, 1 those with bit 0, 2 those with bit 1,
 *     3 those with both; then for each of div, vmag, q, l2 (in this order, at 4 + 4 n) the sum, the sum of squares, the
 *     minimum (+inf when none) and the maximum (-inf when none) of the STORED fp32 values over the finite nodes.  What
 *     depends on a field that is not selected is NaN.  Per-workgroup fp64 partials in `ws` (fs_velgrad{2,3}d_ws_bytes
 *     bytes, 8-byte aligned; needed only with summary), combined by a second launch in a fixed order: bitwise
 *     reproducible, no atomics; step k's numbers do not depend on K.
 *   FS_ERR_NULLPTR: flows, inv_h, inv_2h, scale or out NULL, or summary without ws.  FS_ERR_SHAPE: C other than 2 (2-D) /
 *   3 (3-D), an extent below 2, more than 2^31 - 1 nodes, flow_sstride below C*D*H*W.  FS_ERR_ARG: fields empty or with
 *   unknown bits, K < 1, an inv_h[c], inv_2h[c] or scale[k] that is not finite or not positive.  All of them are returned
 *   before anything is launched.  The _ws_bytes queries launch nothing and return the byte count or -(FS_ERR_*).
 */
enum { FS_VG_DIV = 1, FS_VG_VORT = 2, FS_VG_VMAG = 4, FS_VG_Q = 8, FS_VG_L2 = 16, FS_VG_J = 32, FS_VG_ALL = 63 };
enum { FS_VG_FLAG_Q = 1, FS_VG_FLAG_L2 = 2, FS_VG_FLAG_NONFINITE = 128 };
#define FS_VG_K 20
#define FS_VG_STEPS_PER_LAUNCH 256
long long fs_velgrad2d_ws_bytes(int K, int C, int H, int W);
long long fs_velgrad3d_ws_bytes(int K, int C, int D, int H, int W);
int fs_velgrad2d(const float* flows, int K, int C, int H, int W, long long flow_sstride, const double* inv_h,
                 const double* inv_2h, const double* scale, unsigned fields, float* out, unsigned char* flags,
                 double* ws, double* summary, fs_stream_t stream);
int fs_velgrad3d(const float* flows, int K, int C, int D, int H, int W, long long flow_sstride, const double* inv_h,
                 const double* inv_2h, const double* scale, unsigned fields, float* out, unsigned char* flags,
                 double* ws, double* summary, fs_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Regions -- connected components of K flag maps, one table row per region, and the label every foreground node is
 * carried onto by the step flow to the next map.  Node (z, y, x) of a step at (z * H + y) * W + x (2-D: D = 1); a step
 * holds fewer than 2^31 - 1 nodes, every extent >= 1 (FS_ERR_SHAPE otherwise).
 *
 * fs_label_regions{2,3}d
 *   mask: uint8, step k at + k * mask_sstride elements (>= D*H*W: every other map of a stack is read in place).  A node
 *     is FOREGROUND iff (m & require) == require && (m & reject) == 0  (require, reject in 0..255).
 *   conn: 0 = face neighbours (4 / 6), 1 = the full neighbourhood (8 / 26); anything else FS_ERR_ARG.
 *   labels: int32 [K][D*H*W].  Background 0; a foreground node's label is 1 + the smallest linear index, within its own
 *     step, of any node of its component.  Components never join across steps.  The definition does not depend on the
 *     order of merges: the result is bitwise reproducible.
 *   n_regions: int32 [K], the nodes of step k with labels == index + 1.  status: int32 [1], 0, or bit 0 set when a
 *     find / union loop ran into its iteration cap (it cannot while parents strictly decrease; the cap keeps a bug from
 *     spinning).  Both are zeroed by the call.
 *   ws: fs_label_regions{2,3}d_ws_bytes bytes (the int32 parent array).
 *   Three launches per FS_REGION_STEPS_PER_LAUNCH steps: tiles of FS_REGION_TILE* nodes are labelled in LDS by union-find
 *   (parent < child); foreground nodes on tile faces unite with their earlier neighbours in other tiles through
 *   agent-scope atomics (relaxed load, fetch-min) only; every node follows its parents and writes root + 1 to `labels`.
 *   FS_ERR_NULLPTR: any pointer NULL.  FS_ERR_ARG: conn, K < 1, require / reject outside 0..255.
 *
 * fs_region_stats{2,3}d
 *   labels as above (K <= FS_REGION_STEPS_PER_LAUNCH); rank: int32 [K][D*H*W], at the root node of a region (index
 *   label - 1) its dense id within the step, 0 .. R_k - 1, in increasing label order; offsets: int64 [K+1] in DEVICE
 *   memory, the prefix sums of R_k; R = offsets[K].  weights: fp32 [K][F][D*H*W] or NULL with F = 0; F <= 8.
 *   Row offsets[k] + rank of every region:  count int64 [R];  coord_sum int64 [R][nd], the sums of the integer node
 *   coordinates in the tensor's axis order ((z,) y, x);  bbox int32 [R][2][nd], inclusive minimum and maximum;  with
 *   weights wsum fp64 [R][F] (fp64 atomic adds: the order is not fixed, the error is bounded by (n - 1) 2^-53 sum |w|),
 *   wmin / wmax fp32 [R][F] (exact; reduced throughout as the order-preserving integer image of fp32, in which -0 < +0).  All outputs are initialised by the call.  A node whose label, rank or offsets do
 *   not name a row of the table is skipped, never written through.  Weights must be finite on foreground nodes (not
 *   checked).  Runs of equal row along x are reduced in the wave before one lane issues the run's atomics.
 *   FS_ERR_ARG: K, F, R out of range.  R == 0: nothing launched.
 *
 * fs_region_follow{2,3}d
 *   labels int32 [K][D*H*W], K >= 2; flows: fp32, step j at + j * flow_sstride elements (>= C*D*H*W), C planes, component
 *   0 along x (W); flow j lives on the grid of map j and points to map j + 1.  dst: int32 [K-1][D*H*W]:
 *     0 where labels[j][x] == 0; else per axis a  r_a = rintf((float)x_a + u_a(x))  (one fp32 add, round half to even);
 *     FS_REGION_OUT where some axis fails r_a >= 0 && r_a <= extent_a - 1 (compared as floats: NaN, +-inf and 1e30 fail);
 *     else L = labels[j+1][r]: L where L > 0, FS_REGION_TO_BACKGROUND otherwise.
 *   FS_ERR_SHAPE: C other than 2 (2-D) / 3 (3-D), flow_sstride below C*D*H*W, an extent above
 *   FS_REGION_FOLLOW_MAX_EXTENT = 2^24 (beyond it extent - 1 need not be a float and the range test would not be exact).
 *   FS_ERR_ARG: K < 2.
 * All validation happens before anything is launched; the _ws_bytes queries launch nothing and return the byte count or
 * -(FS_ERR_*).
 */
#define FS_REGION_TILE2_H 32
#define FS_REGION_TILE2_W 64
#define FS_REGION_TILE3_D 8
#define FS_REGION_TILE3_H 8
#define FS_REGION_TILE3_W 32
#define FS_REGION_MAX_WEIGHTS 8
#define FS_REGION_STEPS_PER_LAUNCH 32768
#define FS_REGION_FOLLOW_MAX_EXTENT 16777216
enum { FS_REGION_OUT = -1, FS_REGION_TO_BACKGROUND = -2 };
long long fs_label_regions2d_ws_bytes(int K, int H, int W);
long long fs_label_regions3d_ws_bytes(int K, int D, int H, int W);
int fs_label_regions2d(const unsigned char* mask, int K, int H, int W, long long mask_sstride, int require, int reject,
                       int conn, int* labels, int* n_regions, int* status, int* ws, fs_stream_t stream);
int fs_label_regions3d(const unsigned char* mask, int K, int D, int H, int W, long long mask_sstride, int require,
                       int reject, int conn, int* labels, int* n_regions, int* status, int* ws, fs_stream_t stream);
int fs_region_stats2d(const int* labels, const int* rank, const long long* offsets, const float* weights, int K, int F,
                      int H, int W, long long R, long long* count, long long* coord_sum, int* bbox, double* wsum,
                      float* wmin, float* wmax, fs_stream_t stream);
int fs_region_stats3d(const int* labels, const int* rank, const long long* offsets, const float* weights, int K, int F,
                      int D, int H, int W, long long R, long long* count, long long* coord_sum, int* bbox, double* wsum,
                      float* wmin, float* wmax, fs_stream_t stream);
int fs_region_follow2d(const int* labels, const float* flows, int K, int C, int H, int W, long long flow_sstride,
                       int* dst, fs_stream_t stream);
int fs_region_follow3d(const int* labels, const float* flows, int K, int C, int D, int H, int W, long long flow_sstride,
                       int* dst, fs_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Ray casting -- K volumes through K cameras and one transfer function to K RGBA images, one launch (two with bricks).
 *   volumes: K fp32 volumes of D*H*W nodes, node (z, y, x) at (z * H + y) * W + x, volume k at + k * sstride elements
 *     (>= D*H*W: every other volume of a stack is read in place); every extent >= 2.  Axis 0 runs along x (W), 1 along
 *     y, 2 along z; spacing: HOST array of 3 doubles, the node spacing along x, y, z; node i of axis a sits at i * h_a.
 *   cameras: fp32 [K][18] in DEVICE memory, the 3-vectors o, ou, ov, d, du, dv in (x, y, z).  Pixel (i, j) -- column i
 *     of row j of the image -- has the origin o + i ou + j ov and the direction normalize(d + i du + j dv)
 *     (orthographic: du = dv = 0; perspective: ou = ov = 0).
 *   tf: fp32 [n][4] RGBA in DEVICE memory, 16-byte aligned, 2 <= n <= FS_RC_MAX_TF, spread uniformly over [lo, hi];
 *     finite, A >= 0 (not checked).
 *   Per pixel, in fp32; the lines marked * without fused multiply-adds, in exactly this order, so that a restatement
 *   (tests/raycast_ref.py) picks the same cell for every sample:
 *   * O = (o + i ou) + j ov;  g = (d + i du) + j dv;  dir = g / sqrt((g_x^2 + g_y^2) + g_z^2)
 *   * sample k = 0, 1, ...:  t = (k + 0.5) dt;  q_a = (O_a + t dir_a) * ih_a,  ih_a = fp32(1 / h_a)     (index position)
 *     coverage  c = (c_x c_y) c_z,  c_a = max(0, 1 - max(0, max(-q_a, q_a - (N_a - 1))))
 *     value     v = the trilinear sample at qc = min(max(q, 0), N - 1): cell i_a = min(floor(qc_a), N_a - 2), weight
 *               f_a = qc_a - i_a; along x first (a + f_x (b - a)), then y, then z
 *     position  u = min(max((v - lo) * fp32(1 / (hi - lo)), 0), 1);  table(u): s = u (n - 1), j = min(floor(s), n - 2),
 *               row j + (s - j) (row j+1 - row j)
 *     a sample whose v is not finite (a corner of its cell is NaN or +-inf) contributes nothing.
 *     Every x + w (y - x) above (the interpolations, the table) and every C += w X below is one fused multiply-add;
 *     nothing else is fused, so that the kernel with and without the brick map rounds alike.
 *     FS_RC_DVR:  (R, G, B, A) = table(u);  e = exp(-((A c) dt));  C += T (1 - e) (R, G, B);  T *= e;  from C = 0, T = 1.
 *                 The pixel is (C, 1 - T).  The ray ends after the first sample that leaves T < t_min (0: never).
 *     FS_RC_MIP:  m = max(m, c u) from m = 0.  The pixel is table(m): a ray that meets nothing shows row 0.
 *   The samples do not depend on where a ray meets the box.  The kernel bounds k by a slab test against the box grown
 *   by one cell and a margin of 2^-15 of the coordinates' magnitude, plus one sample at either end; a sample outside
 *   weighs c = 0 and changes nothing, visited or not.  A direction component of exactly 0 is legal; a ray with an
 *   origin or direction that is not finite misses.  Sample indices end at 2^24 - 1.
 *   image: fp32 [K][Hi][Wi][4], 16-byte aligned.  counts: int32 [K][Hi][Wi] or NULL, the samples the pixel gathered.
 *
 * fs_brick_range3d
 *   Brick (bz, by, bx) holds the cells [8 b, 8 b + 8) of every axis, that is the nodes 8 b .. min(8 b + 8, N - 1);
 *   nb_a = ceil((N_a - 1) / 8).  range: fp32 [K][nbz][nby][nbx][2], the minimum and maximum over the brick's finite
 *   nodes (+inf, -inf when none); nonfinite: uint8 [K][nbz][nby][nbx], 1 when a node of the brick is NaN or +-inf.
 *   With brick_range, brick_nonfinite (both as written here) and ws (fs_raycast3d_ws_bytes bytes) fs_raycast3d first
 *   marks, in ws, the bricks no sample of which can contribute: none of its nodes is not finite and, for the range
 *   [mn, mx] widened by 2^-20 max(|mn|, |mx|) (more than three nested fp32 interpolations can leave it by; not at all when
 *   both are 0), in dvr A is 0
 *   in every table row the range touches and one more at either end, in mip mx <= lo.  A ray that samples a cell of
 *   such a brick jumps to the last sample it provably spends in the brick (faces pulled in by the margin above): it
 *   lands early, never late.  Every sample jumped over would have added exactly 0 (e = 1, or c u = 0): the image is the
 *   same bit for bit, only counts is smaller.
 *   FS_ERR_NULLPTR: volumes, cameras, tf, spacing or image NULL, brick_range without brick_nonfinite and ws.
 *   FS_ERR_SHAPE: K outside 1..65535, an extent below 2, more than 2^31 - 1 nodes, sstride below D*H*W, Hi or Wi outside
 *   1..16*65535, n outside 2..FS_RC_MAX_TF.  FS_ERR_ARG: an unknown mode, lo >= hi or not finite, dt or a spacing not
 *   finite and positive, t_min outside [0, 1), tf or image not 16-byte aligned, more than FS_RC_MAX_STEPS samples of dt
 *   along the grown box (sum_a (N_a + 1) h_a / dt).  All of them are returned before anything is launched; the
 *   _ws_bytes query launches nothing and returns the byte count or -(FS_ERR_*).
 */
enum { FS_RC_DVR = 0, FS_RC_MIP = 1 };
#define FS_RC_BRICK 8
#define FS_RC_MAX_TF 1024
#define FS_RC_MAX_STEPS 4194304
int fs_brick_range3d(const float* volumes, int K, int D, int H, int W, long long sstride, float* range,
                     unsigned char* nonfinite, fs_stream_t stream);
long long fs_raycast3d_ws_bytes(int K, int D, int H, int W);
int fs_raycast3d(const float* volumes, int K, int D, int H, int W, long long sstride, const float* cameras,
                 const float* tf, int n, double lo, double hi, double dt, const double* spacing, int mode, double t_min,
                 int Hi, int Wi, const float* brick_range, const unsigned char* brick_nonfinite, unsigned char* ws,
                 float* image, int* counts, fs_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Isosurfaces -- K volumes and one isovalue to K indexed, watertight, consistently oriented triangle meshes: marching
 * tetrahedra on the Kuhn split of every cell (no ambiguous cases; six corner lists and sixteen cases).
 *   volumes: K fp32 volumes of D*H*W nodes, node (z, y, x) at (z * H + y) * W + x, volume k at + k * sstride elements
 *     (>= D*H*W: every other volume of a stack is read in place); every extent >= 2.  Axis 0 runs along x (W), 1 along
 *     y, 2 along z; spacing: HOST array of 3 doubles, the node spacing along x, y, z, each rounded to fp32 once.
 *   iso is rounded to fp32 once.  A finite node is INSIDE iff f >= iso.
 *   Edges.  Every node owns up to 7 edges, to the node at offset (dz, dy, dx) where that node exists:
 *     e0 (0,0,1)  e1 (0,1,0)  e2 (1,0,0)  e3 (0,1,1)  e4 (1,0,1)  e5 (1,1,0)  e6 (1,1,1)
 *     An edge is ACTIVE iff both ends are finite and exactly one end is inside.  An active edge carries one vertex.
 *   Vertex position, in fp32 without fused multiply-adds, in exactly this order (a = the owner, b = the other end):
 *     t = min(max((iso - fa) / (fb - fa), 0), 1);  per axis r  q_r = (float)i_r + (d_r ? t : 0);  p_r = q_r * (float)h_r
 *     Vertices are stored as (x, y, z).  The vertices of a step are ordered by owner node index, then by edge number.
 *   Tetrahedra.  A cell (z, y, x), every coordinate below extent - 1, is cut into 6 tetrahedra, one per permutation pi
 *     of the axes (x = 0, y = 1, z = 2) in lexicographic order, with the corners c0 = the cell's origin node,
 *     c1 = c0 + e_pi0, c2 = c1 + e_pi1, c3 = c0 + (1,1,1).  A cell with a corner that is not finite emits nothing.
 *   Triangles of a tetrahedron; E(p,q) is the vertex on the edge between corners p and q (every such edge is one of
 *     e0..e6 of the corner with the lower number):
 *     0 or 4 corners inside: none.
 *     1 or 3 inside: s the odd corner, a < b < c the others: (E(s,a), E(s,b), E(s,c)).
 *     2 inside: i0 < i1 the inside corners, o0 < o1 the outside ones, q = (E(i0,o0), E(i0,o1), E(i1,o1), E(i1,o0)):
 *       (q0, q1, q2) and (q0, q2, q3).
 *     Orientation: the last two vertices of a triangle are swapped where needed so that, with every vertex moved to its
 *     edge's midpoint in index space, (v1 - v0) x (v2 - v0) has a positive dot product with (centroid of the outside
 *     corners - centroid of the inside corners): normals point towards lower values.  This depends on the case and the
 *     tetrahedron only (csrc/iso_tables.hpp, derived by scripts/gen_iso_tables.py).
 *   Faces are int32 vertex indices local to their step, ordered by cell index, then tetrahedron, then triangle.
 *   Normals (optional).  Node gradient G: per axis (f(i+1) - f(i-1)) / (2 h), on the boundary (f(i+1) - f(i)) / h and
 *     (f(i) - f(i-1)) / h.  G = Ga + t (Gb - Ga);  n = -G / |G|, or (0,0,0) where |G| is 0 or not finite.
 *   Values (optional).  F <= FS_ISO_MAX_VALUES planes of a second field, fp32 [K][F][D*H*W]:  w = wa + t (wb - wa).
 *     Fused multiply-adds are allowed in normals and values.
 *   The result is bitwise reproducible: no atomic decides a position or an order.
 *
 * fs_iso_count3d -- one launch.  ws: fs_iso3d_ws_bytes bytes, 4-byte aligned, written as
 *     int32 nv[K*D*H], int32 nt[K*D*H]: per row (k, z, y) the vertices its nodes own and the triangles its cells emit;
 *     padding to a multiple of 16 bytes;  uint8 mask[K][D*H*W]: bit e of a node's byte = its edge e is active.
 * The caller turns nv and nt into row_offsets, int64 [2][K*D*H + 1] in DEVICE memory: the exclusive prefix sums of nv,
 *   then of nt, over all rows, each with the total at the end.  V and T are those totals.  (Step k's vertices are
 *   row_offsets[0][k*D*H] .. row_offsets[0][(k+1)*D*H].)
 * fs_iso_emit3d -- one launch (none when V and T are 0).  It recomputes every row's in-row prefix from the masks; a
 *   vertex is row (row offset of the owner's row + in-row prefix at the owner + rank of the edge within the owner's
 *   mask) of vertices [V][3], normals [V][3] (NULL: not wanted) and values_out [V][F]; faces is int32 [T][3].  Nothing is
 *   written at or beyond row V or T.  status: int32 [1], zeroed by the CALLER; bit 0 is set when the masks and the
 *   offsets disagree (a row's counts, an index outside its step) -- the outputs are then not a mesh.
 *   FS_ERR_NULLPTR: volumes, spacing, ws, row_offsets or status NULL; vertices with V > 0, faces with T > 0, values with
 *   F > 0, values_out with F > 0 and V > 0.  FS_ERR_SHAPE: K < 1 or K*D*H above 2^31 - 1, an extent below 2, more than
 *   2^31 - 1 nodes, sstride below D*H*W, F outside 0..FS_ISO_MAX_VALUES.  FS_ERR_ARG: iso not finite (as fp32), a spacing
 *   not finite and positive (as fp32), V or T negative, ws not 4-byte aligned.  All of them are returned before anything is
 *   launched; the _ws_bytes query launches nothing and returns the byte count or -(FS_ERR_*).
 */
#define FS_ISO_MAX_VALUES 8
long long fs_iso3d_ws_bytes(int K, int D, int H, int W);
int fs_iso_count3d(const float* volumes, int K, int D, int H, int W, long long sstride, double iso, unsigned char* ws,
                   fs_stream_t stream);
int fs_iso_emit3d(const float* volumes, int K, int D, int H, int W, long long sstride, double iso, const double* spacing,
                  const unsigned char* ws, const long long* row_offsets, long long V, long long T, const float* values,
                  int F, float* vertices, float* normals, float* values_out, int* faces, int* status, fs_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Line integral convolution -- every node's value is a texture averaged along the streamline of the normalised field
 * through that node, L steps of length h each way; K fields and both directions in one call (a streaming pre-pass that
 * packs field and texture into 16-byte elements, then one launch for all the lines).
 *   flows: as for fs_advect*: K fields of C fp32 planes of D*H*W elements (2-D: D = 1, C = 2; 3-D: C = 3), field k at
 *     + k * flow_sstride elements (flow_sstride >= C*D*H*W when K > 1); channel 0 along W.  Each field is steady.
 *   tex: one fp32 plane of D*H*W elements per step, step k at + k * tex_sstride (>= D*H*W when K > 1), or
 *     tex_sstride = 0: one texture shared by all K steps.
 *   weights: fp64 [L+1] in DEVICE memory: w[0] for the node, w[i] for the i-th sample on either side.  Precondition (the
 *     library cannot read them): all finite, w[0] > 0, the others >= 0.
 *   L: 0 .. FS_LIC_MAX_L steps each way.  h: the step length in elements, finite and > 0.  vmin: finite and >= 0.
 *   method: FS_ADV_EULER or FS_ADV_RK2 (midpoint).
 *   out: fp32 [K][D*H*W], contiguous.  ends: uint8 [K][D*H*W] or NULL.  count: int32 [K][D*H*W] or NULL.
 *   ws: fs_lic{2,3}d_ws_bytes(K, ...) bytes (16 per node and step), 16-byte aligned: the packed image (v_x, v_y[, v_z],
 *     tex) the lines are sampled from, written by the call before it is read.  It holds nothing afterwards.
 *   Per node, in fp64 without fused multiply-adds; square root and division are correctly rounded (nothing is
 *   multiplied by a reciprocal); positions stay fp64 for the whole line (a restatement with the same operations in the
 *   same order reproduces every output bit, end code and count):
 *     sample(k, q), classify(p): those of fs_advect* ("The fp64 sample of a step flow" above), the clamp included.
 *     dir(k, q): v = sample(k, q).  Any v_c not finite: NONFINITE.  n2 = (v0*v0 + v1*v1) + v2*v2 (2-D: no third term),
 *       n = sqrt(n2).  !(n > vmin): STAGNANT.  Else d_c = v_c / n.
 *     tsample(k, q): sample's clamp, corner and weight rule on the step's one texture plane, every product formed (a
 *       non-finite texture value propagates, also through a weight of 0).
 *     One side, for s = +1 and then s = -1, with hs = s * h and hh = 0.5 * hs formed on the host: p = the node's integer
 *       coordinates, A = 0.0, Wt = 0.0, n = 0, end = FULL.  For i = 1 .. L:
 *         d = dir(k, p); a code ends the side with that code.  RK2 only: d = dir(k, p + hh * d); likewise.
 *         p' = p + hs * d.  classify(p') not ALIVE: the side ends with OUT; the exit point is not sampled.
 *         Else p = p', A = A + w[i] * tsample(k, p), Wt = Wt + w[i], n += 1.
 *     acc = (w[0] * tsample(k, node) + A_fwd) + A_bwd;  wsum = (w[0] + Wt_fwd) + Wt_bwd;  out = (float)(acc / wsum);
 *     ends = end_fwd | end_bwd << 2;  count = 1 + n_fwd + n_bwd.
 *   Every index is formed from a finite value clamped to the grid: no input makes the kernel read outside its operands.
 *   FS_ERR_NULLPTR: flows, tex, weights, out or ws NULL.  FS_ERR_SHAPE: K < 1, C other than 2 (2-D) / 3 (3-D), an extent
 *   < 1, a stride below its minimum.  FS_ERR_ARG: L outside 0 .. FS_LIC_MAX_L, h not finite or <= 0, vmin not finite or
 *   < 0, a method other than the two, ws not 16-byte aligned.  All of them are returned before anything is launched; the
 *   _ws_bytes queries launch nothing and return the byte count or -(FS_ERR_*).
 */
#define FS_LIC_MAX_L 1024
enum { FS_LIC_FULL = 0, FS_LIC_OUT = 1, FS_LIC_STAGNANT = 2, FS_LIC_NONFINITE = 3 };
long long fs_lic2d_ws_bytes(int K, int H, int W);
long long fs_lic3d_ws_bytes(int K, int D, int H, int W);
int fs_lic2d(const float* flows, int K, int C, int H, int W, long long flow_sstride, const float* tex,
             long long tex_sstride, const double* weights, int L, double h, double vmin, int method, float* out,
             unsigned char* ends, int* count, void* ws, fs_stream_t stream);
int fs_lic3d(const float* flows, int K, int C, int D, int H, int W, long long flow_sstride, const float* tex,
             long long tex_sstride, const double* weights, int L, double h, double vmin, int method, float* out,
             unsigned char* ends, int* count, void* ws, fs_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Critical points -- where K step flows vanish and what kind of zero each is (source, sink, saddle, spiral): the zeros
 * of the piecewise-linear field on the Kuhn split of every cell, with the Jacobian of the affine piece, its invariants
 * and its class.  Two passes with the caller's prefix sum between them, shaped like the isosurface pair.
 *   flows: as for fs_velgrad*: K fields of C fp32 planes of D*H*W elements (2-D: D = 1, C = 2; 3-D: C = 3), field k at
 *     + k * flow_sstride elements (>= C*D*H*W: every other field of a stack is read in place), node (z, y, x) at
 *     (z * H + y) * W + x; component 0 and axis 0 run along x (W), 1 along y, 2 along z.  Every extent >= 2.
 *   inv_h: HOST array of C doubles, 1 / h_c; scale: HOST array of K doubles, velocity = displacement * scale[k]; all
 *     finite and positive.  The scales travel in the launches' arguments: nothing is copied to the device.
 *     vmin >= 0, finite, rounded to fp32 once.
 *   All arithmetic below is fp64 on the widened fp32 values, without fused multiply-adds, in exactly the written order
 *   (a restatement with the same operations in the same order reproduces every bit but vmax's square root;
 *   tests/critical_ref.py).
 *   Simplices.  A cell is a node whose coordinates are all below extent - 1; corner c of it sits at the offset
 *     (dz, dy, dx) = (c >> 2 & 1, c >> 1 & 1, c & 1).
 *     3-D: the six tetrahedra of the isosurface section: one per permutation pi of the axes (x = 0, y = 1, z = 2) in
 *       lexicographic order, t = 0..5, with the corners c0 = the cell's node, c1 = c0 + e_pi0, c2 = c1 + e_pi1,
 *       c3 = c0 + (1,1,1).
 *     2-D: two triangles: t = 0 is pi = (x, y) with c0, c0 + ex, c0 + ex + ey; t = 1 is pi = (y, x) with c0, c0 + ey,
 *       c0 + ex + ey.
 *     The corners of a simplex are in increasing linear node index; the definition rests on this.
 *   Per simplex with corner values v0..vC (C-vectors), in this order:
 *     1. A cell with a corner that has a component that is not finite is NONFINITE: none of its simplices counts or
 *        emits anything.
 *     2. Every corner with (vx^2 + vy^2) + vz^2 <= ((double)(float)vmin)^2 (2-D: vx^2 + vy^2): QUIET, nothing.  With
 *        vmin = 0 an all-zero simplex is quiet.
 *     3. Some component > 0 at all corners, or < 0 at all corners: no point.
 *     4. The face minors m_i = the determinant of the corners other than i, in increasing corner number:
 *          det3(a,b,c) = (a0*(b1*c2 - b2*c1) - a1*(b0*c2 - b2*c0)) + a2*(b0*c1 - b1*c0);  det2(a,b) = a0*b1 - a1*b0
 *        and s_i = (-1)^i m_i.  Two simplices that share a face, in one cell or across cells, evaluate the same
 *        expression on the same nodes in the same order: the minor is the same bits in both, so a zero near a shared
 *        face belongs to exactly one of them.
 *     5. Some s_i is 0 or not finite: the simplex is DEGENERATE; it is counted and emits nothing.
 *     6. All s_i > 0 or all s_i < 0: the simplex holds one critical point.  Otherwise none.
 *   Per point:
 *     S = ((s0 + s1) + s2) + s3,  l_i = s_i / S            (2-D: S = (s0 + s1) + s2)
 *     o0 = (l1 + l2) + l3,  o1 = l2 + l3,  o2 = l3         (2-D: o0 = l1 + l2, o1 = l2)
 *     coordinate along axis pi_k = (double)i_pik + o_k;  position = (float)(coordinate / inv_h[axis]), stored (x, y(, z)).
 *     J[r][pi_k] = (((double)v_{k+1,r} - (double)v_{k,r}) * inv_h[pi_k]) * scale[step], stored fp64 [C*C] at r * C + c.
 *     3-D: P = (J00 + J11) + J22;
 *          Q = ((J00*J11 - J01*J10) + (J00*J22 - J02*J20)) + (J11*J22 - J12*J21);   R = det3(row 0, row 1, row 2);
 *          Delta = (((((18 P) Q) R - (4 ((P P) P)) R) + (P P) (Q Q)) - 4 ((Q Q) Q)) - 27 (R R);   inv = (P, Q, R, Delta).
 *          n_pos (eigenvalues with a positive real part, by Routh-Hurwitz):  R > 0: 3 if (P > 0 and P*Q > R) else 1;
 *          R < 0: 0 if (P < 0 and P*Q < R) else 2;  else 0.
 *     2-D: tr = J00 + J11, det = J00*J11 - J01*J10, disc = tr*tr - 4*det;   inv = (tr, det, disc, 0).
 *          n_pos = 1 if det < 0; 2 if det > 0 and tr > 0; else 0.
 *     cls (uint8) = n_pos | FS_CP_SPIRAL (Delta < 0; 2-D: disc < 0) | FS_CP_DEGENERATE (R, 2-D: det, equal to 0, or an
 *       invariant not finite; n_pos is then 0) | FS_CP_MARGINAL (3-D: P*Q == R; 2-D: det > 0 and tr == 0).
 *       The Poincare index is the sign of R (det).
 *     vmax = (float)(sqrt(the largest of the corners' sums of step 2) * scale[step]).
 *   The points of a step are ordered by cell index, then by t.  Bitwise reproducible: no atomic decides a value or an
 *   order.
 *
 * fs_critical_count{2,3}d -- one launch for all K steps.  ws: fs_critical{2,3}d_ws_bytes bytes, 16-byte aligned, written as
 *     int32 np[K*D*H], int32 ndeg[K*D*H]: per row (k, z, y) the points and the degenerate simplices of its cells;
 *     padding to a multiple of 16 bytes;  uint8 mask[K][D*H*W], one byte per cell's origin node (0 for a node that is no
 *     cell's origin): bit t = simplex t holds a point, FS_CP_MASK_DEGENERATE = the cell has a degenerate simplex,
 *     FS_CP_MASK_NONFINITE = a corner is not finite (no other bit is then set).
 * The caller turns np into row_offsets, int64 [K*D*H + 1] in DEVICE memory: the exclusive prefix sum over all rows with
 *   the total N at the end.
 * fs_critical_emit{2,3}d -- one launch per few hundred steps (none when N = 0).  It recomputes every row's
 *   in-row prefix from the masks; a point is row (row offset + in-row prefix at its cell + rank of t in the cell's mask)
 *   of cell int32 [N] (the origin's node index within its step), simplex uint8 [N], pos fp32 [N][C], jac fp64 [N][C*C],
 *   inv fp64 [N][4], cls uint8 [N] and vmax fp32 [N].  Nothing is written at or beyond row N.  status: int32 [1], zeroed
 *   by the CALLER; bit 0 is set when the masks and the offsets disagree -- the outputs are then not a table.
 *   FS_ERR_NULLPTR: flows, ws (inv_h, scale, row_offsets, status) NULL; an output with N > 0.  FS_ERR_SHAPE: K < 1 or
 *   K*D*H above 2^31 - 1, C other than 2 (2-D) / 3 (3-D), an extent below 2, 2^31 - 1 nodes or more, flow_sstride below
 *   C*D*H*W.  FS_ERR_ARG: an inv_h[c] or scale[k] that is not finite or not positive, vmin negative or not finite (as
 *   fp32), N negative, ws not 16-byte aligned.  All of them are returned before anything is launched; the _ws_bytes
 *   queries launch nothing and return the byte count or -(FS_ERR_*).
 */
enum { FS_CP_NPOS_MASK = 3, FS_CP_SPIRAL = 4, FS_CP_DEGENERATE = 8, FS_CP_MARGINAL = 16 };
enum { FS_CP_MASK_DEGENERATE = 64, FS_CP_MASK_NONFINITE = 128 };
long long fs_critical2d_ws_bytes(int K, int H, int W);
long long fs_critical3d_ws_bytes(int K, int D, int H, int W);
int fs_critical_count2d(const float* flows, int K, int C, int H, int W, long long flow_sstride, double vmin,
                        unsigned char* ws, fs_stream_t stream);
int fs_critical_count3d(const float* flows, int K, int C, int D, int H, int W, long long flow_sstride, double vmin,
                        unsigned char* ws, fs_stream_t stream);
int fs_critical_emit2d(const float* flows, int K, int C, int H, int W, long long flow_sstride, const double* inv_h,
                       const double* scale, double vmin, const unsigned char* ws, const long long* row_offsets, long long N,
                       int* cell, unsigned char* simplex, float* pos, double* jac, double* inv, unsigned char* cls,
                       float* vmax, int* status, fs_stream_t stream);
int fs_critical_emit3d(const float* flows, int K, int C, int D, int H, int W, long long flow_sstride, const double* inv_h,
                       const double* scale, double vmin, const unsigned char* ws, const long long* row_offsets, long long N,
                       int* cell, unsigned char* simplex, float* pos, double* jac, double* inv, unsigned char* cls,
                       float* vmax, int* status, fs_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Streamlines -- S lines through K steady fields as geometry, one launch: line s starts at its seed and follows the
 * NORMALISED field of step step[s], with it or against it, for up to M steps of arc length h, and every vertex is kept.
 *   flows: as for fs_lic*: K fields of C fp32 planes of D*H*W elements (2-D: D = 1, C = 2; 3-D: C = 3), field k at
 *     + k * flow_sstride elements (flow_sstride >= C*D*H*W when K > 1); channel 0 along W.  Every extent >= 2 and fewer
 *     than 2^31 nodes.
 *   seeds: fp64 [C][S], component c at + c * seed_cstride (>= S), in elements, x first.
 *   step: int32 [S], the field a line runs in.  sign: int8 [S]: a value < 0 runs against the field, anything else with it.
 *   home: int32 [S] or NULL: the linear index of the cell the line may start in without being captured, or -1 for none.
 *   capture: uint8 [K][D*H*W], step k at + k * capture_sstride (>= D*H*W when K > 1), or NULL: a nonzero byte at a cell's
 *     origin node marks a capturing cell.
 *   M >= 1.  h: the step length in elements, finite and > 0.  vmin: finite and >= 0.
 *   method: FS_ADV_EULER, FS_ADV_RK2 (midpoint) or FS_ADV_RK4.  h, 0.5 * h and h / 6.0 are formed on the host in fp64;
 *     the device only negates them.
 *   verts: fp32; slot i (0 .. M) of line s, component c at i * vert_sstride + c * vert_cstride + s (vert_cstride >= S,
 *     vert_sstride >= C * vert_cstride).  length: int32 [S].  end: uint8 [S], FS_SL_*.  hit: int32 [S].
 *   Per line, in fp64 on the widened fp32 values without fused multiply-adds; square root and division are correctly
 *   rounded; positions stay fp64 for the whole line (a restatement with the same operations in the same order reproduces
 *   every output bit; tests/streamline_ref.py):
 *     sample(k, q), classify(p), dir(k, q): those of fs_lic* above -- the clamp, NONFINITE for a sampled component that
 *       is not finite, n = sqrt((v0*v0 + v1*v1) + v2*v2) (2-D: no third term), STAGNANT for !(n > vmin), d_c = v_c / n.
 *     Slot 0 receives (float)seed, always.  hit = -1, length = 0, left = (home == NULL or home[s] < 0).
 *     k = step[s] outside 0 .. K-1: the line ends INVALID.  Else classify(seed) not ALIVE: it ends OUT or NONFINITE.
 *       Neither samples anything.
 *     hs = h, hh = 0.5 * h, h6 = h / 6.0, all three negated when sign[s] < 0; p = seed.  For i = 1 .. M:
 *       d1 = dir(k, p).
 *       Euler: p' = p + hs * d1.   RK2: d = dir(k, p + hh * d1), p' = p + hs * d.
 *       RK4: d2 = dir(k, p + hh * d1), d3 = dir(k, p + hh * d2), d4 = dir(k, p + hs * d3),
 *         p' = p + h6 * (((d1 + 2 * d2) + 2 * d3) + d4).
 *       A code at any stage ends the line with that code.  Stage points are clamped by sample and never classified.
 *       classify(p') not ALIVE: the line ends OUT; the exit point is not stored.
 *       Else p = p', slot i receives (float)p, length = i.
 *       cell_a = min((int)floor(p_a), S_a - 2), c = (cz * H + cy) * W + cx (the `cell` column of the critical table).
 *       c != home[s]: left = true.  capture != NULL and left and capture[k][c] != 0: the line ends CAPTURED, hit = c.
 *     After M steps the line ends FULL.  Slots beyond `length` are not written.
 *   Every index is formed from a finite value clamped to the grid, and `step` is checked before it selects a field: no
 *   input makes the kernel read or write outside its operands.  One lane per line; bitwise reproducible.
 *   FS_ERR_NULLPTR: flows, seeds, step, sign, verts, length, end or hit NULL.  FS_ERR_SHAPE: K < 1, S < 1, C other than 2
 *   (2-D) / 3 (3-D), an extent < 2, 2^31 nodes or more, a stride below its minimum.  FS_ERR_ARG: M < 1, h not finite or
 *   <= 0, vmin not finite or < 0, an unknown method.  All of them are returned before anything is launched.
 */
enum { FS_SL_FULL = 0, FS_SL_OUT = 1, FS_SL_STAGNANT = 2, FS_SL_NONFINITE = 3, FS_SL_CAPTURED = 4, FS_SL_INVALID = 5 };
int fs_streamlines2d(const float* flows, int K, int C, int H, int W, long long flow_sstride, const double* seeds,
                     long long seed_cstride, long long S, const int* step, const signed char* sign, const int* home,
                     const unsigned char* capture, long long capture_sstride, int M, double h, double vmin, int method,
                     float* verts, long long vert_sstride, long long vert_cstride, int* length, unsigned char* end,
                     int* hit, fs_stream_t stream);
int fs_streamlines3d(const float* flows, int K, int C, int D, int H, int W, long long flow_sstride, const double* seeds,
                     long long seed_cstride, long long S, const int* step, const signed char* sign, const int* home,
                     const unsigned char* capture, long long capture_sstride, int M, double h, double vmin, int method,
                     float* verts, long long vert_sstride, long long vert_cstride, int* length, unsigned char* end,
                     int* hit, fs_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Parallel vectors -- the line-type feature that goes with the vortex regions: the locus where two vector fields v and w
 * of K steps are parallel (Peikert and Roth), as line segments, one per tetrahedron of the Kuhn split that the locus
 * crosses.  w = J v gives the vortex core lines of Sujudi and Haimes, w = vorticity those of Levy et al.  3-D only: in
 * 2-D the locus is a curve, not a feature.  Two passes with the caller's prefix sum between them, shaped like the
 * critical-point pair.
 *   v, w: K fields each of 3 fp32 planes of D*H*W elements, field k at + k * v_sstride (w_sstride) elements (>= 3*D*H*W:
 *     every other field of a stack is read in place), node (z, y, x) at (z * H + y) * W + x; component 0 and axis 0 run
 *     along x (W), 1 along y, 2 along z.  Every extent >= 2.
 *   aux: NULL, or fp32 [K][D*H*W], step k at + k * aux_sstride (>= D*H*W): a scalar carried along to the points.
 *   inv_h: HOST array of 3 doubles, 1 / h_a, finite and positive; it travels in the launch's arguments.
 *   vmin, wmin: >= 0, finite, rounded to fp32 once.
 *   All arithmetic below is fp64 on the widened fp32 values, without fused multiply-adds, in exactly the written order,
 *   with + - * / sqrt (correctly rounded) and comparisons only: a restatement with the same operations in the same
 *   order reproduces every bit (tests/pv_ref.py).
 *   Simplices.  The six tetrahedra t = 0..5 of the critical-point section: corners 0, c1(t), c2(t), 7 of the cell, with
 *     c1 = 1 1 2 2 4 4 and c2 = 3 5 3 6 5 6.  Face f of a tetrahedron is the triangle that omits its corner f; its three
 *     corners stay in increasing node index.
 *   Faces.  Every face is OWNED by the node that is its lowest corner and lives in one of that node's 12 slots: slot s
 *     has the corners 0 < mid(s) < hi(s) of the cell the node is the origin of (corner c at the offset
 *     (dz, dy, dx) = (c >> 2 & 1, c >> 1 & 1, c & 1)):
 *         s     0  1  2  3  4  5  6  7  8  9 10 11
 *         mid   1  1  2  2  4  4  3  5  6  1  2  4
 *         hi    3  5  3  6  5  6  7  7  7  7  7  7
 *     A node owns slot s when all three corners are nodes of the grid (nodes of the far borders own the slots that lie in
 *     the border).  The global face id is (owner's node index within the step) * 12 + s.  Face f of tetrahedron t of a
 *     cell is owned by the cell's corner o(t, f), in slot s(t, f):
 *         f = 0: o = c1(t), s = 3 5 1 4 0 2 (t = 0..5)      f = 1: o = 0, s = 6 7 6 8 7 8
 *         f = 2: o = 0,     s = 9 + (t >> 1)                f = 3: o = 0, s = t
 *     A face is evaluated in its OWNER's frame only -- origin (ox, oy, oz) = the owner, corners 0, mid, hi, values
 *     v_i, w_i, aux_i (i = 0..2) -- so the two tetrahedra that share it, in one cell or across cells, see the same
 *     expressions on the same nodes in the same order: where both emit a segment that ends on the face, key, pos, mu,
 *     vel and aux are the same bits.  Everything downstream (linking segments into lines) rests on this.
 *   Per face.  A face with a corner at which a component of v or w, or aux when given, is not finite holds nothing and
 *     is not counted.  Otherwise:
 *     1. Quiet.  Corner i is quiet when (vx^2 + vy^2) + vz^2 <= ((double)(float)vmin)^2 or the same sum of w_i <=
 *        ((double)(float)wmin)^2.  A face whose three corners are all quiet holds nothing.
 *     2. Reject.  For every component k of the cross product, with (j, l) = (1, 2), (2, 0), (0, 1) for k = 0, 1, 2 and
 *        x(p, q) = v_p[j] * w_q[l] - v_p[l] * w_q[j]:  the six numbers x(0,0), x(1,1), x(2,2), x(0,1) + x(1,0),
 *        x(0,2) + x(2,0), x(1,2) + x(2,1) are, up to a factor, the Bernstein coefficients of (v x w)_k on the face.  If for
 *        some k all six are > 0 or all six are < 0, the face holds nothing.  (Rigorous: it removes no point.)
 *     3. Pencil.  det3 as in the critical-point section.  dV = det3(v0, v1, v2), dW = det3(w0, w1, w2).  A = w, B = v when
 *        |dW| >= |dV|; otherwise A = v, B = w ("swapped").  dA equal to 0 or not finite: the face is DEGENERATE, it is
 *        counted and holds nothing.  m1 = (det3(A0,B1,B2) + det3(B0,A1,B2)) + det3(B0,B1,A2),
 *        m2 = (det3(A0,A1,B2) + det3(A0,B1,A2)) + det3(B0,A1,A2);  a = -(m2 / dA), b = m1 / dA, c = -(dB / dA);
 *        p(x) = ((x + a) * x + b) * x + c, the monic det(B - x A) / -dA;  p'(x) = (3 * x + 2 * a) * x + b.
 *     4. Real roots.  R = 1 + max(|a|, |b|, |c|) (the maximum by > from the left);  disc = a * a - 3 * b.
 *        disc > 0: q = sqrt(disc), k1 = (-a - q) / 3, k2 = (-a + q) / 3; otherwise k1 = k2 = -R.
 *        For the intervals (lo, hi) = (-R, k1), (k1, k2), (k2, R) in this order: when lo < hi and (p(lo) < 0) differs from
 *        (p(hi) < 0), the interval holds one root: 64 times m = 0.5 * (lo + hi), then lo = m when (p(m) < 0) equals what
 *        (p(lo) < 0) was at the start, else hi = m;  x = 0.5 * (lo + hi);  then twice x' = x - p(x) / p'(x), taken
 *        (x = x') only when x' is finite and lo <= x' <= hi.  The roots of a face are ranked r = 0, 1, 2 in this order.
 *     5. Per root x.  N[c][i] = B_i[c] - x * A_i[c] (rows c: components, columns i: corners).  n = the cross product
 *        (a1*b2 - a2*b1, a2*b0 - a0*b2, a0*b1 - a1*b0) of the row pair (0,1), (0,2) or (1,2) with the largest
 *        (n0^2 + n1^2) + n2^2; a later pair wins only when strictly larger.  The root is an accepted POINT when n0, n1,
 *        n2 are all > 0 or all < 0.  S = (n0 + n1) + n2, l_i = n_i / S.
 *        Coordinate along axis a: c = (double)o_a;  c = c + l_1 when bit a of mid is set;  c = c + l_2 when bit a of hi
 *        is set;  pos[a] = (float)(c / inv_h[a]), stored (x, y, z).
 *        mu (w = mu * v at the point) = x when swapped, else 1 / x; it may be +-inf or 0.
 *        vel[c] = (float)((l_0 * v_0[c] + l_1 * v_1[c]) + l_2 * v_2[c]);  aux likewise.
 *        key = 4 * (global face id) + r.
 *   Per cell.  A cell is a node whose coordinates are all below extent - 1.  A cell with a corner at which a component
 *     of v or w, or aux when given, is not finite is NONFINITE: none of its tetrahedra counts or emits anything.
 *   Per tetrahedron.  n = the points of its four faces.  n == 2: one segment, its endpoints in (f, r) order.  n == 0:
 *     nothing.  Anything else: AMBIGUOUS; it is counted and emits nothing (pairing four points is a choice).
 *   The segments of a step are ordered by cell index, then by t.  Bitwise reproducible: no atomic decides a value or an
 *   order.
 *
 * fs_pv_count3d -- all K steps; two kernels on the stream (faces by their owners, then tetrahedra).  ws: fs_pv3d_ws_bytes
 *     bytes, 16-byte aligned, written as  int32 nseg[R], namb[R], ndeg[R], nnf[R] with R = K*D*H: per row (k, z, y) the
 *     segments and the ambiguous tetrahedra of its cells, the degenerate faces its nodes own (each face once) and its
 *     nonfinite cells; padding to a multiple of 16 bytes;  uint32 faces[K][D*H*W]: bits 2s, 2s+1 = the points of the
 *     node's slot s, FS_PV_NODE_NONFINITE = a value at the node is not finite;  uint8 mask[K][D*H*W], one byte per
 *     cell's origin node: bit t = tetrahedron t holds a segment, FS_PV_MASK_AMBIGUOUS, FS_PV_MASK_NONFINITE.
 * The caller turns nseg into row_offsets, int64 [R + 1] in DEVICE memory: the exclusive prefix sum with N at the end.
 * fs_pv_emit3d -- one launch (none when N = 0) on the same operands.  It re-solves, in the owner's frame, those faces of
 *   the flagged tetrahedra whose count is not 0.  Segment = row (row offset + in-row prefix + rank of t in the cell's
 *   mask) of cell int32 [N] (the cell's node index within its step), simplex uint8 [N], face uint8 [N][2] (f of each
 *   endpoint), key int64 [N][2], pos fp32 [N][2][3], mu fp64 [N][2], vel fp32 [N][2][3] and, when aux is given, aux_out
 *   fp32 [N][2].  Nothing is written at or beyond row N.  status: int32 [1], zeroed by the CALLER; bit 0 is set when the
 *   passes disagree (the mask, the offsets, or a re-solved face) -- the outputs are then not a table.
 *   FS_ERR_NULLPTR: v, w, ws (inv_h, row_offsets, status) NULL; an output with N > 0 (aux_out only when aux is given).
 *   FS_ERR_SHAPE: K < 1 or K*D*H above 2^31 - 1, an extent below 2, 2^31 - 1 nodes or more, v_sstride or w_sstride
 *   below 3*D*H*W, aux_sstride below D*H*W when aux is given.  FS_ERR_ARG: vmin or wmin negative or not finite (as fp32),
 *   an inv_h[a] that is not finite or not positive, N negative, ws not 16-byte aligned.  All of them are returned before
 *   anything is launched; the _ws_bytes query launches nothing and returns the byte count or -(FS_ERR_*).
 */
enum { FS_PV_MASK_AMBIGUOUS = 64, FS_PV_MASK_NONFINITE = 128, FS_PV_NODE_NONFINITE = 1 << 24 };
long long fs_pv3d_ws_bytes(int K, int D, int H, int W);
int fs_pv_count3d(const float* v, long long v_sstride, const float* w, long long w_sstride, const float* aux,
                  long long aux_sstride, int K, int D, int H, int W, double vmin, double wmin, unsigned char* ws,
                  fs_stream_t stream);
int fs_pv_emit3d(const float* v, long long v_sstride, const float* w, long long w_sstride, const float* aux,
                 long long aux_sstride, int K, int D, int H, int W, const double* inv_h, double vmin, double wmin,
                 const unsigned char* ws, const long long* row_offsets, long long N, int* cell, unsigned char* simplex,
                 unsigned char* face, long long* key, float* pos, double* mu, float* vel, float* aux_out, int* status,
                 fs_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Ridge surfaces -- K scalar volumes to K indexed triangle meshes of their height ridges of co-dimension one (Eberly:
 * the points where the gradient is orthogonal to the eigenvector e of the Hessian's smallest eigenvalue lam, and lam is
 * negative), extracted by Marching Ridges (Furst and Pagendarm) on the Kuhn split of every cell.  Of an FTLE field
 * these are the Lagrangian coherent structures (Sadlo and Peikert 2007); with valley != 0 the valley surfaces.
 *   volumes: K fp32 volumes of D*H*W nodes, node (z, y, x) at (z * H + y) * W + x, volume k at + k * sstride elements
 *     (>= D*H*W); every extent >= 2.  Axis 0 runs along x (W), 1 along y, 2 along z.
 *   inv_2h, inv_hh, inv_4hh: HOST arrays of 3 doubles: 1 / (2 h_c) and 1 / h_c^2 for c = x, y, z, and 1 / (4 h_a h_b) for
 *     ab = xy, xz, yz, with h the node spacing.  The host forms them in fp64; the device divides nothing by them.
 *   valley != 0 negates every f as it is read (exactly): the valleys of f are the ridges of -f, bit for bit.
 *
 *   Node pass (fs_ridge_nodes3d), in fp64 without fused multiply-adds; f is widened to fp64 before any arithmetic.  A
 *   restatement with the same operations in the same order reproduces every stored bit.  A node's class is the first
 *   that applies:
 *     FS_RIDGE_BORDER     an index is 0 or extent - 1 along some axis: nothing is extrapolated, the ridge stops one node
 *                         inside.
 *     FS_RIDGE_NONFINITE  one of the 19 stencil values -- the centre, the 6 axis neighbours, the 12 planar diagonals -- is
 *                         not finite; or one of the five stored operands is not finite as fp32 (overflow).
 *     FS_RIDGE_WEAK       !(lam <= -strength), strength >= 0.
 *     FS_RIDGE_LOW        !(f >= fmin); fmin = -inf switches the filter off.
 *     FS_RIDGE_ELIGIBLE   everything else.
 *     g_c  = (f(+c) - f(-c)) * inv_2h[c]
 *     H_cc = ((f(+c) - 2 f) + f(-c)) * inv_hh[c]
 *     H_ab = ((f(+a+b) - f(+a-b)) - (f(-a+b) - f(-a-b))) * inv_4hh[ab]
 *     Eigen-solve: A = H, V = I, then FS_RIDGE_SWEEPS cyclic Jacobi sweeps, each the rotations (p, q) = (0,1), (0,2),
 *       (1,2) in this order, made of IEEE fp64 + - * / sqrt alone.  A rotation with a_pq == 0 changes nothing.  Else
 *         theta = (a_qq - a_pp) / (2 a_pq);   t = 1 / (|theta| + sqrt(theta theta + 1)), negated when theta < 0
 *         c = 1 / sqrt(t t + 1);   s = t c
 *         a_pp' = a_pp - t a_pq;   a_qq' = a_qq + t a_pq;   a_pq' = 0
 *         with r the third index   a_rp' = c a_rp - s a_rq;   a_rq' = s a_rp + c a_rq
 *         for every row k of V     v_kp' = c v_kp - s v_kq;   v_kq' = s v_kp + c v_kq
 *       Equal diagonals give theta = 0 and t = 1 (45 degrees); where theta theta overflows t is 0, c is 1 and the
 *       rotation only clears a_pq, which is then below 2^-511 of the diagonals' difference.  Four sweeps are the fewest
 *       after which |a01| + |a02| + |a12| is at most 2^-45 of H's Frobenius norm on every field of tests/ridge_fields.py
 *       (three leave 6e-6, four 8e-23).
 *     lam = the smallest diagonal entry of A (ties: the lowest index), e = that column of V with the sign it comes out
 *       with, d = (e0 g0 + e1 g1) + e2 g2.
 *   operands: fp32 [K][5][D*H*W] = e0, e1, e2, d, lam, each rounded once; NaN at nodes that are not ELIGIBLE.
 *   cls: uint8 [K][D*H*W].
 *
 *   Marching pass (fs_ridge_count3d, fs_ridge_emit3d).  It reads the stored fp32 operands and classes only, so every
 *   decision can be restated exactly.  Edges e0 .. e6 of the owner node and the six tetrahedra of a cell are those of
 *   the isosurface block above.  For an edge (a, b), a the owner:
 *     o = (ea0 eb0 + ea1 eb1) + ea2 eb2 in fp64;   flip = o < 0;   db' = flip ? -db : db
 *     ACTIVE iff both ends are ELIGIBLE and signbit(da) != signbit(db') (sign bits, not comparisons: +-0 stay consistent
 *     under negation).  An active edge carries one vertex:
 *     t = da / (da - db') in fp64, 0.5 where the denominator is 0, clamped to [0, 1], rounded to fp32 once; the position
 *     follows the isosurface block's formula and order in fp32 (spacing: HOST array of 3 doubles along x, y, z, each
 *     rounded to fp32 once).  The orientation of e is decided per edge from its two ends alone, so every cell sharing an
 *     edge sees the same vertex.
 *   A tetrahedron (corners c0 .. c3) with a corner that is not ELIGIBLE emits nothing.  Otherwise sigma_0 = 0,
 *     sigma_i = (e_c0 . e_ci < 0) for i = 1..3 (the same fp64 dot product), and the tetrahedron is TWISTED when for some
 *     1 <= i < j <= 3 (e_ci . e_cj < 0) != (sigma_i xor sigma_j): e cannot be oriented consistently over it.  A twisted
 *     tetrahedron emits nothing and is counted: a hole in the surface, reported, not an error.  Otherwise corner i is
 *     inside iff !(signbit(d_ci) xor sigma_i), and the triangles are those of the isosurface block for that case
 *     (csrc/iso_tables.hpp).  Every edge the case uses is then active.  The winding is the table's and means nothing
 *     here: a ridge surface need not be orientable, and the sign of e is the solver's -- negating e and d at a node
 *     turns the cases of its tetrahedra into their complements, which hold the same triangles on the same vertices
 *     with the other winding (and, for two triangles, in the other order).
 *   Vertices of a step are ordered by owner node index, then edge number; faces by cell index, tetrahedron, triangle,
 *   as int32 vertex indices local to their step.  values_out (optional): fp32 [V][2] = f (negated under valley) and
 *   the stored lam, each wa + t (wb - wa) in fp32; fused multiply-adds are allowed there.  The result is bitwise
 *   reproducible: no atomic decides a position or an order.
 *
 * fs_ridge_nodes3d -- one launch.
 * fs_ridge_count3d -- one launch.  ws: fs_ridge3d_ws_bytes bytes, 4-byte aligned, written as
 *     int32 nv[K*D*H], nt[K*D*H], ntwisted[K*D*H], ntets[K*D*H]: per row (k, z, y) the vertices its nodes own, the
 *     triangles its cells emit, their twisted tetrahedra and their tetrahedra with four ELIGIBLE corners;
 *     uint8 mask[K][D*H*W]: bit e of a node's byte = its edge e is active.
 * The caller turns nv and nt into row_offsets, int64 [2][K*D*H + 1] in DEVICE memory, as for fs_iso_emit3d.
 * fs_ridge_emit3d -- one launch (none when V and T are 0) on the same operands; vertices [V][3], values_out [V][2] (NULL:
 *   not wanted), faces int32 [T][3].  Nothing is written at or beyond row V or T.  status: int32 [1], zeroed by the
 *   CALLER; bit 0 is set when the passes disagree (a mask that these operands do not give, a row's counts, an index
 *   outside its step, a triangle on an edge that is not active) -- the outputs are then not a mesh.
 *   FS_ERR_NULLPTR: volumes, the host arrays, operands, cls, ws, row_offsets or status NULL; vertices with V > 0, faces
 *   with T > 0.  FS_ERR_SHAPE: K < 1 or K*D*H above 2^31 - 1, an extent below 2, more than 2^31 - 1 nodes, sstride below
 *   D*H*W.  FS_ERR_ARG: an inv_2h, inv_hh, inv_4hh or spacing entry that is not finite and positive (spacing: as fp32),
 *   strength negative or not finite, fmin NaN or +inf, V or T negative, ws not 4-byte aligned.  All of them are returned
 *   before anything is launched; the _ws_bytes query launches nothing and returns the byte count or -(FS_ERR_*).
 */
#define FS_RIDGE_SWEEPS 4
enum { FS_RIDGE_BORDER = 0, FS_RIDGE_NONFINITE = 1, FS_RIDGE_WEAK = 2, FS_RIDGE_LOW = 3, FS_RIDGE_ELIGIBLE = 4 };
long long fs_ridge3d_ws_bytes(int K, int D, int H, int W);
int fs_ridge_nodes3d(const float* volumes, int K, int D, int H, int W, long long sstride, int valley,
                     const double* inv_2h, const double* inv_hh, const double* inv_4hh, double strength, double fmin,
                     float* operands, unsigned char* cls, fs_stream_t stream);
int fs_ridge_count3d(const float* operands, const unsigned char* cls, int K, int D, int H, int W, unsigned char* ws,
                     fs_stream_t stream);
int fs_ridge_emit3d(const float* volumes, int K, int D, int H, int W, long long sstride, int valley,
                    const float* operands, const unsigned char* cls, const double* spacing, const unsigned char* ws,
                    const long long* row_offsets, long long V, long long T, float* vertices, float* values_out,
                    int* faces, int* status, fs_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Training batches out of a stored time series -- Flow-3D/load_datasets.py:29-190 `load_data` (un-pickle, nan_to_num,
 * np.float32, append flipped copies, cut (img0, img1, gt) triplets) and the host-to-device copy of Flow-3D/train.py:144,
 * as one launch per batch over an array that stays on the device in its stored type.
 *   base: `n_elems` elements of `dtype` (FS_SERIES_*: uint8, uint16, IEEE half, float), frames of Ds x Hs x Ws
 *     elements (Ds = 1 for the 2-D models) anywhere inside it.
 *   jobs: B records in DEVICE memory (8-byte aligned), one per sample:
 *     off[3]     element offsets inside base of the frames written to channels 0, 1, 2 (img0, img1, gt): t*Ds*Hs*Ws
 *                for a series [T,D,H,W], (3n + c)*Ds*Hs*Ws for ready-made triplets [N,3,D,H,W]
 *     z0, y0, x0 crop origin
 *     flip       bit 0: mirror along W, bit 1: along H, bit 2: along D -- of the cropped block:
 *                out[z,y,x] = frame[z0 + (flip & 4 ? Do-1-z : z), y0 + (flip & 2 ? Ho-1-y : y), x0 + (flip & 1 ? Wo-1-x : x)]
 *     lo, inv    out = (v - lo) * inv, two separately rounded fp32 operations (no FMA)
 *   out: fp32 [B,3,Do,Ho,Wo], contiguous.
 *   v is the stored value converted exactly to fp32; a non-finite v (NaN, +-inf) becomes 0 before the normalisation
 *   (the reference's np.nan_to_num maps +-inf to +-FLT_MAX instead: a deliberate divergence).
 *   The library cannot read the records, so the kernel checks them: a source coordinate outside the frame, or an
 *   element index outside [0, n_elems), reads as 0 -- no record makes the kernel touch memory outside base.
 *   FS_ERR_SHAPE: B or an extent < 1, a crop larger than the frame, a frame larger than the array, more than 2^31-1
 *   output elements per channel; FS_ERR_ARG: an unknown dtype, base not aligned to its element, jobs to 8 bytes.
 *
 * fs_series_stats: for each of T consecutive frames of frame_elems elements, out[t] = {minimum over the finite
 *   elements (+inf if none), maximum (-inf if none), number of non-finite elements} as fp64 (every value of the four
 *   types and every count below 2^53 is exact).  Partials per workgroup in `ws` (fs_series_stats_ws_bytes bytes, 8-byte
 *   aligned), combined by a second launch in a fixed order: no atomics.  FS_ERR_SHAPE: T < 1 or > 2^22, frame_elems < 1
 *   or > 2^40.  The _ws_bytes query launches nothing and returns the byte count or -(FS_ERR_*).
 */
enum { FS_SERIES_U8 = 0, FS_SERIES_U16 = 1, FS_SERIES_F16 = 2, FS_SERIES_F32 = 3 };
typedef struct FsTripletJob {
  long long off[3];
  int z0, y0, x0;
  unsigned flip;
  float lo, inv;
  int reserved[4];
} FsTripletJob; /* 64 bytes */
int fs_triplet_gather(const void* base, int dtype, long long n_elems, int Ds, int Hs, int Ws, const FsTripletJob* jobs,
                      int B, int Do, int Ho, int Wo, float* out, fs_stream_t stream);
long long fs_series_stats_ws_bytes(int T, long long frame_elems);
int fs_series_stats(const void* base, int dtype, int T, long long frame_elems, double* ws, double* out,
                    fs_stream_t stream);

/* ------------------------------------------------------------------------------------
 * The way back: padded fp32 planes to a stored type -- the crop (`[..., :D, :H, :W]` of what a model returned for
 * inputs padded to multiples of 32) and the conversion in one pass, so that a rebuilt series or its flows leave the
 * device in the type they are kept in.
 *   src: fp32 [N,C,Dp,Hp,Wp], contiguous.  dst: `dtype` (FS_SERIES_*) [N,C,D,H,W], contiguous, = the corner
 *   [0:D, 0:H, 0:W] of every plane (Dp = D = 1 for 2-D).
 *   Per element y = x * span, then y = y + lo: two separately rounded fp32 operations (no FMA), the inverse of the
 *   gather's (v - lo) * inv up to rounding.  A non-finite y is stored as 0 and counted as non-finite (neither low nor
 *   high).  U8 / U16: low when y < 0, high when y > 255 / 65535; clamped, rounded to nearest even, converted.  F16:
 *   low / high when y < -65504 / y > 65504; saturated to +-65504, else fp32 -> half with round to nearest even.
 *   F32: y itself (nothing is low or high).
 *   stats (nullable, together with ws): fp64 [N,5] = {min y, max y over the finite y before clamping (+inf / -inf if
 *   none), n_low, n_high, n_nonfinite} over all C planes of item n.  Partials per workgroup in `ws`
 *   (fs_series_encode_ws_bytes bytes, 8-byte aligned), combined by a second launch in a fixed order: no atomics; which
 *   elements a lane reduces depends on the shape alone, so the stats do not depend on pointer alignment.  With
 *   ws == stats == NULL one launch, no reduction.
 *   A lane owns 4 consecutive outputs of a row when W % 4 == 0 and Wp % 4 == 0 (one 16-byte load and one 4 / 8 /
 *   16-byte store when src is 16-byte aligned and dst aligned to 4 elements), one element otherwise.
 *   FS_ERR_NULLPTR: src or dst NULL, exactly one of ws / stats NULL.  FS_ERR_SHAPE: an extent < 1, D > Dp, H > Hp,
 *   W > Wp, N > 2^20, more than 2^31-1 padded elements per item or 2^40 in all.  FS_ERR_ARG: an unknown dtype, dst not
 *   aligned to its element, src to 4 bytes, ws / stats to 8.  The _ws_bytes query launches nothing and returns the
 *   byte count or -(FS_ERR_*).
 */
long long fs_series_encode_ws_bytes(int N, int C, int D, int H, int W);
int fs_series_encode(const float* src, int N, int C, int Dp, int Hp, int Wp, void* dst, int dtype, int D, int H, int W,
                     float lo, float span, double* ws, double* stats, fs_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Census distance on volumes: the arithmetic of a8 (UPFlow/utils/loss.py:59-71) without the grey conversion, a volume
 * has one channel.  Zero-padded (2r+1)^3 neighbourhood, u = v[n] - v[c], t = u / sqrt(0.81 + u^2),
 *   dist[c] = sum over the (2r+1)^3 taps of (t1 - t2)^2 / (0.1 + (t1 - t2)^2).
 *   vol1, vol2, dist, grad_* [B,1,D,H,W] fp32 contiguous; every extent >= 1 is legal.  radius 1, 2 or 3 (FS_ERR_ARG
 *   otherwise).  FS_ERR_SHAPE: B * ceil(D / 8) or ceil(H / 16) above 65535.  Bitwise equal vol1 and vol2 give a dist and
 *   gradients of exactly 0; a voxel's 2r+1 taps along D are summed first, then added to its sum.
 * bwd: grad_vol1 / grad_vol2 (nullable, overwritten) = d sum(grad_dist * dist) / d vol1, vol2; gather-formulated, no
 * atomics, bit-reproducible.  The loss is fs_robust_sum(dist, ...) as in 2-D.
 */
int fs_census3d_dist_fwd(const float* vol1, const float* vol2, float* dist,
                         int B, int D, int H, int W, int radius, fs_stream_t stream);
int fs_census3d_dist_bwd(const float* vol1, const float* vol2, const float* grad_dist,
                         float* grad_vol1, float* grad_vol2,
                         int B, int D, int H, int W, int radius, fs_stream_t stream);

/* ------------------------------------------------------------------------------------
 * First-order flow smoothness on volumes (the term Flow-3D/model/RIFE.py:147-167 holds commented out), over pairs of
 * voxels that both exist, with an optional edge-aware weight:
 *   sums[0] = sum over b, c, voxel p, axis a in {D,H,W} with p + e_a inside of
 *             w_a(p) * ((flow[b,c,p+e_a] - flow[b,c,p])^2 + eps^2)^q,
 *             w_a(p) = exp(-kappa * |guide[b,0,p+e_a] - guide[b,0,p]|);  guide NULL or kappa == 0: w = 1
 *   sums[1] = the number of (b, c, voxel, axis) pairs counted (exact while it is below 2^24, rounded once above).
 *   flow [B,C,D,H,W], guide [B,1,D,H,W] (no gradient), sums: 2 device floats, ws: 2*FS_REDUCE_BLOCKS floats.
 *   Deterministic (per-workgroup partials, fixed-order finish).  FS_ERR_ARG: q <= 0, kappa < 0, eps^2 not a normal
 *   fp32 number (eps = 0 has no gradient at a zero difference), anything not finite.
 * bwd: grad_flow (overwritten) = coef[0] * d sums[0] / d flow; every voxel gathers its up to six differences.
 */
int fs_flow_smooth3d_fwd(const float* flow, const float* guide, float* sums, float* ws,
                         int B, int C, int D, int H, int W, float q, float eps, float kappa, fs_stream_t stream);
int fs_flow_smooth3d_bwd(const float* flow, const float* guide, const float* coef, float* grad_flow,
                         int B, int C, int D, int H, int W, float q, float eps, float kappa, fs_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* FLOWSCI_HIP_H */
