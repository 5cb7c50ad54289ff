"""torch.autograd bindings of the HIP hot-path kernels (C-ABI in include/flowsci_hip.h).

Every op validates its operands on the host (dtype fp32, CUDA device, matching shapes; operands
are made contiguous) and raises ValueError on a mismatch, then launches on PyTorch's current
stream of the operand's device.  Nothing here computes on the CPU: without a GPU build of
libflowsci_hip.so these functions raise.
"""
import ctypes
from fractions import Fraction

import torch

from . import _lib

WARP2D_RIFE, WARP2D_PWC, WARP2D_PHOTO, WARP2D_DILATED = 0, 1, 2, 3


def _stream(t):
    return torch.cuda.current_stream(t.device).cuda_stream


def _need_cuda_f32(name, t, ndim):
    if not isinstance(t, torch.Tensor):
        raise ValueError("%s must be a tensor" % name)
    if t.dtype != torch.float32:
        raise ValueError("%s must be float32, got %s" % (name, t.dtype))
    if t.dim() != ndim:
        raise ValueError("%s must be %d-D, got shape %s" % (name, ndim, tuple(t.shape)))
    if not t.is_cuda:
        raise ValueError("%s must live on a GPU (the HIP hot path has no CPU fallback); got %s" %
                         (name, t.device))
    return t.contiguous()


def _need_cuda_f32_strided(name, t, ndim):
    """_need_cuda_f32 without the `.contiguous()`: for operands whose strides are handed to the kernel."""
    if not isinstance(t, torch.Tensor):
        raise ValueError("%s must be a tensor" % name)
    if t.dtype != torch.float32 or t.dim() != ndim or not t.is_cuda:
        raise ValueError("%s must be a %d-D float32 GPU tensor, got %s %s on %s" %
                         (name, ndim, t.dtype, tuple(t.shape), t.device))
    return t


def _ptr(t):
    return 0 if t is None else t.data_ptr()


def _aligned16(t):
    """`t`, or a copy of it when its data does not start on a 16-byte boundary: the convolution epilogues read addend /
    act_y 16 bytes at a time and refuse anything else (include/flowsci_hip.h)."""
    return t if t.data_ptr() % 16 == 0 else t.clone()


def _in_dhw(inp, flow):
    """Host int[3] with the sampled volume's extent, or None when it equals the flow's."""
    if tuple(inp.shape[2:]) == tuple(flow.shape[2:]):
        return None
    return (ctypes.c_int * 3)(*inp.shape[2:])


# Optional per-launch timing with HIP events recorded on the launch stream (bench.py's roofline
# leg).  Off by default: no events, no overhead.
_timing = None
_timing_only = None


def enable_kernel_timing(on=True, only=None):
    """Start (on=True: clears previous records) or stop collecting (start, end) event pairs.  `only`: an
    iterable of entry-point names -- every other launch goes out without events (bench.py's timed region
    records just the dominant entry point, so that the headline time carries no profiling overhead)."""
    global _timing, _timing_only
    _timing = {} if on else None
    _timing_only = frozenset(only) if (on and only is not None) else None


def kernel_timings():
    """{entry point: [(ms, algorithmic HBM bytes, matrix-core flops EXECUTED, flops of the direct formulation, kernel
    symbol or None) per launch]} recorded so far (synchronises).  The two flop counts differ for the Winograd
    convolutions only (1/3, 1/2); the kernel symbol is known where the entry point's dispatch can be asked for it."""
    if _timing is None:
        return {}
    torch.cuda.synchronize()
    return {k: [(a.elapsed_time(b), nb, fl, fe, sym) for a, b, nb, fl, fe, sym in v] for k, v in _timing.items()}


def _call(name, *args, algo_bytes=0, algo_flops=0, record_as=None, equiv_flops=None, kernel=None, allow=()):
    """Launch a C-ABI entry point and return its status: 0, or one in `allow` (FS_ERR_UNSUPPORTED: "no such kernel
    for this shape, take the unfused path"); any other status raises.  `algo_bytes` / `algo_flops` = compulsory HBM
    bytes / useful flops of this launch, only used by the optional timing records (`record_as`: file
    the record under another entry point's name -- the *_prelu variants are the same kernels with one more store)."""
    fn = getattr(_lib.lib(), name)
    if _timing is None or (_timing_only is not None and (record_as or name) not in _timing_only):
        rc = fn(*args)
    else:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        rc = fn(*args)
        e1.record()
        if rc == 0:
            _timing.setdefault(record_as or name, []).append((e0, e1, algo_bytes, algo_flops,
                                                              algo_flops if equiv_flops is None else equiv_flops, kernel))
    if rc not in allow:
        _lib.check(rc, name)
    return rc


# The kernel a convolution or 3-D warp launch runs, by the library's own plan for its geometry: the slab kind of
# fs_conv3d_{fwd,tr}_wprep_jobs (FS_WPREP_* in csrc/wprep.hpp), the id of fs_conv3d_wrw_kernel_id (FS_WRW_KERNEL_*) or
# of fs_warp3d_kernel_id (FS_W3_KERNEL_*, both in include/flowsci_hip.h) -> (its symbol as `rocprofv3 --kernel-trace
# --stats` prints it, matrix-core flops EXECUTED per flop of the direct formulation).  Either may be a function of
# (C, W): the launch's output channels and output width (wrw: the gradient's).  The split-bf16 kernels execute six bf16
# products per fp32 multiply-add (priced against the bf16 peak), the Winograd forms 2/3, 1/2 or 1/3 of the direct
# form's multiply-adds.  A plan not listed runs one of several fp32 instantiations: no symbol, the direct flops.
_KERNELS = {
    ("fwd", 4): (None, Fraction(2, 3)),  # FS_WPREP_WINO: F(2,3) along x (ablation build)
    ("fwd", 5): (None, Fraction(1, 2)),  # FS_WPREP_WINO4: F(4,3) along x (ablation build)
    ("fwd", 6): (lambda C, W: "conv3d_wino2d_ps_kernel<0, %d>" % (16 if W % 64 == 0 else 8),  # FS_WPREP_WINO2D
                 Fraction(1, 3)),
    ("fwd", 7): (lambda C, W: "conv3d_fwd_s3_kernel<%d, 8, 4>" % (1 if C <= 32 else 2), 6),  # FS_WPREP_S3K4
    ("tr", 8): ("convtr_s3_kernel<false>", lambda C, W: Fraction(6 * 32 * ((C + 31) // 32), C)),  # FS_WPREP_TRS3
    ("tr", 9): ("convtr_s3_kernel<true>", lambda C, W: Fraction(6 * 16, C)),  # FS_WPREP_TRS3_16
    ("wrw", 2): (None, Fraction(2, 3)),  # FS_WRW_KERNEL_WINO23 (ablation build)
    ("wrw", 3): ("conv3d_wrw_wino4_kernel<0>", Fraction(1, 2)),  # FS_WRW_KERNEL_WINO43
    ("wrw", 4): (lambda C, W: "conv3d_wrw_s3_kernel<8, 2, 1, 2, 4, 0, %d>" % (16 if W == 16 else 32) if C > 32
                 else "conv3d_wrw_s3_kernel<6, 1, 2, 2, 3, 0, 32>", 6),  # FS_WRW_KERNEL_S3
    ("warp3d_fwd", 1): ("warp3d_rc_kernel<false, 2, 6, 0>", 0),  # FS_W3_KERNEL_RC
    ("warp3d_bwd", 1): ("warp3d_rc_kernel<true, 4, 5, 0>", 0),
}
_plans = {}  # (family, misalignments) + geometry -> (plan id, (kernel symbol, flops executed, direct flops))


def _plan(family, mis, geo):
    """The library's plan for one launch of `family` ('fwd', 'tr', 'wrw', 'warp3d_fwd', 'warp3d_bwd'), asked once per
    key and nothing launched: (plan id, (kernel symbol or None, matrix-core flops executed, flops of the direct
    formulation)).  `geo`: the shape arguments of the family's query in its order; `mis`: the 16-byte misalignment of
    each pointer that query inspects (it is handed placeholders)."""
    key = (family, mis) + geo
    hit = _plans.get(key)
    if hit is not None:
        return hit
    L = _lib.lib()
    ptrs = [0x1000 + m for m in mis]
    if family in ("fwd", "tr"):  # B, Cin, Cout, Di, Hi, Wi, Do, Ho, Wo, then k, stride, pad, wmode (fwd) / has_z (tr)
        B, Cin, Cout, Di, Hi, Wi, Do, Ho, Wo = geo[:9]
        jobs = (_lib.FsWprepJob * 8)()
        query = L.fs_conv3d_fwd_wprep_jobs if family == "fwd" else L.fs_conv3d_tr_wprep_jobs
        n = query(jobs, 8, *ptrs, 0x1000, 0x1000, *geo)
        kinds = {jobs[i].kind for i in range(min(n, 8))}
        pid = kinds.pop() if len(kinds) == 1 else None
        C, W = Cout, Wo
        direct = 2 * B * Cin * Cout * (geo[9] ** 3 * Do * Ho * Wo if family == "fwd" else 64 * Di * Hi * Wi)
    elif family == "wrw":  # B, Cg, Cs, Do, Ho, Wo, Di, Hi, Wi, k, stride, pad
        B, C, Cs, Do, Ho, W = geo[:6]
        pid = int(L.fs_conv3d_wrw_kernel_id(*ptrs, *geo))
        direct = 2 * B * C * Cs * geo[9] ** 3 * Do * Ho * W
    else:  # B, C, Di, Hi, Wi, D, H, W, with_grad_in
        B, C, Di, Hi, Wi, D, H, W, with_grad_in = geo
        pid = int(L.fs_warp3d_kernel_id(*ptrs, B, C, (ctypes.c_int * 3)(Di, Hi, Wi), D, H, W,
                                        int(family == "warp3d_bwd"), with_grad_in))
        direct = 0
    sym, factor = (v(C, W) if callable(v) else v for v in _KERNELS.get((family, pid), (None, 1)))
    hit = _plans[key] = (pid, (sym, int(direct * factor), direct))
    return hit


def _kernel_accounting(family, mis, *geo):
    """(kernel symbol or None, matrix-core flops executed, flops of the direct formulation) of a launch, for the timing
    records (see _plan); (None, 0, 0) without asking anything while launches are not timed."""
    return (None, 0, 0) if _timing is None else _plan(family, mis, geo)[1]


# --------------------------------------------------------------------------------------------
# a2: Flow-3D/model/warplayer.py:9-41
# --------------------------------------------------------------------------------------------
class _Warp3D(torch.autograd.Function):
    @staticmethod
    def forward(ctx, inp, flow):
        inp = _need_cuda_f32("tenInput", inp, 5)
        flow = _need_cuda_f32("tenFlow", flow, 5)
        B, C = inp.shape[:2]
        if flow.shape[0] != B or flow.shape[1] != 3:
            raise ValueError("tenFlow must be [B,3,D,H,W] with tenInput's batch %s, got %s" %
                             (tuple(inp.shape), tuple(flow.shape)))
        if inp.device != flow.device:
            raise ValueError("tenInput and tenFlow are on different devices")
        D, H, W = flow.shape[2:]  # the output takes the flow's extent (warplayer.py:11-22, 36)
        out = inp.new_empty((B, C, D, H, W))
        with torch.cuda.device(inp.device):
            _call("fs_warp3d_fwd", inp.data_ptr(), flow.data_ptr(), out.data_ptr(),
                  B, C, _in_dhw(inp, flow), D, H, W, _stream(inp))
        ctx.save_for_backward(inp, flow)
        return out

    @staticmethod
    def backward(ctx, gout):
        inp, flow = ctx.saved_tensors
        need_in, need_flow = ctx.needs_input_grad
        if not (need_in or need_flow):
            return None, None
        gout = gout.contiguous()
        B, C = inp.shape[:2]
        D, H, W = flow.shape[2:]
        gin = torch.zeros_like(inp) if need_in else None
        gflow = torch.empty_like(flow) if need_flow else None
        with torch.cuda.device(inp.device):
            _call("fs_warp3d_bwd", inp.data_ptr(), flow.data_ptr(), gout.data_ptr(),
                  _ptr(gin), _ptr(gflow), B, C, _in_dhw(inp, flow), D, H, W, _stream(inp))
        return gin, gflow


def _empty_like_graph(shape, *tensors):
    """Empty-batch result: zeros of `shape` (numel 0) that still hang on the inputs' autograd graph, as
    `F.grid_sample` / `Corr_pyTorch` return for B = 0.  No kernel is launched for an empty batch."""
    out = tensors[0].new_zeros(shape)
    for t in tensors:
        if t is not None and t.requires_grad:
            out = out + 0 * t.sum()
    return out


def warp3d(tenInput, tenFlow):
    """Trilinear backward warp with the reference's axis-rotating grid (Flow-3D warplayer.warp)."""
    if tenInput.dim() == 5 and tenFlow.dim() == 5 and tenInput.shape[0] == 0 and tenFlow.shape[0] == 0:
        return _empty_like_graph((0, tenInput.shape[1]) + tuple(tenFlow.shape[2:]), tenInput, tenFlow)
    return _Warp3D.apply(tenInput, tenFlow)


# --------------------------------------------------------------------------------------------
# 2-D warps: a1, a5, a6, a7, a11
# --------------------------------------------------------------------------------------------
def _in_hw(inp, flow):
    """Host int[2] with the sampled image's extent, or None when it equals the flow's."""
    if tuple(inp.shape[2:]) == tuple(flow.shape[2:]):
        return None
    return (ctypes.c_int * 2)(*inp.shape[2:])


class _Warp2D(torch.autograd.Function):
    @staticmethod
    def forward(ctx, inp, flow, start, mode, with_mask):
        inp = _need_cuda_f32("input", inp, 4)
        flow = _need_cuda_f32("flow", flow, 4)
        B, C = inp.shape[:2]
        H, W = flow.shape[2:]  # the output takes the flow's extent
        same = tuple(flow.shape[2:]) == tuple(inp.shape[2:])
        if flow.shape[0] != B or flow.shape[1] != 2 or not (same or mode == WARP2D_RIFE):
            # only the RIFE warp defines input extent != flow extent (Flow-2D/model/warplayer.py:10-20)
            raise ValueError("flow must be [B,2,H,W] matching input %s, got %s" %
                             (tuple(inp.shape), tuple(flow.shape)))
        if inp.device != flow.device:
            raise ValueError("input and flow are on different devices")
        if start is not None:
            start = _need_cuda_f32("start", start.reshape(start.shape[0], 2), 2)
            if start.shape[0] != B:
                raise ValueError("start must be [B,2,1,1]")
        out = inp.new_empty((B, C, H, W))
        with torch.cuda.device(inp.device):
            _call("fs_warp2d_fwd", inp.data_ptr(), flow.data_ptr(), _ptr(start),
                  out.data_ptr(), B, C, _in_hw(inp, flow), H, W, mode, int(with_mask), _stream(inp),
                  algo_bytes=4 * flow.numel() + 8 * out.numel())  # flow 8 + per channel gather 4 + store 4
        ctx.save_for_backward(inp, flow, start)
        ctx.mode, ctx.with_mask = mode, int(with_mask)
        return out

    @staticmethod
    def backward(ctx, gout):
        inp, flow, start = ctx.saved_tensors
        need_in, need_flow = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (need_in or need_flow):
            return None, None, None, None, None
        gout = gout.contiguous()
        B, C = inp.shape[:2]
        H, W = flow.shape[2:]
        gin = torch.zeros_like(inp) if need_in else None
        gflow = torch.empty_like(flow) if need_flow else None
        with torch.cuda.device(inp.device):
            _call("fs_warp2d_bwd", inp.data_ptr(), flow.data_ptr(), _ptr(start),
                  gout.data_ptr(), _ptr(gin), _ptr(gflow), B, C, _in_hw(inp, flow), H, W, ctx.mode,
                  ctx.with_mask, _stream(inp),
                  algo_bytes=4 * flow.numel() * (2 if need_flow else 1) + 4 * gout.numel() * (3 if need_in else 2))
        return gin, gflow, None, None, None


def _empty2d(x, flow):
    return x.dim() == 4 and flow.dim() == 4 and x.shape[0] == 0 and flow.shape[0] == 0


def warp2d(tenInput, tenFlow):
    """a1: Flow-2D/model/warplayer.py:7-26 (border pad, align_corners=True)."""
    if _empty2d(tenInput, tenFlow):
        return _empty_like_graph(tuple(tenInput.shape[:2]) + tuple(tenFlow.shape[2:]), tenInput, tenFlow)
    return _Warp2D.apply(tenInput, tenFlow, None, WARP2D_RIFE, 0)


def warp2d_pwc(x, flow, with_mask):
    """a5/a6: pwc_modules.WarpingLayer_no_div (with_mask) / tools.torch_warp (no mask)."""
    if _empty2d(x, flow):
        return _empty_like_graph(x.shape, x, flow)
    return _Warp2D.apply(x, flow, None, WARP2D_PWC, 1 if with_mask else 0)


def occ_check2d(flow_f, flow_b, alpha1, alpha2, scale=1, obj_out_all="obj"):
    """§8f.2: UPFlow/utils/tools.py:560-719 `occ_check_model.__call__` as one launch -- both
    torch_warp calls, the L1 magnitudes, the threshold test, the outgoing masks and their
    combination.  Returns (occ_fw, occ_bw) [B,1,H,W] float {0,1}; no gradient (bool in the
    reference)."""
    mode = {"all": 0, "obj": 1, "out": 2}[obj_out_all]
    flow_f = _need_cuda_f32("flow_f", flow_f.detach(), 4)
    flow_b = _need_cuda_f32("flow_b", flow_b.detach(), 4)
    if flow_f.shape != flow_b.shape or flow_f.shape[1] != 2:
        raise ValueError("flows must both be [B,2,H,W], got %s / %s" % (tuple(flow_f.shape), tuple(flow_b.shape)))
    B, _, H, W = flow_f.shape
    occ_f = torch.empty((B, 1, H, W), device=flow_f.device, dtype=torch.float32)
    occ_b = torch.empty_like(occ_f)
    with torch.cuda.device(flow_f.device):
        _call("fs_occ_check2d", flow_f.data_ptr(), flow_b.data_ptr(), occ_f.data_ptr(), occ_b.data_ptr(),
              B, H, W, float(alpha1), float(alpha2 / scale), mode, _stream(flow_f),
              algo_bytes=24 * B * H * W)
    return occ_f, occ_b


def warp2d_photo(frame, flow):
    """a11: the `backwrd_warp` closure of Flow-2D/model/RIFE.py:244-262."""
    return _Warp2D.apply(frame, flow, None, WARP2D_PHOTO, 0)


def warp2d_dilated(I, flow, start=None):
    """a7: tools.boundary_dilated_warp.warp_im (UPFlow/utils/tools.py:533-541)."""
    return _Warp2D.apply(I, flow, start, WARP2D_DILATED, 0)


# --------------------------------------------------------------------------------------------
# IFNet call site: both frames warped by the two halves of one flow tensor, one launch
# (Flow-3D/model/IFNet.py:190-191, Flow-2D/model/IFNet.py:191-192)
# --------------------------------------------------------------------------------------------
def _check_pair(img0, img1, flow):
    nd = flow.dim() - 2
    if nd not in (2, 3):
        raise ValueError("flow must be [B,4,H,W] or [B,6,D,H,W], got %s" % (tuple(flow.shape),))
    img0 = _need_cuda_f32("img0", img0, nd + 2)
    img1 = _need_cuda_f32("img1", img1, nd + 2)
    flow = _need_cuda_f32("flow", flow, nd + 2)
    if img0.shape != img1.shape:
        raise ValueError("img0 %s and img1 %s differ" % (tuple(img0.shape), tuple(img1.shape)))
    if flow.shape[0] != img0.shape[0] or flow.shape[1] != 2 * nd:
        raise ValueError("flow %s does not match the images %s" %
                         (tuple(flow.shape), tuple(img0.shape)))
    if not (img0.device == img1.device == flow.device):
        raise ValueError("operands are on different devices")
    return img0, img1, flow, nd


def _pair_forward(img0, img1, flow, nd):
    oshape = tuple(img0.shape[:2]) + tuple(flow.shape[2:])  # the warps take the flow's extent
    out0, out1 = img0.new_empty(oshape), img1.new_empty(oshape)
    B, C = img0.shape[:2]
    with torch.cuda.device(flow.device):
        if nd == 3:
            D, H, W = flow.shape[2:]
            mis = (img0.data_ptr() % 16, img1.data_ptr() % 16, flow.data_ptr() % 16)
            sym, fl, fq = _kernel_accounting("warp3d_fwd", mis, B, C, *img0.shape[2:], D, H, W, 0)
            _call("fs_warp3d_pair_fwd", img0.data_ptr(), img1.data_ptr(), flow.data_ptr(),
                  out0.data_ptr(), out1.data_ptr(), B, C, _in_dhw(img0, flow), D, H, W,
                  _stream(flow), algo_bytes=4 * flow.numel() + 8 * out0.numel() * 2, algo_flops=fl, equiv_flops=fq,
                  kernel=sym)
        else:
            H, W = flow.shape[2:]
            _call("fs_warp2d_pair_fwd", img0.data_ptr(), img1.data_ptr(), flow.data_ptr(),
                  out0.data_ptr(), out1.data_ptr(), B, C, _in_hw(img0, flow), H, W,
                  WARP2D_RIFE, _stream(flow), algo_bytes=4 * flow.numel() + 8 * out0.numel() * 2)
    return out0, out1


def _flow_addends(grads, flow):
    """The (pointer, batch stride) pairs fs_*_bwd*3 take for up to three gradients of a [B,C,D,H,W] flow:
    contiguous tensors or channel slices of wider contiguous ones (what `torch.cat`'s backward hands out) go
    through as they are; anything else is made contiguous.  Returns (flat argument list, tensors to keep alive,
    bytes read)."""
    vol = flow.shape[2] * flow.shape[3] * flow.shape[4]
    want_inner = (vol, flow.shape[3] * flow.shape[4], flow.shape[4], 1)
    keep, args, nbytes = [], [], 0
    for g in grads:
        if g is None:
            continue
        g = _need_cuda_f32_strided("grad_flow", g, 5)
        if tuple(g.shape) != tuple(flow.shape):
            raise ValueError("gradient %s does not match the flow %s" % (tuple(g.shape), tuple(flow.shape)))
        if tuple(g.stride()[1:]) != want_inner or g.stride(0) < flow.shape[1] * vol or g.data_ptr() % 16 or g.stride(0) % 4:
            g = g.contiguous()
        keep.append(g)
        args += [g.data_ptr(), int(g.stride(0))]
        nbytes += 4 * g.numel()
    if len(keep) > 3:  # (never in IFNet: three consumers per flow)
        extra = keep[3]
        for g in keep[4:]:
            extra = extra + g
        keep = keep[:2] + [keep[2] + extra]
        args = []
        for g in keep:
            g = g.contiguous()
            args += [g.data_ptr(), int(g.stride(0))]
    while len(args) < 6:
        args += [None, 0]
    return args, keep, nbytes


def _gout_strided(g, like):
    """(tensor, batch stride or 0) of a warped frame's gradient for fs_*_bwd*3: dense, or a channel slice of a wider
    contiguous tensor (torch.cat's backward) handed to the kernel with its batch stride; anything else is copied."""
    vol = like.shape[2] * like.shape[3] * like.shape[4]
    inner = (vol, like.shape[3] * like.shape[4], like.shape[4], 1)
    if g.is_contiguous():
        return g, 0
    if (g.dim() == 5 and tuple(g.stride()[1:]) == inner and g.stride(0) >= g.shape[1] * vol and g.stride(0) % 4 == 0
            and g.data_ptr() % 16 == 0):
        return g, int(g.stride(0))
    return g.contiguous(), 0


def _pair_backward(img0, img1, flow, g0, g1, need_img, need_flow, gflow_add=None):
    """(grad_img0, grad_img1, grad_flow); `gflow_add` (3-D only): a gradient, or a list of up to three, reaching
    the flow from its other consumers, summed into grad_flow by the same launch."""
    if flow.dim() == 5 and gflow_add is not None:
        (g0, s0), (g1, s1) = _gout_strided(g0, flow), _gout_strided(g1, flow)
    else:
        g0, g1, s0, s1 = g0.contiguous(), g1.contiguous(), 0, 0
    gi0 = torch.zeros_like(img0) if need_img else None
    gi1 = torch.zeros_like(img1) if need_img else None
    B, C = img0.shape[:2]
    gflow = None
    with torch.cuda.device(flow.device):
        if flow.dim() == 5:
            D, H, W = flow.shape[2:]
            nb = 8 * flow.numel() + 8 * g0.numel() * 2 + (8 * img0.numel() if need_img else 0)
            mis = (img0.data_ptr() % 16, img1.data_ptr() % 16, flow.data_ptr() % 16)
            sym, fl, fq = _kernel_accounting("warp3d_bwd", mis, B, C, *img0.shape[2:], D, H, W, int(need_img))
            if gflow_add is not None:
                adds = gflow_add if isinstance(gflow_add, (list, tuple)) else [gflow_add]
                aargs, keep, abytes = _flow_addends(adds, flow)
                gflow = torch.empty_like(flow)
                _call("fs_warp3d_pair_bwd_acc3", img0.data_ptr(), img1.data_ptr(), flow.data_ptr(),
                      g0.data_ptr(), s0, g1.data_ptr(), s1, _ptr(gi0), _ptr(gi1), *aargs, gflow.data_ptr(),
                      B, C, _in_dhw(img0, flow), D, H, W, _stream(flow), algo_bytes=nb + abytes, algo_flops=fl,
                      equiv_flops=fq, kernel=sym)
                del keep
            else:
                gflow = torch.empty_like(flow) if need_flow else None
                _call("fs_warp3d_pair_bwd", img0.data_ptr(), img1.data_ptr(), flow.data_ptr(),
                      g0.data_ptr(), g1.data_ptr(), _ptr(gi0), _ptr(gi1), _ptr(gflow), B, C,
                      _in_dhw(img0, flow), D, H, W, _stream(flow), algo_bytes=nb, algo_flops=fl, equiv_flops=fq,
                      kernel=sym)
        else:
            H, W = flow.shape[2:]
            gflow = torch.empty_like(flow) if need_flow else None
            _call("fs_warp2d_pair_bwd", img0.data_ptr(), img1.data_ptr(), flow.data_ptr(),
                  g0.data_ptr(), g1.data_ptr(), _ptr(gi0), _ptr(gi1), _ptr(gflow), B, C,
                  _in_hw(img0, flow), H, W, WARP2D_RIFE, _stream(flow),
                  algo_bytes=4 * flow.numel() * (2 if need_flow else 1) + 8 * g0.numel() * (3 if need_img else 2))
            if gflow_add is not None and gflow is not None:
                for g in (gflow_add if isinstance(gflow_add, (list, tuple)) else [gflow_add]):
                    if g is not None:
                        gflow = gflow + g
    return gi0, gi1, gflow


class _WarpPair(torch.autograd.Function):
    @staticmethod
    def forward(ctx, img0, img1, flow):
        img0, img1, flow, nd = _check_pair(img0, img1, flow)
        out0, out1 = _pair_forward(img0, img1, flow, nd)
        ctx.save_for_backward(img0, img1, flow)
        return out0, out1

    @staticmethod
    def backward(ctx, g0, g1):
        img0, img1, flow = ctx.saved_tensors
        need_img = ctx.needs_input_grad[0] or ctx.needs_input_grad[1]
        need_flow = ctx.needs_input_grad[2]
        if not (need_img or need_flow):
            return None, None, None
        gi0, gi1, gflow = _pair_backward(img0, img1, flow, g0, g1, need_img, need_flow)
        return (gi0 if ctx.needs_input_grad[0] else None, gi1 if ctx.needs_input_grad[1] else None,
                gflow)


class _WarpPairAcc(torch.autograd.Function):
    """(w0, w1, flow_a, flow_b, flow_c) with flow_* three aliases of `flow`: the caller hands ONE alias to each
    of the flow's other consumers (next block's input, next block's accumulation, distillation), so autograd
    delivers their gradients to this node one by one, and the warp's backward launch adds all of them to its own
    result (fs_warp3d_pair_bwd_acc3) -- no autograd `add` over the full-size flow, and the 6-channel slice of the
    next block's 11-channel input gradient is read in place."""

    @staticmethod
    def forward(ctx, img0, img1, flow):
        img0, img1, flow_c, nd = _check_pair(img0, img1, flow)
        out0, out1 = _pair_forward(img0, img1, flow_c, nd)
        ctx.save_for_backward(img0, img1, flow_c)
        ctx.set_materialize_grads(False)
        return out0, out1, flow_c.view_as(flow_c), flow_c.view_as(flow_c), flow_c.view_as(flow_c)

    @staticmethod
    def backward(ctx, g0, g1, ga, gb, gc):
        img0, img1, flow = ctx.saved_tensors
        need_img = ctx.needs_input_grad[0] or ctx.needs_input_grad[1]
        need_flow = ctx.needs_input_grad[2]
        if not (need_img or need_flow):
            return None, None, None
        adds = [g for g in (ga, gb, gc) if g is not None]
        gflow_out = adds if adds else None
        if g0 is None and g1 is None:
            tot = None
            for g in adds:
                tot = g if tot is None else tot + g
            return None, None, (tot if need_flow else None)
        oshape = tuple(img0.shape[:2]) + tuple(flow.shape[2:])
        g0 = flow.new_zeros(oshape) if g0 is None else g0
        g1 = flow.new_zeros(oshape) if g1 is None else g1
        gi0, gi1, gflow = _pair_backward(img0, img1, flow, g0, g1, need_img, need_flow,
                                         gflow_out if need_flow else None)
        return (gi0 if ctx.needs_input_grad[0] else None, gi1 if ctx.needs_input_grad[1] else None,
                gflow)


def warp_pair(img0, img1, flow):
    """(warp(img0, flow[:, :nd]), warp(img1, flow[:, nd:2nd])) in one launch; nd = 2 or 3."""
    if img0.shape[0] == 0 and img1.shape[0] == 0 and flow.shape[0] == 0 and flow.dim() in (4, 5):
        shape = (0, img0.shape[1]) + tuple(flow.shape[2:])
        return _empty_like_graph(shape, img0, flow), _empty_like_graph(shape, img1, flow)
    return _WarpPair.apply(img0, img1, flow)


def warp_pair_acc(img0, img1, flow):
    """warp_pair that also returns the flow for its OTHER consumers: (w0, w1, (flow_a, flow_b, flow_c)).  Use one
    alias per downstream consumer instead of `flow`; the gradients arriving there are folded into the warp's
    backward launch."""
    if img0.shape[0] == 0 and img1.shape[0] == 0 and flow.shape[0] == 0 and flow.dim() in (4, 5):
        return warp_pair(img0, img1, flow) + ((flow, flow, flow),)
    w0, w1, fa, fb, fc = _WarpPairAcc.apply(img0, img1, flow)
    return w0, w1, (fa, fb, fc)


class _UpsampleWarpPair(torch.autograd.Function):
    """flow = prev + scale * trilinear_upsample(delta, factor); (w0, w1) = warp pair with that
    flow -- one kernel forward (fs_upsample_warp3d_pair_fwd), and backward one warp launch that folds in the
    gradient reaching `flow` from its other consumers plus the separable up-sampling adjoint."""

    @staticmethod
    def forward(ctx, img0, img1, delta, prev, factor, scale):
        delta = _need_cuda_f32("delta", delta, 5)
        img0 = _need_cuda_f32("img0", img0, 5)
        img1 = _need_cuda_f32("img1", img1, 5)
        B, C = img0.shape[:2]
        if delta.shape[0] != B or delta.shape[1] != 6 or img0.shape != img1.shape:
            raise ValueError("delta must be [B,6,d,h,w] for images %s / %s, got %s" %
                             (tuple(img0.shape), tuple(img1.shape), tuple(delta.shape)))
        Ds, Hs, Ws = delta.shape[2:]
        full = (B, 6, Ds * factor, Hs * factor, Ws * factor)
        if prev is not None:
            prev = _need_cuda_f32("prev", prev, 5)
            if tuple(prev.shape) != full:
                raise ValueError("prev %s must have the up-sampled shape %s" % (tuple(prev.shape), full))
        flow = delta.new_empty(full)
        out0, out1 = img0.new_empty((B, C) + full[2:]), img0.new_empty((B, C) + full[2:])
        with torch.cuda.device(delta.device):
            _call("fs_upsample_warp3d_pair_fwd", img0.data_ptr(), img1.data_ptr(), delta.data_ptr(), _ptr(prev),
                  flow.data_ptr(), out0.data_ptr(), out1.data_ptr(), B, C, _in_dhw(img0, flow), Ds, Hs, Ws,
                  int(factor), float(scale), _stream(delta),
                  algo_bytes=4 * (delta.numel() + flow.numel() * (2 if prev is not None else 1)) + 8 * out0.numel() * 2)
        ctx.save_for_backward(img0, img1, flow)
        ctx.cfg = (tuple(delta.shape), int(factor), float(scale), prev is not None)
        ctx.set_materialize_grads(False)
        return flow, flow.view_as(flow), flow.view_as(flow), out0, out1

    @staticmethod
    def backward(ctx, gfa, gfb, gfc, g0, g1):
        img0, img1, flow = ctx.saved_tensors
        dshape, factor, scale, has_prev = ctx.cfg
        need_delta, need_prev = ctx.needs_input_grad[2], has_prev and ctx.needs_input_grad[3]
        need_img = ctx.needs_input_grad[0] or ctx.needs_input_grad[1]
        if not (need_delta or need_prev or need_img):
            return (None,) * 6
        B, C = img0.shape[:2]
        Ds, Hs, Ws = dshape[2:]
        D, H, W = flow.shape[2:]
        adds = [g for g in (gfa, gfb, gfc) if g is not None]
        if g0 is None and g1 is None and not adds:
            return (None,) * 6
        oshape = (B, C, D, H, W)
        gi0 = gi1 = None
        if need_img and not (g0 is None and g1 is None):
            # the frames carry no gradient in IFNet, so the fused launch below has no image-gradient output; a caller
            # whose frames do require grad gets them from the plain pair backward (scatter with float atomics)
            gi0, gi1, _ = _pair_backward(img0, img1, flow, flow.new_zeros(oshape) if g0 is None else g0,
                                         flow.new_zeros(oshape) if g1 is None else g1, True, False)
            gi0 = gi0 if ctx.needs_input_grad[0] else None
            gi1 = gi1 if ctx.needs_input_grad[1] else None
        if not (need_delta or need_prev):
            return gi0, gi1, None, None, None, None
        g0, s0 = (flow.new_zeros(oshape), 0) if g0 is None else _gout_strided(g0, flow)
        g1, s1 = (flow.new_zeros(oshape), 0) if g1 is None else _gout_strided(g1, flow)
        aargs, keep, abytes = _flow_addends(adds, flow)
        gtot = torch.empty_like(flow)
        gdelta = flow.new_empty(dshape)
        ws = flow.new_empty(B * 6 * (D * H * Ws + D * Hs * Ws))
        with torch.cuda.device(flow.device):
            _call("fs_upsample_warp3d_pair_bwd3", img0.data_ptr(), img1.data_ptr(), flow.data_ptr(), g0.data_ptr(),
                  s0, g1.data_ptr(), s1, *aargs, gtot.data_ptr(), gdelta.data_ptr(), ws.data_ptr(), B, C,
                  _in_dhw(img0, flow), Ds, Hs, Ws, factor, scale, _stream(flow),
                  algo_bytes=8 * flow.numel() + 8 * g0.numel() * 2 + abytes + 4 * (flow.numel() + gdelta.numel()))
        del keep
        return gi0, gi1, (gdelta if need_delta else None), (gtot if need_prev else None), None, None


def upsample_warp_pair(img0, img1, delta, prev, factor, scale=None):
    """((flow_a, flow_b, flow_c), w0, w1) with flow = prev + scale * F.interpolate(delta, scale_factor=factor,
    trilinear, align_corners=False) (prev may be None; scale defaults to factor, Flow-3D/model/IFNet.py:118) and
    (w0, w1) = warp_pair(img0, img1, flow): IFBlock's flow up-scaling, the running-flow accumulation and the
    two backward warps in one launch.  flow_* are three aliases of the flow, one per downstream consumer (see
    _WarpPairAcc): their gradients are summed inside the backward warp launch."""
    fa, fb, fc, w0, w1 = _UpsampleWarpPair.apply(img0, img1, delta, prev, int(factor),
                                                 float(factor if scale is None else scale))
    return (fa, fb, fc), w0, w1


# --------------------------------------------------------------------------------------------
# a11: photometric term of Flow-2D Model.update (Flow-2D/model/RIFE.py:190-191, 244-279)
# --------------------------------------------------------------------------------------------
def rife2d_photometric(flow4, merged, img0, img1):
    """loss_photo = mean over the two directions of sum_pixels ((warp(merged) - frame)^2 + eps^2)^0.25
    / 3 / B, with `backwrd_warp`'s half-pixel-shifted zero-padded sampling done by the HIP kernel.
    The reference's two F.interpolate calls (:248 merged -> the flow's extent, align_corners=True; :269
    frame -> the warped extent, align_corners=False) are exact identities when the extents agree -- every
    size that is a multiple of 16 -- and are skipped then; for extents where IFNet crops its outputs below
    the input (floor(n/4) % 4 == 0 and n % 4 != 0, e.g. H = 145..147) they are real bilinear resizes."""
    import torch.nn.functional as F
    if merged.shape[2:] != flow4.shape[2:]:
        merged = F.interpolate(merged, size=tuple(flow4.shape[2:]), mode='bilinear', align_corners=True)

    def term(flow2, frame):
        w = warp2d_photo(merged, flow2)
        if frame.shape[2:] != w.shape[2:]:
            frame = F.interpolate(frame, size=tuple(w.shape[2:]), mode='bilinear', align_corners=False)
        # charbonnier(x, 0.25, 1e-9) = (x^2 + 1e-18)^0.25, summed, / 3 / B: one fused penalty+reduction
        return robust_loss(w, frame, None, PEN_CHARBONNIER, 0.25, 1.e-9 ** 2, form="sum") / 3 / frame.size(0)

    return (term(flow4[:, 2:4], img0) + term(flow4[:, :2], img1)) / 2


# --------------------------------------------------------------------------------------------
# a3/a4: local-window correlation (UPFlow/model/correlation_package/correlation.py:8-45)
# --------------------------------------------------------------------------------------------
def corr2d_forward_into(input1, input2, output, max_displacement):
    """correlation_cuda.forward semantics: `output` is resized and filled in place."""
    input1 = _need_cuda_f32("input1", input1, 4)
    input2 = _need_cuda_f32("input2", input2, 4)
    if input1.shape != input2.shape or input1.device != input2.device:
        raise ValueError("input1 %s and input2 %s must match" %
                         (tuple(input1.shape), tuple(input2.shape)))
    B, C, H, W = input1.shape
    nd = 2 * max_displacement + 1
    output.resize_(B, nd * nd, H, W)
    with torch.cuda.device(input1.device):
        _call("fs_corr2d_fwd", input1.data_ptr(), input2.data_ptr(), output.data_ptr(), B, C, H, W,
              int(max_displacement), _stream(input1), algo_bytes=4 * (2 * input1.numel() + output.numel()),
              algo_flops=2 * output.numel() * C)
    return output


def corr2d_backward_into(input1, input2, grad_output, grad_input1, grad_input2, max_displacement):
    """correlation_cuda.backward semantics: grad tensors are resized and filled in place
    (pass None to skip one of them)."""
    input1 = _need_cuda_f32("input1", input1, 4)
    input2 = _need_cuda_f32("input2", input2, 4)
    grad_output = _need_cuda_f32("grad_output", grad_output, 4)
    B, C, H, W = input1.shape
    nd = 2 * max_displacement + 1
    if tuple(grad_output.shape) != (B, nd * nd, H, W):
        raise ValueError("grad_output must be %s, got %s" % ((B, nd * nd, H, W),
                                                             tuple(grad_output.shape)))
    for g in (grad_input1, grad_input2):
        if g is not None:
            g.resize_(B, C, H, W)
    with torch.cuda.device(input1.device):
        _call("fs_corr2d_bwd", input1.data_ptr(), input2.data_ptr(), grad_output.data_ptr(),
              _ptr(grad_input1), _ptr(grad_input2), B, C, H, W, int(max_displacement),
              _stream(input1), algo_bytes=4 * (2 * input1.numel() + grad_output.numel()) + 4 * input1.numel() * sum(
                  1 for g in (grad_input1, grad_input2) if g is not None),
              algo_flops=2 * grad_output.numel() * C * sum(1 for g in (grad_input1, grad_input2) if g is not None))


class _Corr2D(torch.autograd.Function):
    @staticmethod
    def forward(ctx, f1, f2, md):
        out = corr2d_forward_into(f1, f2, f1.new_empty(0), md)
        ctx.save_for_backward(f1.contiguous(), f2.contiguous())
        ctx.md = md
        return out

    @staticmethod
    def backward(ctx, gout):
        f1, f2 = ctx.saved_tensors
        g1 = torch.empty_like(f1) if ctx.needs_input_grad[0] else None
        g2 = torch.empty_like(f2) if ctx.needs_input_grad[1] else None
        if g1 is None and g2 is None:
            return None, None, None
        corr2d_backward_into(f1, f2, gout, g1, g2, ctx.md)
        return g1, g2, None


def corr2d(f1, f2, max_displacement=4):
    """Cost volume [B,(2md+1)^2,H,W] = channel-mean of f1 * shifted f2 (zero padded)."""
    if f1.dim() == 4 and f2.dim() == 4 and f1.shape[0] == 0 and f2.shape[0] == 0:
        nd = 2 * int(max_displacement) + 1
        return _empty_like_graph((0, nd * nd) + tuple(f1.shape[2:]), f1, f2)
    return _Corr2D.apply(f1, f2, int(max_displacement))


class _Corr2DNorm(torch.autograd.Function):
    """§8f.4: corr2d(normalize(f1), normalize(f2)) with per-(b,c)-plane moments, normalisation folded
    into the correlation kernels' tile loads (upflow.py:96-138 + correlation.py:26)."""

    @staticmethod
    def forward(ctx, f1, f2, md):
        f1 = _need_cuda_f32("f1", f1, 4)
        f2 = _need_cuda_f32("f2", f2, 4)
        if f1.shape != f2.shape:
            raise ValueError("f1 %s and f2 %s must match" % (tuple(f1.shape), tuple(f2.shape)))
        B, C, H, W = f1.shape
        if H * W < 2:
            raise ValueError("per-plane variance needs at least two pixels")
        st1, st2 = f1.new_empty(B * C, 2), f1.new_empty(B * C, 2)
        nd = 2 * md + 1
        out = f1.new_empty(B, nd * nd, H, W)
        with torch.cuda.device(f1.device):
            s = _stream(f1)
            _call("fs_plane_moments", f1.data_ptr(), st1.data_ptr(), B * C, H * W, s, algo_bytes=4 * f1.numel())
            _call("fs_plane_moments", f2.data_ptr(), st2.data_ptr(), B * C, H * W, s, algo_bytes=4 * f2.numel())
            _call("fs_corr2d_norm_fwd", f1.data_ptr(), f2.data_ptr(), st1.data_ptr(), st2.data_ptr(),
                  out.data_ptr(), B, C, H, W, md, s, algo_bytes=4 * (2 * f1.numel() + out.numel()))
        ctx.save_for_backward(f1, f2, st1, st2)
        ctx.md = md
        return out

    @staticmethod
    def backward(ctx, gout):
        f1, f2, st1, st2 = ctx.saved_tensors
        B, C, H, W = f1.shape
        gout = _need_cuda_f32("grad_output", gout, 4)
        need1, need2 = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (need1 or need2):
            return None, None, None
        gn1 = torch.empty_like(f1) if need1 else None
        gn2 = torch.empty_like(f2) if need2 else None
        g1 = g2 = None
        with torch.cuda.device(f1.device):
            s = _stream(f1)
            _call("fs_corr2d_norm_bwd", f1.data_ptr(), f2.data_ptr(), st1.data_ptr(), st2.data_ptr(),
                  gout.data_ptr(), _ptr(gn1), _ptr(gn2), B, C, H, W, ctx.md, s,
                  algo_bytes=4 * (2 * f1.numel() + gout.numel()))
            if need1:
                g1 = torch.empty_like(f1)
                _call("fs_plane_norm_bwd", f1.data_ptr(), st1.data_ptr(), gn1.data_ptr(), g1.data_ptr(),
                      B * C, H * W, s, algo_bytes=12 * f1.numel())
            if need2:
                g2 = torch.empty_like(f2)
                _call("fs_plane_norm_bwd", f2.data_ptr(), st2.data_ptr(), gn2.data_ptr(), g2.data_ptr(),
                      B * C, H * W, s, algo_bytes=12 * f2.numel())
        return g1, g2, None


def corr2d_normalized(f1, f2, max_displacement=4):
    """Cost volume of the per-plane centred / scaled feature maps (UPFlow `if_norm_before_cost_volume`
    with moments per channel and per image), without materialising the normalised maps."""
    return _Corr2DNorm.apply(f1, f2, int(max_displacement))


class _Corr2DPair(torch.autograd.Function):
    """Both directions of one UPFlow pyramid level (upflow.py:649, 652) in one launch each way:
    (corr(f1a, f2a), corr(f1b, f2b)); with `normalize` the per-(b,c)-plane normalisation of
    normalize_features (upflow.py:96-138) is folded into the tile loads (§8f.4) and the four moment /
    adjoint passes run as one launch each."""

    @staticmethod
    def forward(ctx, f1a, f2a, f1b, f2b, md, normalize):
        ts = [_need_cuda_f32(n, t, 4) for n, t in (("f1a", f1a), ("f2a", f2a), ("f1b", f1b), ("f2b", f2b))]
        f1a, f2a, f1b, f2b = ts
        if not (f1a.shape == f2a.shape == f1b.shape == f2b.shape):
            raise ValueError("the four feature maps must share one shape, got %s" % ([tuple(t.shape) for t in ts],))
        B, C, H, W = f1a.shape
        nd = 2 * md + 1
        outa, outb = f1a.new_empty(B, nd * nd, H, W), f1a.new_empty(B, nd * nd, H, W)
        stats = None
        with torch.cuda.device(f1a.device):
            s = _stream(f1a)
            if normalize:
                if H * W < 2:
                    raise ValueError("per-plane variance needs at least two pixels")
                stats = f1a.new_empty(4, B * C, 2)
                _call("fs_plane_moments4", f1a.data_ptr(), f2a.data_ptr(), f1b.data_ptr(), f2b.data_ptr(),
                      stats.data_ptr(), B * C, H * W, s, algo_bytes=16 * f1a.numel(), record_as="fs_plane_moments")
            _call("fs_corr2d_pair_fwd", f1a.data_ptr(), f2a.data_ptr(), f1b.data_ptr(), f2b.data_ptr(), _ptr(stats),
                  outa.data_ptr(), outb.data_ptr(), B, C, H, W, md, s,
                  algo_bytes=8 * (2 * f1a.numel() + outa.numel()), algo_flops=4 * outa.numel() * C)
        ctx.save_for_backward(f1a, f2a, f1b, f2b, stats)
        ctx.md = md
        return outa, outb

    @staticmethod
    def backward(ctx, ga, gb):
        f1a, f2a, f1b, f2b, stats = ctx.saved_tensors
        need = ctx.needs_input_grad[:4]
        if not any(need):
            return (None,) * 6
        B, C, H, W = f1a.shape
        nd = 2 * ctx.md + 1
        ga = torch.zeros(B, nd * nd, H, W, device=f1a.device) if ga is None else _need_cuda_f32("grad_output", ga, 4)
        gb = torch.zeros_like(ga) if gb is None else _need_cuda_f32("grad_output", gb, 4)
        gn = [torch.empty_like(f1a) if n else None for n in need]
        with torch.cuda.device(f1a.device):
            s = _stream(f1a)
            _call("fs_corr2d_pair_bwd", f1a.data_ptr(), f2a.data_ptr(), f1b.data_ptr(), f2b.data_ptr(), _ptr(stats),
                  ga.data_ptr(), gb.data_ptr(), _ptr(gn[0]), _ptr(gn[1]), _ptr(gn[2]), _ptr(gn[3]), B, C, H, W,
                  ctx.md, s, algo_bytes=8 * (2 * f1a.numel() + ga.numel()) + 4 * sum(f1a.numel() for n in need if n),
                  algo_flops=4 * ga.numel() * C * sum(1 for n in need[:2] if n))
            if stats is None:
                return tuple(gn) + (None, None)
            gf = [torch.empty_like(f1a) if n else None for n in need]
            _call("fs_plane_norm_bwd4", f1a.data_ptr(), f2a.data_ptr(), f1b.data_ptr(), f2b.data_ptr(),
                  stats.data_ptr(), _ptr(gn[0]), _ptr(gn[1]), _ptr(gn[2]), _ptr(gn[3]), _ptr(gf[0]), _ptr(gf[1]),
                  _ptr(gf[2]), _ptr(gf[3]), B * C, H * W, s, algo_bytes=12 * f1a.numel() * sum(1 for n in need if n),
                  record_as="fs_plane_norm_bwd")
        return tuple(gf) + (None, None)


def corr2d_pair(f1a, f2a, f1b, f2b, max_displacement=4, normalize=False):
    """(corr2d(f1a, f2a), corr2d(f1b, f2b)) -- or their corr2d_normalized forms -- in one launch per pass."""
    return _Corr2DPair.apply(f1a, f2a, f1b, f2b, int(max_displacement), bool(normalize))


# --------------------------------------------------------------------------------------------
# a9/a10: robust penalty + masked reduction (UPFlow/utils/loss.py:17-48, upflow.py:267-289)
# --------------------------------------------------------------------------------------------
PEN_ABS_ROBUST, PEN_CHARBONNIER, PEN_L1_EPS, PEN_L1 = 0, 1, 2, 3
_REDUCE_BLOCKS = 1024


def _flat3(t):
    """[B,C,*spatial] -> (B, C, S) sizes of a contiguous tensor."""
    return t.shape[0], t.shape[1], int(t[0, 0].numel())


class _RobustLoss(torch.autograd.Function):
    """loss = form(S1, S2);  S1 = sum pen(x - y) * w,  S2 = sum w  (one HIP pass)."""

    @staticmethod
    def forward(ctx, x, y, w, mode, q, eps, border, form):
        x = _need_cuda_f32("x", x, x.dim())
        if y is not None:
            y = _need_cuda_f32("y", y, x.dim())
            if y.shape != x.shape:
                raise ValueError("x %s and y %s differ" % (tuple(x.shape), tuple(y.shape)))
        B, C, S = _flat3(x)
        if w is not None:
            w = _need_cuda_f32("mask", w, x.dim())
            if tuple(w.shape) != (B, 1) + tuple(x.shape[2:]):
                raise ValueError("mask must be [B,1,...] matching x %s, got %s" %
                                 (tuple(x.shape), tuple(w.shape)))
        H, W = (x.shape[2], x.shape[3]) if x.dim() == 4 else (1, S)
        sums = x.new_empty(2)
        ws = x.new_empty(2 * _REDUCE_BLOCKS)
        with torch.cuda.device(x.device):
            _call("fs_robust_sum", x.data_ptr(), _ptr(y), _ptr(w), sums.data_ptr(), ws.data_ptr(),
                  B, C, S, H, W, border, mode, float(q), float(eps), _stream(x),
                  algo_bytes=4 * x.numel() * (2 if y is not None else 1))
        S1, S2 = sums[0], sums[1]
        n = float(B * C * S)
        if form == "mean":
            loss, dS1 = S1 / n, torch.full_like(S1, 1.0 / n)  # fill kernel: graph-capturable
        elif form == "sum":
            loss, dS1 = S1 * 1.0, torch.ones_like(S1)
        elif form == "ratio":      # sum(l * w) / (sum(w) + 1e-6)          upflow.py:287
            dS1 = 1.0 / (S2 + 1e-6)
            loss = S1 * dS1
        elif form == "ratio2":     # sum(l * w) / (sum(w) * 2 + 1e-6)      loss.py:39-42
            dS1 = 1.0 / (S2 * 2 + 1e-6)
            loss = S1 * dS1
        elif form == "mean_ratio2":  # mean(l * w) / (mean(w) * 2 + 1e-6)  loss.py:20-29
            dS1 = (1.0 / n) / ((S2 / float(B * S)) * 2 + 1e-6)
            loss = S1 * dS1
        else:
            raise ValueError("unknown reduction form %r" % form)
        ctx.save_for_backward(x, y, w, dS1)
        ctx.cfg = (mode, float(q), float(eps), border)
        return loss

    @staticmethod
    def backward(ctx, gout):
        x, y, w, dS1 = ctx.saved_tensors
        need_x = ctx.needs_input_grad[0]
        need_y = y is not None and ctx.needs_input_grad[1]
        if not (need_x or need_y):
            return (None,) * 8
        mode, q, eps, border = ctx.cfg
        B, C, S = _flat3(x)
        H, W = (x.shape[2], x.shape[3]) if x.dim() == 4 else (1, S)
        coef = (gout * dS1).reshape(1).contiguous()
        gx = torch.empty_like(x) if need_x else None
        gy = torch.empty_like(x) if need_y else None
        with torch.cuda.device(x.device):
            _call("fs_robust_sum_bwd", x.data_ptr(), _ptr(y), _ptr(w), coef.data_ptr(), _ptr(gx),
                  _ptr(gy), B, C, S, H, W, border, mode, q, eps, _stream(x),
                  algo_bytes=4 * x.numel() * ((2 if y is not None else 1) + int(need_x) + int(need_y)))
        return gx, gy, None, None, None, None, None, None


def robust_loss(x, y, mask, mode, q=1.0, eps=0.0, border=0, form="mean"):
    return _RobustLoss.apply(x, y, mask, mode, q, eps, border, form)


def l1_loss(a, b):
    """torch.nn.functional.l1_loss(a, b) (mean) in one fused pass (Flow-3D/model/RIFE.py:132-134)."""
    return robust_loss(a, b, None, PEN_L1, form="mean")


def photo_loss_function(diff, mask, q, charbonnier_or_abs_robust, if_use_occ, averge=True):
    """UPFlow/utils/loss.py:17-48."""
    if charbonnier_or_abs_robust:
        if if_use_occ:
            return robust_loss(diff, None, mask, PEN_CHARBONNIER, q, 1e-6,
                               form="mean_ratio2" if averge else "ratio2")
        return robust_loss(diff, None, None, PEN_CHARBONNIER, q, 1e-8, form="mean" if averge else "sum")
    if if_use_occ:
        return robust_loss(diff, None, mask, PEN_ABS_ROBUST, q, form="ratio2")
    return robust_loss(diff, None, None, PEN_ABS_ROBUST, q, form="mean" if averge else "sum")


def photo_loss_multi_type(x, y, occ_mask, photo_loss_type='abs_robust', photo_loss_delta=0.4,
                          photo_loss_use_occ=False):
    """UPFlow/model/upflow.py:267-289: abs_robust / charbonnier / L1 through fs_robust_sum, SSIM through
    fs_wssim."""
    if photo_loss_type == 'SSIM':
        return weighted_ssim_loss(x, y, occ_mask, photo_loss_use_occ)
    mode, q, eps = {"abs_robust": (PEN_ABS_ROBUST, photo_loss_delta, 0.0),
                    "charbonnier": (PEN_CHARBONNIER, photo_loss_delta, 1e-6),
                    "L1": (PEN_L1_EPS, 1.0, 0.0)}[photo_loss_type]
    if photo_loss_use_occ:
        return robust_loss(x, y, occ_mask, mode, q, eps, form="ratio")
    return robust_loss(x, y, None, mode, q, eps, form="mean")


# --------------------------------------------------------------------------------------------
# a8: census loss (UPFlow/utils/loss.py:51-91)
# --------------------------------------------------------------------------------------------
class _CensusDist(torch.autograd.Function):
    @staticmethod
    def forward(ctx, img1, img2, max_distance):
        img1 = _need_cuda_f32("img1", img1, 4)
        img2 = _need_cuda_f32("img1_warp", img2, 4)
        if img1.shape != img2.shape or img1.shape[1] != 3:
            raise ValueError("census needs two [B,3,H,W] images, got %s and %s" %
                             (tuple(img1.shape), tuple(img2.shape)))
        B, _, H, W = img1.shape
        dist = img1.new_empty(B, 1, H, W)
        with torch.cuda.device(img1.device):
            _call("fs_census_dist_fwd", img1.data_ptr(), img2.data_ptr(), dist.data_ptr(), B, H, W,
                  int(max_distance), _stream(img1), algo_bytes=4 * (2 * img1.numel() + dist.numel()))
        ctx.save_for_backward(img1, img2)
        ctx.md = int(max_distance)
        return dist

    @staticmethod
    def backward(ctx, gdist):
        img1, img2 = ctx.saved_tensors
        n1, n2 = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (n1 or n2):
            return None, None, None
        gdist = gdist.contiguous()
        B, _, H, W = img1.shape
        g1 = torch.empty_like(img1) if n1 else None
        g2 = torch.empty_like(img2) if n2 else None
        with torch.cuda.device(img1.device):
            _call("fs_census_dist_bwd", img1.data_ptr(), img2.data_ptr(), gdist.data_ptr(), _ptr(g1),
                  _ptr(g2), B, H, W, ctx.md, _stream(img1),
                  algo_bytes=4 * (2 * img1.numel() + gdist.numel()) + 4 * img1.numel() * (int(n1) + int(n2)))
        return g1, g2, None


def census_dist(img1, img1_warp, max_distance=3):
    return _CensusDist.apply(img1, img1_warp, max_distance)


def census_loss(img1, img1_warp, mask, q, charbonnier_or_abs_robust, if_use_occ, averge=True,
                max_distance=3):
    """loss_functions.census_loss_torch.  The occ x inner-border mask only matters when
    if_use_occ is set (reference quirk, loss.py:42-47: otherwise it is built and ignored)."""
    dist = census_dist(img1, img1_warp, max_distance)
    if charbonnier_or_abs_robust:
        if if_use_occ:
            return robust_loss(dist, None, mask, PEN_CHARBONNIER, q, 1e-6, border=max_distance,
                               form="mean_ratio2" if averge else "ratio2")
        return robust_loss(dist, None, None, PEN_CHARBONNIER, q, 1e-8, form="mean" if averge else "sum")
    if if_use_occ:
        return robust_loss(dist, None, mask, PEN_ABS_ROBUST, q, border=max_distance, form="ratio2")
    return robust_loss(dist, None, None, PEN_ABS_ROBUST, q, form="mean" if averge else "sum")


# --------------------------------------------------------------------------------------------
# the flow-side unsupervised terms of Flow-3D: census distance and first-order smoothness on volumes
# --------------------------------------------------------------------------------------------
def _census3d_flops(numel, radius):
    """Useful flops of one census launch: about 14 per tap (2 rsq, 1 rcp and the multiply-adds around them)."""
    return 14 * (2 * radius + 1) ** 3 * numel


class _Census3DDist(torch.autograd.Function):
    @staticmethod
    def forward(ctx, vol1, vol2, radius):
        vol1 = _need_cuda_f32("vol1", vol1, 5)
        vol2 = _need_cuda_f32("vol2", vol2, 5)
        if vol1.shape != vol2.shape or vol1.shape[1] != 1:
            raise ValueError("census3d needs two [B,1,D,H,W] volumes, got %s and %s" %
                             (tuple(vol1.shape), tuple(vol2.shape)))
        if radius not in (1, 2, 3):
            raise ValueError("census3d radius must be 1, 2 or 3, got %r" % (radius,))
        B, _, D, H, W = vol1.shape
        dist = torch.empty_like(vol1)
        with torch.cuda.device(vol1.device):
            _call("fs_census3d_dist_fwd", vol1.data_ptr(), vol2.data_ptr(), dist.data_ptr(), B, D, H, W, radius,
                  _stream(vol1), algo_bytes=12 * vol1.numel(), algo_flops=_census3d_flops(vol1.numel(), radius))
        ctx.save_for_backward(vol1, vol2)
        ctx.radius = radius
        return dist

    @staticmethod
    def backward(ctx, gdist):
        vol1, vol2 = ctx.saved_tensors
        n1, n2 = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (n1 or n2):
            return None, None, None
        gdist = gdist.contiguous()
        B, _, D, H, W = vol1.shape
        g1 = torch.empty_like(vol1) if n1 else None
        g2 = torch.empty_like(vol2) if n2 else None
        with torch.cuda.device(vol1.device):
            _call("fs_census3d_dist_bwd", vol1.data_ptr(), vol2.data_ptr(), gdist.data_ptr(), _ptr(g1), _ptr(g2),
                  B, D, H, W, ctx.radius, _stream(vol1), algo_bytes=4 * vol1.numel() * (3 + int(n1) + int(n2)),
                  algo_flops=_census3d_flops(vol1.numel(), ctx.radius))
        return g1, g2, None


def census3d_dist(vol1, vol2, radius=1):
    """Per-voxel soft Hamming distance between the soft ternary transforms of two [B,1,D,H,W] volumes over the
    zero-padded (2 radius + 1)^3 neighbourhood (a8's arithmetic, UPFlow/utils/loss.py:59-71), [B,1,D,H,W]."""
    return _Census3DDist.apply(vol1, vol2, radius)


def census3d_loss(vol1, vol2, radius=1, q=0.4):
    """mean((|dist| + 0.01)^q) over every voxel: a8's robust tail (loss.py:44-48, `photo_loss_use_occ=False`)."""
    return robust_loss(census3d_dist(vol1, vol2, radius), None, None, PEN_ABS_ROBUST, q, form="mean")


class _FlowSmooth3D(torch.autograd.Function):
    @staticmethod
    def forward(ctx, flow, guide, q, eps, kappa):
        flow = _need_cuda_f32("flow", flow, 5)
        B, C, D, H, W = flow.shape
        if guide is not None:
            guide = _need_cuda_f32("guide", guide, 5)
            if tuple(guide.shape) != (B, 1, D, H, W):
                raise ValueError("guide must be [B,1,D,H,W] matching flow %s, got %s" %
                                 (tuple(flow.shape), tuple(guide.shape)))
        if not (q > 0 and eps > 0 and kappa >= 0):
            raise ValueError("flow_smooth3d needs q > 0, eps > 0 and kappa >= 0, got %r, %r, %r" % (q, eps, kappa))
        if flow.numel() == 0:
            raise ValueError("flow_smooth3d needs a non-empty flow, got %s" % (tuple(flow.shape),))
        if kappa == 0:
            guide = None
        sums = flow.new_empty(2)
        ws = flow.new_empty(2 * _REDUCE_BLOCKS)
        nbytes = 4 * (flow.numel() + (0 if guide is None else guide.numel()))
        with torch.cuda.device(flow.device):
            _call("fs_flow_smooth3d_fwd", flow.data_ptr(), _ptr(guide), sums.data_ptr(), ws.data_ptr(), B, C, D, H, W,
                  float(q), float(eps), float(kappa), _stream(flow), algo_bytes=nbytes)
        # mean over the pairs counted; a flow of one voxel has none and a loss of 0
        inv = 1.0 / sums[1].clamp(min=1.0)
        ctx.save_for_backward(flow, guide, inv)
        ctx.cfg = (float(q), float(eps), float(kappa), nbytes)
        return sums[0] * inv

    @staticmethod
    def backward(ctx, gout):
        flow, guide, inv = ctx.saved_tensors
        if not ctx.needs_input_grad[0]:
            return (None,) * 5
        q, eps, kappa, nbytes = ctx.cfg
        B, C, D, H, W = flow.shape
        coef = (gout * inv).reshape(1).contiguous()
        gflow = torch.empty_like(flow)
        with torch.cuda.device(flow.device):
            _call("fs_flow_smooth3d_bwd", flow.data_ptr(), _ptr(guide), coef.data_ptr(), gflow.data_ptr(), B, C, D, H,
                  W, q, eps, kappa, _stream(flow), algo_bytes=nbytes + 4 * flow.numel())
        return gflow, None, None, None, None


def flow_smooth3d(flow, guide=None, q=0.25, eps=1e-9, kappa=0.0):
    """First-order smoothness of a [B,C,D,H,W] flow: the mean over channels, voxels p and axes a with p + e_a inside
    of w_a(p) * ((flow[p + e_a] - flow[p])^2 + eps^2)^q, w_a(p) = exp(-kappa |guide[p + e_a] - guide[p]|)
    (`guide` [B,1,D,H,W], no gradient; None or kappa = 0: unweighted).  One HIP pass each way."""
    return _FlowSmooth3D.apply(flow, guide, q, eps, kappa)


# --------------------------------------------------------------------------------------------
# a12: IFNet epilogues
# --------------------------------------------------------------------------------------------
class _Merge(torch.autograd.Function):
    @staticmethod
    def forward(ctx, w0, w1, m):
        w0 = _need_cuda_f32("warped_img0", w0, w0.dim())
        w1 = _need_cuda_f32("warped_img1", w1, w0.dim())
        m = _need_cuda_f32("mask", m, w0.dim())
        B, C, S = _flat3(w0)
        if w1.shape != w0.shape or tuple(m.shape) != (B, 1) + tuple(w0.shape[2:]):
            raise ValueError("merge operands mismatch: %s %s %s" %
                             (tuple(w0.shape), tuple(w1.shape), tuple(m.shape)))
        merged, sig = torch.empty_like(w0), torch.empty_like(m)
        with torch.cuda.device(w0.device):
            _call("fs_merge_fwd", w0.data_ptr(), w1.data_ptr(), m.data_ptr(), merged.data_ptr(),
                  sig.data_ptr(), B, C, S, _stream(w0), algo_bytes=4 * (3 * w0.numel() + 2 * m.numel()))
        ctx.save_for_backward(w0, w1, m)
        # the sigmoid output usually has no consumer with a gradient (Flow-3D returns it, no loss reads it): an
        # undefined gradient stays None instead of a zero-filled tensor the kernel would then read
        ctx.set_materialize_grads(False)
        return merged, sig

    @staticmethod
    def backward(ctx, gmerged, gsig):
        w0, w1, m = ctx.saved_tensors
        n0, n1, nm = ctx.needs_input_grad
        if not (n0 or n1 or nm) or (gmerged is None and gsig is None):
            return None, None, None
        B, C, S = _flat3(w0)
        gmerged = torch.zeros_like(w0) if gmerged is None else gmerged.contiguous()
        gsig = gsig.contiguous() if gsig is not None else None
        g0 = torch.empty_like(w0) if n0 else None
        g1 = torch.empty_like(w1) if n1 else None
        gm = torch.empty_like(m) if nm else None
        with torch.cuda.device(w0.device):
            _call("fs_merge_bwd", w0.data_ptr(), w1.data_ptr(), m.data_ptr(), gmerged.data_ptr(),
                  _ptr(gsig), _ptr(g0), _ptr(g1), _ptr(gm), B, C, S, _stream(w0),
                  algo_bytes=4 * ((3 + int(n0) + int(n1)) * w0.numel() + (1 + int(gsig is not None) + int(nm)) * m.numel()))
        return g0, g1, gm


def merge(warped_img0, warped_img1, mask_logit):
    """(merged, sigmoid(mask)) with merged = w0 * sigmoid(m) + w1 * (1 - sigmoid(m))."""
    return _Merge.apply(warped_img0, warped_img1, mask_logit)


class _Distill(torch.autograd.Function):
    @staticmethod
    def forward(ctx, merged_i, merged_tea, gt, flow_i, flow_tea):
        d = merged_i.dim()
        ts = [_need_cuda_f32(n, t, d) for n, t in (("merged", merged_i), ("merged_teacher", merged_tea),
                                                    ("gt", gt), ("flow", flow_i),
                                                    ("flow_teacher", flow_tea))]
        merged_i, merged_tea, gt, flow_i, flow_tea = ts
        B, C, S = _flat3(merged_i)
        F_ = flow_i.shape[1]
        if not (merged_tea.shape == merged_i.shape == gt.shape and flow_tea.shape == flow_i.shape
                and flow_i.shape[2:] == merged_i.shape[2:]):
            raise ValueError("distill operands mismatch")
        sums = merged_i.new_empty(2)
        ws = merged_i.new_empty(2 * _REDUCE_BLOCKS)
        with torch.cuda.device(merged_i.device):
            _call("fs_distill_fwd", merged_i.data_ptr(), merged_tea.data_ptr(), gt.data_ptr(),
                  flow_i.data_ptr(), flow_tea.data_ptr(), sums.data_ptr(), ws.data_ptr(), B, C, F_, S,
                  _stream(merged_i), algo_bytes=4 * (3 * merged_i.numel() + 2 * flow_i.numel()))
        ctx.save_for_backward(merged_i, merged_tea, gt, flow_i, flow_tea)
        return sums[0] / float(B * S)

    @staticmethod
    def backward(ctx, gout):
        merged_i, merged_tea, gt, flow_i, flow_tea = ctx.saved_tensors
        if not ctx.needs_input_grad[3]:
            return (None,) * 5
        B, C, S = _flat3(merged_i)
        F_ = flow_i.shape[1]
        coef = (gout / float(B * S)).reshape(1).contiguous()
        gf = torch.empty_like(flow_i)
        with torch.cuda.device(merged_i.device):
            _call("fs_distill_bwd", merged_i.data_ptr(), merged_tea.data_ptr(), gt.data_ptr(),
                  flow_i.data_ptr(), flow_tea.data_ptr(), coef.data_ptr(), gf.data_ptr(), B, C, F_, S,
                  _stream(merged_i), algo_bytes=4 * (3 * merged_i.numel() + 3 * flow_i.numel()))
        return None, None, None, gf, None


class _Distill3(torch.autograd.Function):
    """Sum of the three student blocks' distillation terms in one launch each way (fs_distill3_*)."""

    @staticmethod
    def forward(ctx, m0, m1, m2, merged_tea, gt, f0, f1, f2, flow_tea):
        d = m0.dim()
        ms = [_need_cuda_f32("merged", t, d) for t in (m0, m1, m2)]
        fl = [_need_cuda_f32("flow", t, d) for t in (f0, f1, f2)]
        merged_tea, gt = _need_cuda_f32("merged_teacher", merged_tea, d), _need_cuda_f32("gt", gt, d)
        flow_tea = _need_cuda_f32("flow_teacher", flow_tea, d)
        B, C, S = _flat3(ms[0])
        F_ = fl[0].shape[1]
        if not (all(t.shape == ms[0].shape for t in ms + [merged_tea, gt]) and
                all(t.shape == fl[0].shape for t in fl + [flow_tea]) and fl[0].shape[2:] == ms[0].shape[2:]):
            raise ValueError("distill operands mismatch")
        sums = ms[0].new_empty(4)
        ws = ms[0].new_empty(4 * _REDUCE_BLOCKS)
        with torch.cuda.device(ms[0].device):
            _call("fs_distill3_fwd", ms[0].data_ptr(), ms[1].data_ptr(), ms[2].data_ptr(), merged_tea.data_ptr(),
                  gt.data_ptr(), fl[0].data_ptr(), fl[1].data_ptr(), fl[2].data_ptr(), flow_tea.data_ptr(),
                  sums.data_ptr(), ws.data_ptr(), B, C, F_, S, _stream(ms[0]),
                  algo_bytes=4 * (5 * ms[0].numel() + 4 * fl[0].numel()), record_as="fs_distill_fwd")
        ctx.save_for_backward(*ms, merged_tea, gt, *fl, flow_tea)
        n = float(B * S)
        return (0 + sums[0] / n) + sums[1] / n + sums[2] / n  # the order of IFNet.forward's running sum

    @staticmethod
    def backward(ctx, gout):
        m0, m1, m2, merged_tea, gt, f0, f1, f2, flow_tea = ctx.saved_tensors
        if not any(ctx.needs_input_grad[5:8]):
            return (None,) * 9
        B, C, S = _flat3(m0)
        F_ = f0.shape[1]
        coef = (gout / float(B * S)).reshape(1).contiguous()
        g = [torch.empty_like(f0) for _ in range(3)]
        with torch.cuda.device(m0.device):
            _call("fs_distill3_bwd", m0.data_ptr(), m1.data_ptr(), m2.data_ptr(), merged_tea.data_ptr(),
                  gt.data_ptr(), f0.data_ptr(), f1.data_ptr(), f2.data_ptr(), flow_tea.data_ptr(), coef.data_ptr(),
                  g[0].data_ptr(), g[1].data_ptr(), g[2].data_ptr(), B, C, F_, S, _stream(m0),
                  algo_bytes=4 * (5 * m0.numel() + 7 * f0.numel()), record_as="fs_distill_bwd")
        return (None, None, None, None, None) + tuple(g[i] if ctx.needs_input_grad[5 + i] else None
                                                      for i in range(3)) + (None,)


def distill_terms3(merged, merged_teacher, gt, flows, flow_teacher):
    """sum_i distill_term(merged[i], merged_teacher, gt, flows[i], flow_teacher) for the three student blocks
    in one launch each way; the operands of the three terms must share their shapes."""
    return _Distill3.apply(merged[0], merged[1], merged[2], merged_teacher, gt, flows[0], flows[1], flows[2],
                           flow_teacher)


def distill_term(merged_i, merged_teacher, gt, flow_i, flow_teacher):
    """One block's term of loss_distill; gradient reaches flow_i only (the reference detaches the
    teacher flow and the loss mask)."""
    return _Distill.apply(merged_i, merged_teacher, gt, flow_i, flow_teacher)


# --------------------------------------------------------------------------------------------
# §8f.1: trilinear resize of IFBlock with a gather-formulated HIP backward
# --------------------------------------------------------------------------------------------
# --------------------------------------------------------------------------------------------
# §8f.3: Flow-2D/model/laplacian.py:49-88 LapLoss as one pyramid of (input - target)
# --------------------------------------------------------------------------------------------
def _lap_sizes(N, H, W, levels):
    import ctypes
    a, b, c = ctypes.c_longlong(0), ctypes.c_longlong(0), ctypes.c_longlong(0)
    code = _lib.lib().fs_laploss2d_sizes(N, H, W, levels, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c))
    if code != 0:
        raise ValueError("LapLoss needs every pyramid level >= 3 px per side (reflect padding by 2) and "
                         "1 <= levels <= 8; got [%d,%d,%d], %d levels" % (N, H, W, levels))
    return a.value, b.value, c.value


class _LapLoss2D(torch.autograd.Function):
    @staticmethod
    def forward(ctx, inp, target, levels):
        inp = _need_cuda_f32("input", inp, 4)
        target = _need_cuda_f32("target", target, 4)
        if inp.shape != target.shape:
            raise ValueError("input %s and target %s differ in shape" % (tuple(inp.shape), tuple(target.shape)))
        B, C, H, W = inp.shape
        n_sgn, n_fwd, n_bwd = _lap_sizes(B * C, H, W, levels)
        sgn = inp.new_empty(n_sgn)
        ws = inp.new_empty(n_fwd)
        loss = inp.new_empty(2)
        with torch.cuda.device(inp.device):
            _call("fs_laploss2d_fwd", inp.data_ptr(), target.data_ptr(), sgn.data_ptr(), ws.data_ptr(),
                  loss.data_ptr(), B * C, H, W, levels, _stream(inp), algo_bytes=8 * inp.numel())
        ctx.save_for_backward(sgn)
        ctx.cfg = (B, C, H, W, levels, n_bwd)
        return loss[0]

    @staticmethod
    def backward(ctx, gloss):
        (sgn,) = ctx.saved_tensors
        B, C, H, W, levels, n_bwd = ctx.cfg
        gl = gloss.detach().to(torch.float32).reshape(1).contiguous()
        ws = sgn.new_empty(n_bwd)
        gd = sgn.new_empty((B, C, H, W))
        with torch.cuda.device(sgn.device):
            _call("fs_laploss2d_bwd", sgn.data_ptr(), gl.data_ptr(), ws.data_ptr(), gd.data_ptr(), B * C, H, W,
                  levels, _stream(sgn), algo_bytes=8 * gd.numel())
        gi = gd if ctx.needs_input_grad[0] else None
        gt = -gd if ctx.needs_input_grad[1] else None
        return gi, gt, None


def laploss2d(inp, target, max_levels=5):
    """LapLoss(max_levels)(input, target) of Flow-2D/model/laplacian.py:76-88 (scalar)."""
    return _LapLoss2D.apply(inp, target, int(max_levels))


class _LapLoss3D(torch.autograd.Function):
    """3-D Laplacian-pyramid L1 loss (csrc/laplacian3d.hip): the 3-D analogue of Flow-2D's LapLoss.  PARITY
    UNPINNED -- the reference's Flow-3D/model/laplacian.py is dead code with a CPU scipy round trip and no
    gradient through the pyramid; the oracle is this build's own restatement."""

    @staticmethod
    def forward(ctx, inp, target, levels):
        inp = _need_cuda_f32("input", inp, 5)
        target = _need_cuda_f32("target", target, 5)
        if inp.shape != target.shape:
            raise ValueError("input %s and target %s differ in shape" % (tuple(inp.shape), tuple(target.shape)))
        B, C, D, H, W = inp.shape
        a, b, c = ctypes.c_longlong(0), ctypes.c_longlong(0), ctypes.c_longlong(0)
        if _lib.lib().fs_laploss3d_sizes(B * C, D, H, W, levels, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)):
            raise ValueError("LapLoss needs every pyramid level >= 3 voxels per side (reflect padding by 2) and "
                             "1 <= levels <= 8; got %s, %d levels" % (tuple(inp.shape), levels))
        sgn, ws, loss = inp.new_empty(a.value), inp.new_empty(b.value), inp.new_empty(2)
        with torch.cuda.device(inp.device):
            _call("fs_laploss3d_fwd", inp.data_ptr(), target.data_ptr(), sgn.data_ptr(), ws.data_ptr(),
                  loss.data_ptr(), B * C, D, H, W, levels, _stream(inp), algo_bytes=8 * inp.numel())
        ctx.save_for_backward(sgn)
        ctx.cfg = (tuple(inp.shape), levels, c.value)
        return loss[0]

    @staticmethod
    def backward(ctx, gloss):
        (sgn,) = ctx.saved_tensors
        shape, levels, n_bwd = ctx.cfg
        B, C, D, H, W = shape
        gl = gloss.detach().to(torch.float32).reshape(1).contiguous()
        ws, gd = sgn.new_empty(n_bwd), sgn.new_empty(shape)
        with torch.cuda.device(sgn.device):
            _call("fs_laploss3d_bwd", sgn.data_ptr(), gl.data_ptr(), ws.data_ptr(), gd.data_ptr(), B * C, D, H, W,
                  levels, _stream(sgn), algo_bytes=8 * gd.numel())
        return (gd if ctx.needs_input_grad[0] else None), (-gd if ctx.needs_input_grad[1] else None), None


def laploss3d(inp, target, max_levels=5):
    """3-D LapLoss(max_levels)(input, target) (scalar); see _LapLoss3D for its parity status."""
    return _LapLoss3D.apply(inp, target, int(max_levels))


class _Interp3D(torch.autograd.Function):
    """mul * F.interpolate(x, scale_factor = factor or 1/factor, trilinear, align_corners=False): HIP forward
    (ATen's arithmetic, bit-identical) and gather-form HIP backward."""

    @staticmethod
    def forward(ctx, x, factor, up, mul):
        x = _need_cuda_f32("x", x, 5)
        B, C, Di, Hi, Wi = x.shape
        with torch.cuda.device(x.device):
            if up:
                y = x.new_empty((B, C, Di * factor, Hi * factor, Wi * factor))
                _call("fs_upsample3d_scale_add", x.data_ptr(), 0, y.data_ptr(), B, C, Di, Hi, Wi, int(factor),
                      float(mul), _stream(x), algo_bytes=4 * (x.numel() + y.numel()))
            else:
                if min(Di, Hi, Wi) // factor < 1:
                    raise ValueError("input %s is too small to be down-sampled by %d" % (tuple(x.shape), factor))
                y = x.new_empty((B, C, Di // factor, Hi // factor, Wi // factor))
                _call("fs_downsample3d_fwd", x.data_ptr(), y.data_ptr(), B, C, Di, Hi, Wi, int(factor), float(mul),
                      _stream(x), algo_bytes=4 * (x.numel() + y.numel()))
        ctx.cfg = (tuple(x.shape), int(factor), bool(up), float(mul))
        return y

    @staticmethod
    def backward(ctx, gy):
        shape, factor, up, mul = ctx.cfg
        gy = _need_cuda_f32("grad_output", gy, 5)
        gx = gy.new_empty(shape)
        B, C, Di, Hi, Wi = shape
        Do, Ho, Wo = gy.shape[2:]
        ws = gy.new_empty(B * C * (Do * Ho * Wi + Do * Hi * Wi)) if up else None
        with torch.cuda.device(gy.device):
            if up:
                _call("fs_interp3d_bwd_scaled", gy.data_ptr(), gx.data_ptr(), ws.data_ptr(), B, C, Di, Hi, Wi, Do,
                      Ho, Wo, factor, 1, mul, _stream(gy), algo_bytes=4 * (gy.numel() + gx.numel()),
                      record_as="fs_interp3d_bwd")
            else:
                # the exact float4 form takes the scale itself; the general forms need a separate pass
                fold = (mul != 1.0 and (Di, Hi, Wi) == (Do * factor, Ho * factor, Wo * factor) and Wi % 4 == 0
                        and gx.data_ptr() % 16 == 0)
                _call("fs_interp3d_bwd_scaled", gy.data_ptr(), gx.data_ptr(), 0, B, C, Di, Hi, Wi, Do, Ho, Wo,
                      factor, 0, float(mul) if fold else 1.0, _stream(gy), algo_bytes=4 * (gy.numel() + gx.numel()),
                      record_as="fs_interp3d_bwd")
                if mul != 1.0 and not fold:
                    gx.mul_(mul)
        return gx, None, None, None


class _DownsampleCat(torch.autograd.Function):
    """F.interpolate(torch.cat(pieces, 1), scale_factor=1/factor, trilinear) without the concatenation
    (fs_downsample3d_fwd_ms reads every channel where it lies); backward: the adjoint over the concatenated
    gradient, handed out as channel slices as torch.cat's backward would."""

    @staticmethod
    def forward(ctx, factor, *pieces):
        planes = _channel_planes(pieces)
        x0 = pieces[0]
        B, (Di, Hi, Wi) = x0.shape[0], x0.shape[2:]
        if planes is None or min(Di, Hi, Wi) // factor < 1:
            raise ValueError("pieces cannot be read in place")  # (interpolate3d_cat checks first)
        pv, sv, C = planes
        y = x0.new_empty((B, C, Di // factor, Hi // factor, Wi // factor))
        with torch.cuda.device(x0.device):
            _call("fs_downsample3d_fwd_ms", pv, sv, y.data_ptr(), B, C, Di, Hi, Wi, int(factor), 1.0, _stream(x0),
                  algo_bytes=4 * (B * C * Di * Hi * Wi + y.numel()), record_as="fs_downsample3d_fwd")
        ctx.cfg = ((B, C, Di, Hi, Wi), int(factor), [int(t.shape[1]) for t in pieces])
        return y

    @staticmethod
    def backward(ctx, gy):
        shape, factor, splits = ctx.cfg
        gy = _need_cuda_f32("grad_output", gy, 5)
        gx = gy.new_empty(shape)
        B, C, Di, Hi, Wi = shape
        Do, Ho, Wo = gy.shape[2:]
        with torch.cuda.device(gy.device):
            _call("fs_interp3d_bwd_scaled", gy.data_ptr(), gx.data_ptr(), 0, B, C, Di, Hi, Wi, Do, Ho, Wo, factor, 0, 1.0,
                  _stream(gy), algo_bytes=4 * (gy.numel() + gx.numel()), record_as="fs_interp3d_bwd")
        need = ctx.needs_input_grad[1:]
        return (None,) + tuple(g if n else None for g, n in zip(gx.split(splits, 1), need))


def interpolate3d_cat(pieces, factor):
    """F.interpolate(torch.cat(pieces, 1), scale_factor=1/factor, mode="trilinear", align_corners=False) for
    factor 2 / 4 with the pieces read in place, or None when they cannot be (the caller concatenates)."""
    if factor not in (2, 4) or _channel_planes(pieces) is None or min(pieces[0].shape[2:]) // factor < 1:
        return None
    return _DownsampleCat.apply(int(factor), *pieces)


class _UpsampleScaleAdd(torch.autograd.Function):
    @staticmethod
    def forward(ctx, small, prev, factor, scale):
        small = _need_cuda_f32("small", small, 5)
        B, C, Di, Hi, Wi = small.shape
        out_shape = (B, C, Di * factor, Hi * factor, Wi * factor)
        if prev is not None:
            prev = _need_cuda_f32("prev", prev, 5)
            if tuple(prev.shape) != out_shape:
                raise ValueError("prev %s must have the up-sampled shape %s" % (tuple(prev.shape), out_shape))
        out = small.new_empty(out_shape)
        with torch.cuda.device(small.device):
            _call("fs_upsample3d_scale_add", small.data_ptr(), _ptr(prev), out.data_ptr(), B, C, Di, Hi, Wi,
                  int(factor), float(scale), _stream(small),
                  algo_bytes=4 * (small.numel() + out.numel() * (2 if prev is not None else 1)))
        ctx.cfg = (tuple(small.shape), int(factor), float(scale), prev is not None)
        return out

    @staticmethod
    def backward(ctx, gout):
        shape, factor, scale, has_prev = ctx.cfg
        gout = _need_cuda_f32("grad_output", gout, 5)
        gs = None
        if ctx.needs_input_grad[0]:
            gs = gout.new_empty(shape)
            B, C, Di, Hi, Wi = shape
            Do, Ho, Wo = gout.shape[2:]
            ws = gout.new_empty(B * C * (Do * Ho * Wi + Do * Hi * Wi))
            with torch.cuda.device(gout.device):
                _call("fs_interp3d_bwd_scaled", gout.data_ptr(), gs.data_ptr(), ws.data_ptr(), B, C, Di, Hi, Wi, Do,
                      Ho, Wo, factor, 1, scale, _stream(gout), algo_bytes=4 * (gout.numel() + gs.numel()),
                      record_as="fs_interp3d_bwd")
        gp = gout if (has_prev and ctx.needs_input_grad[1]) else None
        return gs, gp, None, None


def upsample3d_scale_add(small, prev, factor, scale=1.0):
    """prev + scale * F.interpolate(small, scale_factor=factor, trilinear, align_corners=False) in one pass
    (IFBlock's flow / mask accumulation); prev may be None."""
    return _UpsampleScaleAdd.apply(small, prev, int(factor), float(scale))


def _int_factor(scale_factor):
    for f in (2, 4):
        if scale_factor == f:
            return f, True
        if scale_factor == 1.0 / f:
            return f, False
    return None, None


def interpolate3d(x, scale_factor, mul=1.0):
    """mul * F.interpolate(x, scale_factor, mode="trilinear", align_corners=False) for the IFBlock factors
    (4, 2, 1/2, 1/4) on the HIP kernels (forward and backward); other factors / dtypes: stock autograd."""
    f, up = _int_factor(scale_factor)
    if f is not None and x.is_cuda and x.dtype == torch.float32 and x.dim() == 5 and \
            (up or min(x.shape[2:]) // f >= 1):
        return _Interp3D.apply(x, f, up, float(mul))
    y = torch.nn.functional.interpolate(x, scale_factor=scale_factor, mode="trilinear",
                                        align_corners=False, recompute_scale_factor=False)
    return y if mul == 1.0 else y * mul


class _Interp2D(torch.autograd.Function):
    """mul * F.interpolate(x, scale_factor = factor or 1/factor, bilinear, align_corners=False) of the 2-D
    IFBlock (Flow-2D/model/IFNet.py:89, 92, 115-116): fs_resize2d_fwd / fs_resize2d_bwd."""

    @staticmethod
    def forward(ctx, x, factor, up, mul):
        x = _need_cuda_f32("x", x, 4)
        B, C, Hi, Wi = x.shape
        Ho, Wo = (Hi * factor, Wi * factor) if up else (Hi // factor, Wi // factor)
        if min(Ho, Wo) < 1:
            raise ValueError("input %s is too small to be down-sampled by %d" % (tuple(x.shape), factor))
        y = x.new_empty((B, C, Ho, Wo))
        with torch.cuda.device(x.device):
            _call("fs_resize2d_fwd", x.data_ptr(), y.data_ptr(), B, C, Hi, Wi, Ho, Wo, int(factor), int(up),
                  float(mul), _stream(x), algo_bytes=4 * (x.numel() + y.numel()))
        ctx.cfg = (tuple(x.shape), int(factor), bool(up), float(mul))
        return y

    @staticmethod
    def backward(ctx, gy):
        shape, factor, up, mul = ctx.cfg
        gy = _need_cuda_f32("grad_output", gy, 4)
        B, C, Hi, Wi = shape
        gx = gy.new_empty(shape)
        with torch.cuda.device(gy.device):
            _call("fs_resize2d_bwd", gy.data_ptr(), gx.data_ptr(), B, C, Hi, Wi, gy.shape[2], gy.shape[3], factor,
                  int(up), mul, _stream(gy), algo_bytes=4 * (gy.numel() + gx.numel()))
        return gx, None, None, None


def interpolate2d(x, scale_factor, mul=1.0):
    """mul * F.interpolate(x, scale_factor, mode="bilinear", align_corners=False) for the IFBlock factors on
    the HIP kernels; other factors / dtypes: stock autograd."""
    f, up = _int_factor(scale_factor)
    if f is not None and x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and \
            (up or min(x.shape[2:]) // f >= 1):
        return _Interp2D.apply(x, f, up, float(mul))
    y = torch.nn.functional.interpolate(x, scale_factor=scale_factor, mode="bilinear", align_corners=False,
                                        recompute_scale_factor=False)
    return y if mul == 1.0 else y * mul


# --------------------------------------------------------------------------------------------
# PReLU after every IFNet convolution: ATen forward, one-pass HIP backward
# --------------------------------------------------------------------------------------------
_PRELU_MAX_CHUNKS = 64


def prelu_backward(x, gy, weight, want_bias_grad=False):
    """fs_prelu_bwd: (grad_x, grad_weight, grad_bias or None) of y = prelu(x, weight) in one pass over
    [B,C,*]; grad_bias = per-channel sum of grad_x (the producing convolution's bias gradient)."""
    x = _need_cuda_f32("x", x, x.dim())
    gy = _need_cuda_f32("grad_output", gy, x.dim())
    B, C, S = _flat3(x)
    gx = torch.empty_like(x)
    gw = torch.empty_like(weight)
    gb = x.new_empty(C) if want_bias_grad else None
    ws = x.new_empty((2 if want_bias_grad else 1) * B * C * _PRELU_MAX_CHUNKS)
    with torch.cuda.device(x.device):
        _call("fs_prelu_bwd", x.data_ptr(), gy.data_ptr(), weight.data_ptr(), gx.data_ptr(),
              gw.data_ptr(), _ptr(gb), ws.data_ptr(), B, C, S, weight.numel(), _stream(x),
              algo_bytes=12 * x.numel())
    return gx, gw, gb


class _PReLU(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight):
        y = torch.nn.functional.prelu(x, weight)
        ctx.save_for_backward(x, weight)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, weight = ctx.saved_tensors
        gx, gw, _ = prelu_backward(x, gy, weight)
        return gx, gw


def prelu(x, weight):
    return _PReLU.apply(x, weight)


# --------------------------------------------------------------------------------------------
# 3-D correlation (new capability; no reference implementation exists)
# --------------------------------------------------------------------------------------------
class _Corr3D(torch.autograd.Function):
    @staticmethod
    def forward(ctx, f1, f2, md):
        f1 = _need_cuda_f32("f1", f1, 5)
        f2 = _need_cuda_f32("f2", f2, 5)
        if f1.shape != f2.shape or f1.device != f2.device:
            raise ValueError("f1 %s and f2 %s must match" % (tuple(f1.shape), tuple(f2.shape)))
        B, C, D, H, W = f1.shape
        nd = 2 * md + 1
        out = f1.new_empty(B, nd ** 3, D, H, W)
        with torch.cuda.device(f1.device):
            _call("fs_corr3d_fwd", f1.data_ptr(), f2.data_ptr(), out.data_ptr(), B, C, D, H, W, md,
                  _stream(f1), algo_bytes=4 * (2 * f1.numel() + out.numel()))
        ctx.save_for_backward(f1, f2)
        ctx.md = md
        return out

    @staticmethod
    def backward(ctx, gout):
        f1, f2 = ctx.saved_tensors
        g1 = torch.empty_like(f1) if ctx.needs_input_grad[0] else None
        g2 = torch.empty_like(f2) if ctx.needs_input_grad[1] else None
        if g1 is None and g2 is None:
            return None, None, None
        gout = _need_cuda_f32("grad_output", gout, 5)
        B, C, D, H, W = f1.shape
        with torch.cuda.device(f1.device):
            _call("fs_corr3d_bwd", f1.data_ptr(), f2.data_ptr(), gout.data_ptr(), _ptr(g1), _ptr(g2), B, C,
                  D, H, W, ctx.md, _stream(f1))
        return g1, g2, None


def corr3d(f1, f2, max_displacement=4):
    """Volume cost volume [B,(2md+1)^3,D,H,W]: channel-mean of f1 * shifted f2, zero padded, dz-major."""
    return _Corr3D.apply(f1, f2, int(max_displacement))


# --------------------------------------------------------------------------------------------
# IFNet-3D convolution weight gradient: implicit GEMM on the fp32 matrix cores
# --------------------------------------------------------------------------------------------
# --------------------------------------------------------------------------------------------
# Prepared convolution weights: one re-layout launch per optimiser step instead of one per convolution
# --------------------------------------------------------------------------------------------
# fs_conv3d_fwd* / fs_conv3d_tr* re-lay their weights into a slab (`ws`) with a ~5 us launch in front of every
# convolution: ~110 launches + dispatch gaps per 256^3 Flow-3D step.  Inside a `with prepared_weights():` block the
# slabs of weights that are autograd LEAVES (a model's parameters) are kept, keyed by (storage address, layer
# geometry), and the first convolution that meets a stale slab re-lays ALL registered weights of the device with ONE
# fs_conv3d_wprep_batch launch.  The block is a promise by its owner -- `Model.update` / `Model.inference` -- that the
# weights change only at its end (the optimiser step): leaving it makes every slab stale.  That explicit epoch is the
# rule; tensor version counters are checked as well, but they cannot be the rule: torch's fused AdamW updates
# parameters without bumping them.  Outside such a block (a bare IFNet, the convgrad modules in someone else's
# model) every convolution prepares its weights itself, as before.  FLOWSCI_WPREP_PER_LAUNCH=1 (ablation mode): never keep slabs.
import contextlib as _contextlib
import os as _os
import weakref as _weakref

_PREP_ON = _lib.ablation_env("FLOWSCI_WPREP_PER_LAUNCH") != "1"
_prep_epoch = 0
_prep_depth = 0
_prep_tables = {}


def invalidate_prepared_weights():
    """Every cached weight slab is stale from now on."""
    global _prep_epoch
    _prep_epoch += 1


@_contextlib.contextmanager
def prepared_weights():
    """Weights are constant inside this block except for an optimiser step at its very end."""
    global _prep_depth
    _prep_depth += 1
    try:
        yield
    finally:
        _prep_depth -= 1
        invalidate_prepared_weights()
        if _prep_depth == 0 and torch.cuda.is_available() and not torch.cuda.is_current_stream_capturing():
            for tab in _prep_tables.values():  # layers met for the first time in this block join the batch table,
                tab._evict()                   # slabs no block has used for a while leave it
                if tab.dirty:
                    tab.upload()


class _PrepEntry:
    __slots__ = ("wref", "ws", "jobs", "stamp", "used", "pinned")


_PREP_KEEP_EPOCHS = 8      # a slab not used for this many weight epochs (optimiser steps / inference calls) is dropped
_PREP_MAX_JOBS = 65535     # fs_conv3d_wprep_batch's grid limit


class _PrepTable:
    def __init__(self, device):
        self.device, self.entries, self.dirty, self.dev_jobs, self.njobs = device, {}, False, None, 0
        # what a HIP-graph capture has baked in as raw pointers -- job tables (the captured fs_conv3d_wprep_batch
        # launch reads `dev_jobs.data_ptr()`) and slabs (the captured convolutions read `ws`) -- must never go back
        # to the caching allocator while the graph may be replayed; a graph has no destructor hook here, so they are
        # kept for the life of the process (a table is 48 B per job, a slab 1-2 MB per layer and shape)
        self.captured = []

    def _live(self):
        live = []
        for k, e in list(self.entries.items()):
            w = e.wref()
            if w is None:  # the weight is gone (its address may be reused): forget the slab
                del self.entries[k]
                self.dirty = True
            elif e.jobs:
                live.append((e, w))
        return live

    def _evict(self):
        """Variable-size inference / evaluation meets a new geometry per call: slabs that no block has used for
        _PREP_KEEP_EPOCHS epochs leave the table (and the batch launch) unless a captured graph reads them."""
        for k, e in list(self.entries.items()):
            if not e.pinned and _prep_epoch - e.used > _PREP_KEEP_EPOCHS:
                del self.entries[k]
                self.dirty = True

    def upload(self):
        """(Re)build the device copy of the job table -- a pinned host buffer and an H2D copy: not capturable, so
        prepared_weights() does it when a block ends, never inside a HIP-graph capture.  The previous table is
        simply dropped unless a capture referenced it (`captured`)."""
        self._evict()
        live = self._live()
        jobs = [j for e, _ in live for j in e.jobs]
        if len(jobs) > _PREP_MAX_JOBS:  # more than one launch can take: every convolution prepares its own weights
            jobs = []
        if jobs:
            arr = (_lib.FsWprepJob * len(jobs))(*jobs)
            host = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).pin_memory()
            self.dev_jobs, self.njobs = host.to(self.device, non_blocking=True), len(jobs)
        else:
            self.dev_jobs, self.njobs = None, 0
        self.dirty = False

    def refresh(self):
        """Re-lay every registered weight with one launch.  False when that is not possible right now (the table
        changed and the stream is capturing): the caller prepares its own weights, as the classic path does."""
        if self.dirty or self.dev_jobs is None:
            if torch.cuda.is_current_stream_capturing():
                return False
            self.upload()
        live = self._live()
        if self.dirty:  # an entry died between the upload and now
            return False
        if not self.njobs:
            return False  # nothing registered, or too many jobs for one launch: per-launch preparation
        if torch.cuda.is_current_stream_capturing():
            self.captured.append(self.dev_jobs)       # the graph replays this launch with this table's address
            for e, _ in live:
                e.pinned = True
        with torch.cuda.device(self.device):
            _call("fs_conv3d_wprep_batch", self.dev_jobs.data_ptr(), self.njobs,
                  torch.cuda.current_stream(self.device).cuda_stream,
                  algo_bytes=8 * sum(j.total for e, _ in live for j in e.jobs))
        for e, w in live:
            e.stamp = (w._version, _prep_epoch)
        return True


def _prepared(w, nfloats, key, plan):
    """(pointer to pass as `w`, slab tensor to pass as `ws`).  plan(jobs, cap, ws) -> number of FsWprepJob records
    written (the library's own dispatch decides the layout).  0 as the pointer means "the slab is prepared"."""
    if not (_PREP_ON and _prep_depth > 0 and w.is_leaf and w.requires_grad):
        return w.data_ptr(), w.new_empty(max(int(nfloats), 1))
    tab = _prep_tables.get((w.device.type, w.device.index))
    if tab is None:
        tab = _prep_tables[(w.device.type, w.device.index)] = _PrepTable(w.device)
    global _last_prep
    k = (w.data_ptr(), tuple(w.shape)) + key
    e = tab.entries.get(k)
    capturing = torch.cuda.is_current_stream_capturing()
    if e is not None and e.wref() is not None:
        e.used = _prep_epoch
        if capturing and not e.pinned:  # a captured convolution reads this slab by address from now on
            e.pinned = True
            tab.captured.append(e.ws)
    _last_prep = None  # (only a first-use stamp can describe a slab nobody has written: _prep_not_written)
    if e is None or e.wref() is None:
        e = _last_prep = _PrepEntry()
        e.wref, e.stamp, e.used, e.pinned = _weakref.ref(w), None, _prep_epoch, capturing
        e.ws = torch.empty(max(int(nfloats), 1), device=w.device, dtype=torch.float32)
        buf = (_lib.FsWprepJob * 4)()
        n = int(plan(buf, 4, e.ws))
        if n < 0 or n > 4:
            raise _lib.FlowsciKernelError("weight re-layout plan failed (%d)" % n)
        e.jobs = [_lib.FsWprepJob.from_buffer_copy(buf[i]) for i in range(n)]
        tab.entries[k] = e
        tab.dirty = True
        if capturing:
            tab.captured.append(e.ws)
        # first use: the convolution re-lays the weights into the (now persistent) slab itself, as the classic path does;
        # from the next stale epoch on the slab is part of the device's one batch launch
        e.stamp = (w._version, _prep_epoch)
        return w.data_ptr(), e.ws
    if not e.jobs:  # this shape's kernel reads the weights as stored
        return w.data_ptr(), e.ws
    if e.stamp != (w._version, _prep_epoch) and not tab.refresh():
        e.stamp = (w._version, _prep_epoch)
        return w.data_ptr(), e.ws
    return 0, e.ws


_last_prep = None


def _prep_not_written():
    """The entry point that was handed a FIRST-USE slab (stamped current on the promise that the call itself lays the
    weights out) answered FS_ERR_UNSUPPORTED: it may have returned before its re-layout ran (csrc/convfwd.hip rejects
    > 12 source planes first), so the stamp does not describe the slab -- the fallback call with the same key must not
    pass w = NULL.  Slabs written by an earlier call or by the batch launch are not touched."""
    if _last_prep is not None:
        _last_prep.stamp = None


def _prepared_fwd(w, xptr, geo):
    """Slab of fs_conv3d_fwd* for a call of geometry `geo` (B, Cin, Cout, Di, Hi, Wi, Do, Ho, Wo, k, stride, pad,
    wmode): which layout (direct taps, or the Winograd-transformed filter of the 64-channel k3 trunk layers) is the
    library's decision for the call's geometry."""
    L = _lib.lib()
    return _prepared(w, L.fs_conv3d_fwd_ws_floats(geo[1], geo[2], geo[9]), ("fwd", xptr % 16) + geo,
                     lambda jobs, cap, ws: L.fs_conv3d_fwd_wprep_jobs(jobs, cap, xptr, w.data_ptr(), ws.data_ptr(), *geo))


def conv3d_wrw_supported(k, stride, padding):
    return (len(k) == 3 and k[0] == k[1] == k[2] and stride[0] == stride[1] == stride[2] and
            padding[0] == padding[1] == padding[2] and (k[0], stride[0]) in ((3, 1), (4, 2)) and
            0 <= padding[0] < k[0])


def _vol(dhw):
    return int(dhw[0]) * int(dhw[1]) * int(dhw[2])


# The convolution kernels address one staged channel chunk with 32-bit byte offsets; these predicates
# mirror the FS_ERR_SHAPE limits of csrc/conv{fwd,tr,wrw}.hip so that callers can route an oversize layer
# (e.g. the first / last layers of a 512^3 volume) to the torch.nn base class instead of raising.
def conv3d_fwd_fits(in_dhw, out_dhw, k):
    return (4 if k == 3 else 2) * _vol(in_dhw) * 4 < (1 << 32) and _vol(out_dhw) < (1 << 31)


def conv3d_tr_fits(in_dhw):
    return 4 * _vol(in_dhw) * 4 < (1 << 32) and 8 * _vol(in_dhw) < (1 << 31)


def conv3d_wrw_fits(src_dhw, g_dhw):
    return 8 * _vol(src_dhw) * 4 < (1 << 32) and 64 * _vol(g_dhw) * 4 < (1 << 32)


# The weight-gradient kernels finish with float atomics into a zero-filled dW: ~56 fill launches of a few KB .. 1.7 MB per
# Flow-3D step (4 us each plus their dispatch gaps).  Inside a prepared_weights() block -- one optimiser step -- the dW
# tensors are slices of ONE arena zeroed by a single memset; the arena is sized from what the previous step asked for and
# lives as long as any gradient that points into it (a new one per step: nothing is ever re-zeroed in place).
_dw_arena = {}   # device -> [epoch, tensor, offset (floats), floats asked for so far in this epoch]
_dw_need = {}    # device -> floats the last complete epoch asked for


def _dw_zeros(like, shape):
    n = 1
    for v in shape:
        n *= int(v)
    if _prep_depth == 0 or not _PREP_ON or torch.cuda.is_current_stream_capturing():
        return like.new_zeros(shape)
    dev = like.device
    st = _dw_arena.get(dev)
    if st is None or st[0] != _prep_epoch:
        if st is not None:
            _dw_need[dev] = st[3]
        need = _dw_need.get(dev, 0)
        st = _dw_arena[dev] = [_prep_epoch, like.new_zeros(need) if need else None, 0, 0]
    pad = (n + 3) // 4 * 4  # slices stay 16-byte aligned
    st[3] += pad
    if st[1] is None or st[2] + pad > st[1].numel():
        return like.new_zeros(shape)  # first step, or a step that asks for more than the last one did
    out = st[1].narrow(0, st[2], n).view(shape)
    st[2] += pad
    return out


def _conv3d_wrw_det(g, src_ptr, pv, sv, geo, nbytes, acct, allow_unsupported=False):
    """fs_conv3d_wrw_det: the same kernels with every run of positions storing its partial tile into its own copy of dW
    (a workspace of runs x |dW| floats) and one more launch adding the copies in run order -- no float atomics, bitwise
    reproducible.  Taken when torch.are_deterministic_algorithms_enabled().  `acct`: the call's _kernel_accounting."""
    L = _lib.lib()
    need = int(L.fs_conv3d_wrw_det_ws_floats(g.data_ptr(), src_ptr, pv, sv, *geo))
    if need == -FS_ERR_UNSUPPORTED and allow_unsupported:
        return None
    if need < 0:
        _lib.check(-need, "fs_conv3d_wrw_det_ws_floats")
    B, Cg, Cs = geo[:3]
    k = geo[9]
    dw = g.new_empty(Cg, Cs, k, k, k)
    ws = g.new_empty(max(need, 1))
    sym, fl, fq = acct
    with torch.cuda.device(g.device):
        _call("fs_conv3d_wrw_det", g.data_ptr(), src_ptr, pv, sv, dw.data_ptr(), ws.data_ptr(), need, *geo, _stream(g),
              algo_bytes=nbytes, algo_flops=fl, equiv_flops=fq, record_as="fs_conv3d_wrw", kernel=sym)
    return dw


def conv3d_wrw(g, src, k, stride, pad):
    """dW[Cg, Cs, k,k,k] = sum_{b,o} g[b,:,o] (x) src[b,:,o*stride + koff - pad]  (fs_conv3d_wrw)."""
    g = _need_cuda_f32("g", g, 5)
    src = _need_cuda_f32("src", src, 5)
    B, Cg = g.shape[:2]
    Cs = src.shape[1]
    if src.shape[0] != B:
        raise ValueError("batch mismatch")
    geo = (B, Cg, Cs, g.shape[2], g.shape[3], g.shape[4], src.shape[2], src.shape[3], src.shape[4], int(k), int(stride), int(pad))
    acct = _kernel_accounting("wrw", (g.data_ptr() % 16, src.data_ptr() % 16), *geo)
    if torch.are_deterministic_algorithms_enabled():
        return _conv3d_wrw_det(g, src.data_ptr(), None, None, geo, 4 * (g.numel() + src.numel()), acct)
    dw = _dw_zeros(g, (Cg, Cs, k, k, k))
    sym, fl, fq = acct
    with torch.cuda.device(g.device):
        _call("fs_conv3d_wrw", g.data_ptr(), src.data_ptr(), dw.data_ptr(), *geo, _stream(g),
              algo_bytes=4 * (g.numel() + src.numel()), algo_flops=fl, equiv_flops=fq, kernel=sym)
    return dw


WRW_KERNEL_BRICK, WRW_KERNEL_DMA, WRW_KERNEL_WINO23, WRW_KERNEL_WINO43, WRW_KERNEL_S3 = 0, 1, 2, 3, 4  # include/flowsci_hip.h FS_WRW_KERNEL_*


def conv3d_wrw_kernel_id(g_ptr, src_ptr, B, Cg, Cs, g_dhw, src_dhw, k, stride, pad):
    """The kernel fs_conv3d_wrw dispatches this call to (WRW_KERNEL_*): the library's own answer
    (fs_conv3d_wrw_kernel_id; nothing is launched, the pointers are inspected for alignment only)."""
    kid = _plan("wrw", (int(g_ptr) % 16, int(src_ptr) % 16),
                tuple(int(v) for v in (B, Cg, Cs, *g_dhw, *src_dhw, k, stride, pad)))[0]
    if kid < 0:
        _lib.check(-kid, "fs_conv3d_wrw_kernel_id")
    return kid


def conv3d_wrw_takes_winograd(B, Cg, Cs, g_dhw, src_dhw, k, stride, pad, g_misalign=0, src_misalign=0):
    """Does fs_conv3d_wrw run this call in a Winograd domain (F(4,3), csrc/convwrwwino4.hpp: half the direct form's
    multiply-adds)?  Asked of the library's dispatch: the 64 -> 64 k3 s1 p1 layers with rows of 64 x, an even number
    of y rows, >= 1024 position bricks, 16-byte aligned operands."""
    return conv3d_wrw_kernel_id(0x1000 + g_misalign, 0x1000 + src_misalign, B, Cg, Cs, g_dhw, src_dhw, k, stride,
                                pad) in (WRW_KERNEL_WINO23, WRW_KERNEL_WINO43)


FS_ERR_UNSUPPORTED = 5


def _channel_planes(pieces):
    """(pointer array, batch-stride array, Cin) for fs_*_ms -- two ctypes HOST arrays of Cin entries, read by the entry
    point at launch (the caller keeps `pieces` alive across the launch) -- every channel of every piece as the
    plane it already is.  A piece is a [B, Ci, D,H,W] tensor, contiguous or a channel slice of a wider contiguous
    one; None when a piece has other strides / alignment (the caller concatenates instead)."""
    B, dhw = pieces[0].shape[0], tuple(pieces[0].shape[2:])
    vol = dhw[0] * dhw[1] * dhw[2]
    inner = (vol, dhw[1] * dhw[2], dhw[2], 1)
    ptrs, strides = [], []
    for t in pieces:
        if (not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32 or t.dim() != 5 or
                t.shape[0] != B or tuple(t.shape[2:]) != dhw or tuple(t.stride()[1:]) != inner or
                t.stride(0) < t.shape[1] * vol or t.stride(0) % 4 or t.data_ptr() % 16 or vol % 4):
            return None
        for c in range(t.shape[1]):
            ptrs.append(t.data_ptr() + 4 * c * vol)
            strides.append(t.stride(0))
    n = len(ptrs)
    if n > 12:
        return None
    return (ctypes.c_void_p * n)(*ptrs), (ctypes.c_longlong * n)(*strides), n


def conv3d_fwd_prelu_ms(pieces, w, bias, prelu_weight, k, stride, pad):
    """(y, prelu(y)) of conv3d(torch.cat(pieces, 1), w, bias, stride, pad) without the concatenation
    (fs_conv3d_fwd_prelu_ms: the loader waves read every channel where it lies), or None when no such kernel
    covers the shape -- the caller then concatenates."""
    planes = _channel_planes(pieces)
    if planes is None:
        return None
    pv, sv, Cin = planes
    w = _need_cuda_f32("w", w, 5)
    a = _need_cuda_f32("prelu_weight", prelu_weight, 1)
    Cout = w.shape[0]
    if w.shape[1] != Cin or tuple(w.shape[2:]) != (k, k, k):
        raise ValueError("weight %s does not fit %d input channels" % (tuple(w.shape), Cin))
    if bias is not None:
        bias = _need_cuda_f32("bias", bias, 1)
    x0 = pieces[0]
    B = x0.shape[0]
    Di, Hi, Wi = x0.shape[2:]
    Do, Ho, Wo = [(n + 2 * pad - k) // stride + 1 for n in (Di, Hi, Wi)]
    if min(Do, Ho, Wo) < 1:
        return None
    y = x0.new_empty((B, Cout, Do, Ho, Wo))
    z = torch.empty_like(y)
    geo = (B, Cin, Cout, Di, Hi, Wi, Do, Ho, Wo, int(k), int(stride), int(pad), 0)
    wp, ws = _prepared_fwd(w, x0.data_ptr(), geo)
    # (the multi-source dispatch is the single-tensor one's for the same shape; the first plane stands for the alignment)
    sym, fl, fq = _kernel_accounting("fwd", (x0.data_ptr() % 16,), *geo)
    xbytes = 4 * B * Cin * Di * Hi * Wi
    with torch.cuda.device(x0.device):
        rc = _call("fs_conv3d_fwd_prelu_ms", pv, sv, wp, _ptr(bias), a.data_ptr(), y.data_ptr(), z.data_ptr(),
                   ws.data_ptr(), B, Cin, Cout, Di, Hi, Wi, Do, Ho, Wo, int(k), int(stride), int(pad), int(a.numel()),
                   _stream(x0), algo_bytes=xbytes + 8 * y.numel(), algo_flops=fl, equiv_flops=fq, kernel=sym,
                   record_as="fs_conv3d_fwd", allow=(FS_ERR_UNSUPPORTED,))
    if rc == FS_ERR_UNSUPPORTED:
        _prep_not_written()
        return None
    return y, z


def conv3d_wrw_ms(g, pieces, k, stride, pad):
    """conv3d_wrw(g, torch.cat(pieces, 1), ...) without the concatenation (fs_conv3d_wrw_ms), or None."""
    planes = _channel_planes(pieces)
    if planes is None:
        return None
    pv, sv, Cs = planes
    g = _need_cuda_f32("g", g, 5)
    B, Cg = g.shape[:2]
    Di, Hi, Wi = pieces[0].shape[2:]
    geo = (B, Cg, Cs, g.shape[2], g.shape[3], g.shape[4], Di, Hi, Wi, int(k), int(stride), int(pad))
    # (the multi-source dispatch is the single-tensor one's for the same shape; the first plane stands for the alignment)
    acct = _kernel_accounting("wrw", (g.data_ptr() % 16, pieces[0].data_ptr() % 16), *geo)
    if torch.are_deterministic_algorithms_enabled():
        return _conv3d_wrw_det(g, 0, pv, sv, geo, 4 * (g.numel() + B * Cs * Di * Hi * Wi), acct, allow_unsupported=True)
    dw = _dw_zeros(g, (Cg, Cs, k, k, k))
    sym, fl, fq = acct
    with torch.cuda.device(g.device):
        rc = _call("fs_conv3d_wrw_ms", g.data_ptr(), pv, sv, dw.data_ptr(), *geo, _stream(g),
                   algo_bytes=4 * (g.numel() + B * Cs * Di * Hi * Wi), algo_flops=fl, equiv_flops=fq, kernel=sym,
                   record_as="fs_conv3d_wrw", allow=(FS_ERR_UNSUPPORTED,))
    if rc == FS_ERR_UNSUPPORTED:
        return None
    return dw


def conv3d_deconv_grad_input_dprelu(gy, w, act_y, prelu_weight):
    """Input gradient of ConvTranspose3d(4, 2, 1) with weight w [Cin, Cout, 4,4,4] whose INPUT was z = prelu(act_y):
    (grad_act_y, grad_prelu_weight, grad_bias_of_the_layer_that_produced_act_y) in one launch
    (fs_conv3d_fwd_dprelu: the PReLU backward is the convolution's epilogue), or None when that fused kernel does not
    cover the shape -- the caller then runs conv3d_fwd + prelu_backward."""
    gy = _need_cuda_f32("grad_output", gy, 5)
    w = _need_cuda_f32("w", w, 5)
    act_y = _aligned16(_need_cuda_f32("act_y", act_y, 5))
    a = _need_cuda_f32("prelu_weight", prelu_weight, 1)
    B, Cg = gy.shape[:2]                      # the strided convolution's input = grad_out: Cg = deconv Cout
    Cin_t = w.shape[0]                        # its output channels = the deconvolution's input channels
    if w.shape[1] != Cg or tuple(w.shape[2:]) != (4, 4, 4) or act_y.shape[1] != Cin_t or a.numel() not in (1, Cin_t):
        raise ValueError("shapes do not describe a k4 s2 deconvolution: gy %s w %s act_y %s" %
                         (tuple(gy.shape), tuple(w.shape), tuple(act_y.shape)))
    Di, Hi, Wi = gy.shape[2:]
    Do, Ho, Wo = act_y.shape[2:]
    if any((n + 2 - 4) // 2 + 1 != m for n, m in zip((Di, Hi, Wi), (Do, Ho, Wo))) or Cin_t > 32:
        return None
    L = _lib.lib()
    npart = int(L.fs_conv3d_fwd_dprelu_part_floats(B, Cin_t, Do, Ho, Wo))
    if npart < 0:
        return None
    out = torch.empty_like(act_y)
    ga, gb = torch.empty_like(a), act_y.new_empty(Cin_t)
    part = act_y.new_empty(npart)
    geo = (B, Cg, Cin_t, Di, Hi, Wi, Do, Ho, Wo, 4, 2, 1, 0)
    wp, ws = _prepared_fwd(w, gy.data_ptr(), geo)
    sym, fl, fq = _kernel_accounting("fwd", (gy.data_ptr() % 16,), *geo)
    with torch.cuda.device(gy.device):
        rc = _call("fs_conv3d_fwd_dprelu", gy.data_ptr(), wp, act_y.data_ptr(), a.data_ptr(), a.numel(), out.data_ptr(),
                   ga.data_ptr(), gb.data_ptr(), part.data_ptr(), ws.data_ptr(), B, Cg, Cin_t, Di, Hi, Wi, Do, Ho, Wo,
                   4, 2, 1, _stream(gy), algo_bytes=4 * (gy.numel() + 2 * out.numel()), algo_flops=fl, equiv_flops=fq,
                   kernel=sym, record_as="fs_conv3d_fwd", allow=(FS_ERR_UNSUPPORTED,))
    if rc == FS_ERR_UNSUPPORTED:
        _prep_not_written()
        return None
    return out, ga, gb


def conv3d_k3_grad_input_dprelu(gy, w, act_y, prelu_weight):
    """Input gradient of a stride-1 'same' Conv3d (weight w [Cout, Cin, 3,3,3]) whose INPUT was z = prelu(act_y) -- the
    inner PReLU of an IFBlock residual unit: (grad_act_y, grad_prelu_weight, grad_bias of the layer that produced act_y)
    in one launch (fs_conv3d_fwd_dprelu, kernel 3: the PReLU backward is the convolution's epilogue), or None when the
    fused kernel does not cover the shape (the caller then runs conv3d_fwd wmode 1 + prelu_backward)."""
    gy = _need_cuda_f32("grad_output", gy, 5)
    w = _need_cuda_f32("w", w, 5)
    act_y = _aligned16(_need_cuda_f32("act_y", act_y, 5))
    a = _need_cuda_f32("prelu_weight", prelu_weight, 1)
    B, Cg = gy.shape[:2]
    Cx = w.shape[1]                           # the gradient's channels = the convolution's input channels
    if w.shape[0] != Cg or tuple(w.shape[2:]) != (3, 3, 3) or tuple(act_y.shape) != (B, Cx) + tuple(gy.shape[2:]):
        raise ValueError("shapes do not belong to one convolution: %s %s %s" % (tuple(gy.shape), tuple(w.shape), tuple(act_y.shape)))
    if a.numel() not in (1, Cx):
        raise ValueError("prelu_weight must have 1 or %d elements" % Cx)
    D, H, W = gy.shape[2:]
    L = _lib.lib()
    npart = int(L.fs_conv3d_fwd_dprelu_part_floats_k3(B, Cx, D, H, W))
    if npart < 0:
        return None
    out = torch.empty_like(act_y)
    ga, gb = torch.empty_like(a), act_y.new_empty(Cx)
    part = act_y.new_empty(npart)
    geo = (B, Cg, Cx, D, H, W, D, H, W, 3, 1, 1, 1)
    wp, ws = _prepared_fwd(w, gy.data_ptr(), geo)
    sym, fl, fq = _kernel_accounting("fwd", (gy.data_ptr() % 16,), *geo)
    with torch.cuda.device(gy.device):
        rc = _call("fs_conv3d_fwd_dprelu", gy.data_ptr(), wp, act_y.data_ptr(), a.data_ptr(), a.numel(),
                   out.data_ptr(), ga.data_ptr(), gb.data_ptr(), part.data_ptr(), ws.data_ptr(), B, Cg, Cx, D, H, W,
                   D, H, W, 3, 1, 1, _stream(gy), algo_bytes=4 * (gy.numel() + 2 * out.numel()), algo_flops=fl,
                   equiv_flops=fq, kernel=sym, record_as="fs_conv3d_fwd", allow=(FS_ERR_UNSUPPORTED,))
    if rc == FS_ERR_UNSUPPORTED:
        _prep_not_written()
        return None
    return out, ga, gb


def conv3d_fwd_workgroups(B, Cout, out_dhw, k):
    """Workgroups fs_conv3d_fwd launches for this layer (mirrors its brick choice, csrc/convfwd.hip)."""
    Do, Ho, Wo = out_dhw
    cd = lambda a, b: -(-a // b)
    tw = 32 if Wo > 16 else 16
    r = 32 // tw
    if k == 3:
        mg = cd(Cout, 64)
        big = B * cd(Do, 2) * cd(Ho, 8 * r) * cd(Wo, tw) * mg
        if big >= 512:
            return big
        small = B * Do * cd(Ho, 4 * r) * cd(Wo, tw) * mg
        return small if small >= 256 else 2 * small  # 32-channel workgroups when 64-channel ones cannot fill the chip
    if Cout <= 32:
        return B * Do * cd(Ho, 8 * r) * cd(Wo, tw)
    mg = cd(Cout, 64)
    big = B * cd(Do, 2) * cd(Ho, 8 * r) * cd(Wo, tw) * mg
    if big >= 256:
        return big
    small = B * Do * cd(Ho, 4 * r) * cd(Wo, tw) * mg  # quarter-size bricks, then 32-channel workgroups
    return small if small >= 256 else 2 * small


def conv3d_fwd(x, w, bias, k, stride, pad, wmode=0, prelu_weight=None, addend=None):
    """fs_conv3d_fwd: y = conv3d(x, W, bias, stride, pad) with W = w (wmode 0, [Cout,Cin,k,k,k]) or the
    flipped transpose of w (wmode 1, w [Cin,Cout,k,k,k]: input gradient of a stride-1 same conv).
    With `prelu_weight` (wmode 0): returns (y, prelu(y) [+ addend]), both written by the convolution's
    epilogue.  `addend` without `prelu_weight`: y = conv + bias + addend."""
    x = _need_cuda_f32("x", x, 5)
    w = _need_cuda_f32("w", w, 5)
    B, Cin = x.shape[:2]
    Cout = w.shape[1] if wmode else w.shape[0]
    if (w.shape[0] if wmode else w.shape[1]) != Cin or tuple(w.shape[2:]) != (k, k, k):
        raise ValueError("weight %s does not fit input %s (wmode %d)" % (tuple(w.shape), tuple(x.shape), wmode))
    if bias is not None:
        bias = _need_cuda_f32("bias", bias, 1)
        if bias.numel() != Cout:
            raise ValueError("bias must have %d elements" % Cout)
    Di, Hi, Wi = x.shape[2:]
    Do, Ho, Wo = [(n + 2 * pad - k) // stride + 1 for n in (Di, Hi, Wi)]
    if min(Do, Ho, Wo) < 1:
        raise ValueError("convolution output is empty for input %s" % (tuple(x.shape),))
    y = x.new_empty((B, Cout, Do, Ho, Wo))
    geo = (B, Cin, Cout, Di, Hi, Wi, Do, Ho, Wo, int(k), int(stride), int(pad), int(wmode))
    wp, ws = _prepared_fwd(w, x.data_ptr(), geo)
    sym, fl, fq = _kernel_accounting("fwd", (x.data_ptr() % 16,), *geo)
    acct = dict(algo_flops=fl, equiv_flops=fq, kernel=sym, record_as="fs_conv3d_fwd")
    nb = 4 * (x.numel() + y.numel())
    if addend is not None:
        addend = _aligned16(_need_cuda_f32("addend", addend, 5))
        if addend.shape != y.shape:
            raise ValueError("addend %s must have the output shape %s" % (tuple(addend.shape), tuple(y.shape)))
        nb += 4 * y.numel()
    with torch.cuda.device(x.device):
        if prelu_weight is None and addend is not None:
            _call("fs_conv3d_fwd_add", x.data_ptr(), wp, _ptr(bias), addend.data_ptr(), y.data_ptr(),
                  ws.data_ptr(), *geo, _stream(x), algo_bytes=nb, **acct)
            return y
        if prelu_weight is None:
            _call("fs_conv3d_fwd", x.data_ptr(), wp, _ptr(bias), y.data_ptr(), ws.data_ptr(), *geo, _stream(x),
                  algo_bytes=nb, **acct)
            return y
        if wmode:
            raise ValueError("the fused PReLU epilogue is forward-only (wmode 0)")
        a = _need_cuda_f32("prelu_weight", prelu_weight, 1)
        if a.numel() not in (1, Cout):
            raise ValueError("prelu_weight must have 1 or %d elements" % Cout)
        z = torch.empty_like(y)
        _call("fs_conv3d_fwd_prelu", x.data_ptr(), wp, _ptr(bias), a.data_ptr(), _ptr(addend),
              y.data_ptr(), z.data_ptr(), ws.data_ptr(), B, Cin, Cout, Di, Hi, Wi, Do, Ho, Wo, int(k), int(stride),
              int(pad), a.numel(), _stream(x), algo_bytes=nb + 4 * y.numel(), **acct)
    return y, z


def conv3d_tr_supported(cout, k, stride, padding):
    return (tuple(k) == (4, 4, 4) and tuple(stride) == (2, 2, 2) and tuple(padding) == (1, 1, 1) and
            (cout <= 32 or (cout % 32 == 0 and cout <= 128)))


def conv3d_tr(x, w, bias, out_dhw=None, prelu_weight=None, addend=None):
    """fs_conv3d_tr: ConvTranspose3d(4, 2, 1)(x) with weight w [Cin,Cout,4,4,4]; with out_dhw = the
    input extent of a Conv3d(4, 2, 1) layer and w = that layer's weight, its input gradient.
    With `prelu_weight`: returns (y, prelu(y)), both written by the epilogue.  With `addend` (y's shape):
    y = conv_transpose(x) + bias + addend."""
    x = _need_cuda_f32("x", x, 5)
    w = _need_cuda_f32("w", w, 5)
    B, Cin = x.shape[:2]
    Cout = w.shape[1]
    if w.shape[0] != Cin or tuple(w.shape[2:]) != (4, 4, 4):
        raise ValueError("weight %s does not fit input %s" % (tuple(w.shape), tuple(x.shape)))
    if bias is not None:
        bias = _need_cuda_f32("bias", bias, 1)
        if bias.numel() != Cout:
            raise ValueError("bias must have %d elements" % Cout)
    Di, Hi, Wi = x.shape[2:]
    Do, Ho, Wo = (2 * Di, 2 * Hi, 2 * Wi) if out_dhw is None else tuple(int(v) for v in out_dhw)
    y = x.new_empty((B, Cout, Do, Ho, Wo))
    nws = int(_lib.lib().fs_conv3d_tr_ws_floats(Cin, Cout))
    if nws < 0:
        raise ValueError("fs_conv3d_tr supports up to 32 output channels or 64 / 96 / 128, got %d" % Cout)
    L = _lib.lib()
    has_z = int(prelu_weight is not None)
    geo = (B, Cin, Cout, Di, Hi, Wi, Do, Ho, Wo, has_z)
    wp, ws = _prepared(w, nws, ("tr",) + geo + (x.data_ptr() % 16,),
                       lambda jobs, cap, slab: L.fs_conv3d_tr_wprep_jobs(jobs, cap, x.data_ptr(), w.data_ptr(),
                                                                        slab.data_ptr(), *geo))
    sym, fl, fq = _kernel_accounting("tr", (x.data_ptr() % 16,), *geo)
    acct = dict(algo_flops=fl, equiv_flops=fq, kernel=sym, record_as="fs_conv3d_tr")
    nb = 4 * (x.numel() + y.numel())
    with torch.cuda.device(x.device):
        if addend is not None:
            if prelu_weight is not None:
                raise ValueError("addend and prelu_weight are mutually exclusive")
            addend = _aligned16(_need_cuda_f32("addend", addend, 5))
            if addend.shape != y.shape:
                raise ValueError("addend %s must have the output shape %s" % (tuple(addend.shape), tuple(y.shape)))
            _call("fs_conv3d_tr_add", x.data_ptr(), wp, _ptr(bias), addend.data_ptr(), y.data_ptr(),
                  ws.data_ptr(), B, Cin, Cout, Di, Hi, Wi, Do, Ho, Wo, _stream(x), algo_bytes=nb + 4 * y.numel(),
                  **acct)
            return y
        if prelu_weight is None:
            _call("fs_conv3d_tr", x.data_ptr(), wp, _ptr(bias), y.data_ptr(), ws.data_ptr(), B, Cin,
                  Cout, Di, Hi, Wi, Do, Ho, Wo, _stream(x), algo_bytes=nb, **acct)
            return y
        a = _need_cuda_f32("prelu_weight", prelu_weight, 1)
        if a.numel() not in (1, Cout):
            raise ValueError("prelu_weight must have 1 or %d elements" % Cout)
        z = torch.empty_like(y)
        _call("fs_conv3d_tr_prelu", x.data_ptr(), wp, _ptr(bias), a.data_ptr(), y.data_ptr(),
              z.data_ptr(), ws.data_ptr(), B, Cin, Cout, Di, Hi, Wi, Do, Ho, Wo, a.numel(), _stream(x),
              algo_bytes=nb + 4 * y.numel(), **acct)
    return y, z


# --------------------------------------------------------------------------------------------
# a9 'SSIM' branch: weighted SSIM + masked reduction, fused (upflow.py:141-196, 285-289)
# --------------------------------------------------------------------------------------------
class _WSSIMLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, y, weight, use_occ):
        x = _need_cuda_f32("x", x, 4)
        y = _need_cuda_f32("y", y, 4)
        weight = _need_cuda_f32("occ_mask", weight, 4)
        B, C, H, W = x.shape
        if y.shape != x.shape or tuple(weight.shape) != (B, 1, H, W):
            raise ValueError("weighted SSIM operands mismatch: %s %s %s" %
                             (tuple(x.shape), tuple(y.shape), tuple(weight.shape)))
        sums = x.new_empty(2)
        ws = x.new_empty(2 * _REDUCE_BLOCKS)
        with torch.cuda.device(x.device):
            _call("fs_wssim_fwd", x.data_ptr(), y.data_ptr(), weight.data_ptr(), sums.data_ptr(),
                  ws.data_ptr(), B, C, H, W, int(bool(use_occ)), _stream(x),
                  algo_bytes=4 * (2 * x.numel() + weight.numel()))
        if use_occ:
            dS1 = 1.0 / (sums[1] + 1e-6)
        else:
            dS1 = torch.full_like(sums[0], 1.0 / float(B * C * (H - 2) * (W - 2)))
        ctx.save_for_backward(x, y, weight, dS1)
        ctx.use_occ = int(bool(use_occ))
        return sums[0] * dS1

    @staticmethod
    def backward(ctx, gout):
        x, y, weight, dS1 = ctx.saved_tensors
        nx, ny = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (nx or ny):
            return None, None, None, None
        B, C, H, W = x.shape
        coef = (gout * dS1).reshape(1).contiguous()
        gx = torch.empty_like(x) if nx else None
        gy = torch.empty_like(y) if ny else None
        with torch.cuda.device(x.device):
            _call("fs_wssim_bwd", x.data_ptr(), y.data_ptr(), weight.data_ptr(), coef.data_ptr(), _ptr(gx),
                  _ptr(gy), B, C, H, W, ctx.use_occ, _stream(x))
        return gx, gy, None, None


def weighted_ssim_loss(x, y, occ_mask, photo_loss_use_occ):
    """photo_loss_multi_type(..., photo_loss_type='SSIM') in one fused pass."""
    return _WSSIMLoss.apply(x, y, occ_mask, bool(photo_loss_use_occ))


# --------------------------------------------------------------------------------------------
# Sequence evaluation: error.py:27-56 calculate_psnr / ssim per frame (fs_frame_metrics{2,3}d)
# --------------------------------------------------------------------------------------------
def frame_metrics_cost(shape, window="2d"):
    """(HBM bytes, flops) the algorithm needs for one frame_metrics call on [N,C,*spatial] inputs: both inputs
    read once; per element of the SSIM region 3 products, the five maps filtered with 11 taps along each axis (2 flops
    a tap) and ~15 flops of SSIM formula; per element 3 flops of squared error."""
    nd = 2 if window == "2d" else 3
    n = 1
    for s in shape:
        n *= int(s)
    lead = int(shape[0]) * int(shape[1])
    valid = lead
    for s in shape[2:]:
        valid *= int(s) - 10
    return 2 * 4 * n, 3 * n + valid * (3 + 5 * 11 * 2 * nd + 15)


def frame_metrics(pred, gt, data_range=1.0, window="2d"):
    """Per-frame PSNR and SSIM of `pred` against `gt` -- error.py:27-56 (calculate_psnr, ssim) for N frames in one
    launch.  window="2d": [N,C,H,W] (or [N,H,W]), the reference's 11x11 Gaussian SSIM, mean over the C channels' maps;
    window="3d": [N,C,D,H,W] (or [N,D,H,W]), the same window along three axes (no reference form exists: pinned by the
    project's fp64 restatement).  The window sums are fp64 inside the kernel (fp32 sums of E[x^2] - mu^2 lose ~1e-5 of
    SSIM on flat regions), the result within ~1e-7 of an fp64 evaluation.  Every filtered extent must be >= 11.  Inputs of another dtype are converted to fp32,
    non-contiguous ones copied once.  Returns (psnr [N], ssim [N]) as fp64 tensors on the inputs' device;
    psnr = 10 log10(L^2 / mse), +inf where mse == 0 (error.py:31-33), L = data_range."""
    if window not in ("2d", "3d"):
        raise ValueError("window must be '2d' or '3d', got %r" % (window,))
    nd = 2 if window == "2d" else 3
    for name, t in (("pred", pred), ("gt", gt)):
        if not isinstance(t, torch.Tensor):
            raise ValueError("%s must be a tensor" % name)
        if not t.is_cuda:
            raise ValueError("%s must live on a GPU (the HIP hot path has no CPU fallback); got %s" % (name, t.device))
        if t.dim() not in (nd + 1, nd + 2):
            raise ValueError("%s must be [N,C,%s] or [N,%s] for window=%r, got shape %s" %
                             (name, ",".join("DHW"[3 - nd:]), ",".join("DHW"[3 - nd:]), window, tuple(t.shape)))
    if pred.shape != gt.shape:
        raise ValueError("pred and gt differ in shape: %s vs %s" % (tuple(pred.shape), tuple(gt.shape)))
    if pred.device != gt.device:
        raise ValueError("pred and gt are on different devices")
    if not float(data_range) > 0:
        raise ValueError("data_range must be > 0, got %r" % (data_range,))
    if pred.dim() == nd + 1:
        pred, gt = pred.unsqueeze(1), gt.unsqueeze(1)
    if any(s < 11 for s in pred.shape[2:]):
        raise ValueError("every filtered extent must be >= 11 (11-tap valid window), got %s" % (tuple(pred.shape),))
    x = pred.to(torch.float32).contiguous()
    y = gt.to(torch.float32).contiguous()
    N, C = x.shape[:2]
    sp = tuple(x.shape[2:])
    if N == 0:
        e = torch.empty(0, dtype=torch.float64, device=x.device)
        return e, e.clone()
    lib = _lib.lib()
    nb = (lib.fs_frame_metrics2d_ws_bytes(N, C, *sp) if nd == 2 else lib.fs_frame_metrics3d_ws_bytes(N, C, *sp))
    if nb < 0:
        _lib.check(int(-nb), "fs_frame_metrics%dd_ws_bytes" % nd)
    ws = torch.empty((nb + 7) // 8, dtype=torch.float64, device=x.device)
    sums = torch.empty(2, N, dtype=torch.float64, device=x.device)
    nbytes, flops = frame_metrics_cost(x.shape, window)
    name = "fs_frame_metrics%dd" % nd
    with torch.cuda.device(x.device):
        _call(name, x.data_ptr(), y.data_ptr(), N, C, *sp, float(data_range), ws.data_ptr(), sums[0].data_ptr(),
              sums[1].data_ptr(), _stream(x), algo_bytes=nbytes, algo_flops=flops)
    L = float(data_range)
    per = C
    for s in sp:
        per *= s
    valid = C
    for s in sp:
        valid *= s - 10
    mse = sums[0] / per
    psnr = 10.0 * torch.log10((L * L) / mse)  # mse == 0 -> L^2/0 = inf -> +inf
    return psnr, sums[1] / valid


# --------------------------------------------------------------------------------------------
# Flow accuracy: EPE / RMSE / angular error / KITTI Fl against a ground-truth displacement (fs_flow_metrics{2,3}d)
# --------------------------------------------------------------------------------------------
FLOW_DISP, FLOW_RIFE3D = 0, 1
_FLOW_CONVENTIONS = {"disp": FLOW_DISP, "rife3d": FLOW_RIFE3D}
FLOW_METRICS_K = 13  # FS_FLOW_METRICS_K: the per-flow sums, in the order include/flowsci_hip.h documents


def flow_metrics_cost(shape, masks=2, write_map=False):
    """(HBM bytes, flops) the algorithm needs for one flow_metrics call on [N,C,*spatial] flows: both flows read once,
    `masks` uint8 masks read once, the fp32 EPE map written once if asked; ~60 flops per element (differences, norms,
    the cross product, the atan2 and the sums)."""
    n = 1
    for s in shape:
        n *= int(s)
    elems = n // int(shape[1])
    return 2 * 4 * n + masks * elems + (4 * elems if write_map else 0), 60 * elems


def rife3d_to_disp(flow):
    """Displacement (x along W, y along H, z along D) of a Flow-3D flow [N,3,D,H,W]: the model's warp samples the input
    at ix = (h+F0)(W-1)/(H-1), iy = (d+F1)(H-1)/(D-1), iz = (w+F2)(D-1)/(W-1) (Flow-3D/model/warplayer.py, the axis
    rotation), so x = ix - w, y = iy - h, z = iz - d -- not clamped.  A flow of zero is not "no motion".  Plain torch
    element-wise ops in the flow's dtype (not a hot path); every extent must be >= 2."""
    D, H, W = _rife3d_extent(flow)
    d, h, w = _dhw(flow)
    return torch.stack([(h + flow[:, 0]) * ((W - 1) / (H - 1)) - w,
                        (d + flow[:, 1]) * ((H - 1) / (D - 1)) - h,
                        (w + flow[:, 2]) * ((D - 1) / (W - 1)) - d], 1)


def disp_to_rife3d(disp):
    """Inverse of rife3d_to_disp: the Flow-3D flow [N,3,D,H,W] whose warp samples the input at (w + x, h + y, d + z),
    i.e. the flow that lets a ground-truth displacement drive the model's own warp (ops.warp3d)."""
    D, H, W = _rife3d_extent(disp)
    d, h, w = _dhw(disp)
    return torch.stack([(w + disp[:, 0]) * ((H - 1) / (W - 1)) - h,
                        (h + disp[:, 1]) * ((D - 1) / (H - 1)) - d,
                        (d + disp[:, 2]) * ((W - 1) / (D - 1)) - w], 1)


def _rife3d_extent(t):
    if not isinstance(t, torch.Tensor) or t.dim() != 5 or t.shape[1] != 3:
        raise ValueError("a 3-D flow must be [N,3,D,H,W], got %s" % (tuple(t.shape) if isinstance(t, torch.Tensor)
                                                                      else type(t).__name__,))
    D, H, W = (int(s) for s in t.shape[2:])
    if min(D, H, W) < 2:
        raise ValueError("the rife3d convention needs every extent >= 2, got %s" % (tuple(t.shape),))
    return D, H, W


def _dhw(t):
    D, H, W = t.shape[2:]
    kw = dict(dtype=t.dtype, device=t.device)
    return (torch.arange(D, **kw).view(1, D, 1, 1), torch.arange(H, **kw).view(1, 1, H, 1),
            torch.arange(W, **kw).view(1, 1, 1, W))


def _flow_operand(name, t, nd):
    """[N,C,*sp] fp32 on a GPU whose C planes per flow are contiguous [C,*sp] blocks: the batch stride may be anything
    (a channel slice flow[:, C:2C] passes as it is).  Anything else is converted / copied once."""
    if not isinstance(t, torch.Tensor):
        raise ValueError("%s must be a tensor" % name)
    if not t.is_cuda:
        raise ValueError("%s must live on a GPU (the HIP hot path has no CPU fallback); got %s" % (name, t.device))
    if t.dim() != nd + 2 or t.shape[1] != nd:
        raise ValueError("%s must be [N,%d,%s], got shape %s" % (name, nd, ",".join("DHW"[3 - nd:]), tuple(t.shape)))
    if t.dtype != torch.float32:
        t = t.to(torch.float32)
    inner = t[0] if t.shape[0] > 0 else t
    if t.shape[0] > 0 and not inner.is_contiguous():
        t = t.contiguous()
    if t.shape[0] > 1 and t.stride(0) < inner.numel():
        t = t.contiguous()
    return t


def _flow_mask(name, m, shape, device):
    if m is None:
        return None
    if not isinstance(m, torch.Tensor):
        raise ValueError("%s must be a tensor or None" % name)
    if m.device != device:
        raise ValueError("%s must be on the flows' device %s, got %s" % (name, device, m.device))
    if m.dim() == len(shape) + 1 and m.shape[1] == 1:
        m = m[:, 0]
    if tuple(m.shape) != tuple(shape):
        raise ValueError("%s must be [N,*spatial] = %s, got %s" % (name, tuple(shape), tuple(m.shape)))
    if m.dtype == torch.bool:
        m = m.contiguous().view(torch.uint8)
    elif m.dtype == torch.uint8:
        m = m.contiguous()
    else:
        m = (m != 0).contiguous().view(torch.uint8)
    return m


def flow_metrics(pred, gt, valid=None, noc=None, convention="disp", tau=(3.0, 0.05), return_map=False):
    """Accuracy of N predicted flows against N ground-truth displacements, one launch (fs_flow_metrics{2,3}d).

    pred, gt: [N,2,H,W] (channel 0 along W, 1 along H) or [N,3,D,H,W] (0 along W, 1 along H, 2 along D), in elements,
    on a GPU.  A channel slice such as IFNet's flow[:, C:2C] is read in place (only the per-flow [C,*sp] block has to
    be contiguous).  valid / noc: optional bool or uint8 [N,*sp] masks; valid None = all valid, noc None = no
    occlusion split (the noc / occ entries are NaN); noc counts only where valid is set.
    convention: "disp" (pred is a displacement: 2-D RIFE and PWC / UPFlow flows) or "rife3d" (a Flow-3D flow, whose
    warp rotates axes: converted to a displacement inside the kernel, as rife3d_to_disp does; every extent >= 2).
    gt is always a displacement.  tau = (tau_abs, tau_rel): an element is an outlier (KITTI Fl) when
    epe > tau_abs and epe > tau_rel |gt|.

    Returns a dict of fp64 [N] tensors: epe, epe_noc, epe_occ (mean end-point error over valid / noc / valid minus noc),
    rmse, ae_deg (Barron's angular error between (p, 1) and (g, 1), degrees), fl, fl_noc, fl_occ (outlier fractions),
    max_epe, n_valid, n_noc, n_nonfinite; with return_map=True also epe_map, fp32 [N,*sp] (epe at every element,
    NaN where pred or gt is not finite).  An element whose pred or gt is not finite counts as an outlier and in
    n_nonfinite, and is left out of the means and the max.  An empty subset gives NaN."""
    if convention not in _FLOW_CONVENTIONS:
        raise ValueError("convention must be 'disp' or 'rife3d', got %r" % (convention,))
    if not isinstance(pred, torch.Tensor) or pred.dim() not in (4, 5):
        raise ValueError("pred must be [N,2,H,W] or [N,3,D,H,W], got %s" %
                         (tuple(pred.shape) if isinstance(pred, torch.Tensor) else type(pred).__name__,))
    nd = pred.dim() - 2
    pred = _flow_operand("pred", pred, nd)
    gt = _flow_operand("gt", gt, nd)
    if pred.shape != gt.shape:
        raise ValueError("pred and gt differ in shape: %s vs %s" % (tuple(pred.shape), tuple(gt.shape)))
    if pred.device != gt.device:
        raise ValueError("pred and gt are on different devices")
    conv = _FLOW_CONVENTIONS[convention]
    if conv == FLOW_RIFE3D and nd != 3:
        raise ValueError("convention 'rife3d' is for [N,3,D,H,W] Flow-3D flows")
    sp = tuple(int(s) for s in pred.shape[2:])
    if conv == FLOW_RIFE3D and min(sp) < 2:
        raise ValueError("the rife3d convention needs every extent >= 2, got %s" % (tuple(pred.shape),))
    tau_abs, tau_rel = (float(v) for v in tau)
    if not (0 <= tau_abs < float("inf") and 0 <= tau_rel < float("inf")):
        raise ValueError("tau must be two finite values >= 0, got %r" % (tau,))
    N = int(pred.shape[0])
    mshape = (N,) + sp
    valid = _flow_mask("valid", valid, mshape, pred.device)
    noc_m = _flow_mask("noc", noc, mshape, pred.device)
    emap = torch.empty(mshape, dtype=torch.float32, device=pred.device) if return_map else None
    if N == 0:
        res = {k: torch.empty(0, dtype=torch.float64, device=pred.device) for k in _FLOW_KEYS}
        if return_map:
            res["epe_map"] = emap
        return res
    lib = _lib.lib()
    nb = (lib.fs_flow_metrics2d_ws_bytes(N, nd, *sp) if nd == 2 else
          lib.fs_flow_metrics3d_ws_bytes(N, nd, *sp, conv))
    if nb < 0:
        _lib.check(int(-nb), "fs_flow_metrics%dd_ws_bytes" % nd)
    ws = torch.empty((nb + 7) // 8, dtype=torch.float64, device=pred.device)
    out = torch.empty(N, FLOW_METRICS_K, dtype=torch.float64, device=pred.device)
    nbytes, flops = flow_metrics_cost(pred.shape, (valid is not None) + (noc_m is not None), return_map)
    P = 1
    for v in sp:
        P *= v
    pbs = pred.stride(0) if N > 1 else nd * P  # (a single flow's batch stride is never used)
    gbs = gt.stride(0) if N > 1 else nd * P
    args = (pred.data_ptr(), gt.data_ptr(), N, nd) + sp + (pbs, gbs, _ptr(valid), _ptr(noc_m))
    args += ((conv,) if nd == 3 else ()) + (tau_abs, tau_rel, _ptr(emap), ws.data_ptr(), out.data_ptr(), _stream(pred))
    with torch.cuda.device(pred.device):
        _call("fs_flow_metrics%dd" % nd, *args, algo_bytes=nbytes, algo_flops=flops)
    return _flow_stats(out, noc is not None, emap)


_FLOW_KEYS = ("epe", "epe_noc", "epe_occ", "rmse", "ae_deg", "fl", "fl_noc", "fl_occ", "max_epe", "n_valid", "n_noc",
              "n_nonfinite")


def _flow_stats(out, split, emap):
    """The per-flow statistics from the kernel's sums `out` [N, K] (fp64)."""
    nan = torch.tensor(float("nan"), dtype=torch.float64, device=out.device)

    def div(a, b):
        return torch.where(b > 0, a / torch.where(b > 0, b, torch.ones_like(b)), nan)

    n, s1, s2, sae, nout, mx = (out[:, k] for k in range(6))
    nn, s1n, s2n, saen, noutn = (out[:, k] for k in range(6, 11))
    nf, nfn = out[:, 11], out[:, 12]
    fin, finn = n - nf, nn - nfn
    res = {"epe": div(s1, fin), "rmse": torch.sqrt(div(s2, fin)), "ae_deg": torch.rad2deg(div(sae, fin)),
           "fl": div(nout, n), "max_epe": torch.where(fin > 0, mx, nan), "n_valid": n, "n_nonfinite": nf}
    if split:
        res.update(epe_noc=div(s1n, finn), epe_occ=div(s1 - s1n, fin - finn), fl_noc=div(noutn, nn),
                   fl_occ=div(nout - noutn, n - nn), n_noc=nn)
    else:
        res.update({k: torch.full_like(n, float("nan")) for k in ("epe_noc", "epe_occ", "fl_noc", "fl_occ", "n_noc")})
    if emap is not None:
        res["epe_map"] = emap
    return res


# --------------------------------------------------------------------------------------------
# Flow quality without ground truth: forward-backward consistency and the photometric error of the warp
# (fs_flow_consistency{2,3}d)
# --------------------------------------------------------------------------------------------
FLOW_CONSISTENCY_K = 13  # FS_FLOW_CONSISTENCY_K: the per-pair sums, in the order include/flowsci_hip.h documents
FC_NOT_VALID, FC_CONSISTENT, FC_OCCLUDED, FC_OUTGOING, FC_NONFINITE = 0, 1, 2, 3, 4  # FS_FC_*: class_map codes
_CONSISTENCY_KEYS = ("fb_mean", "fb_rmse", "fb_max", "fb_mean_noc", "occ_frac", "out_frac", "warp_l1", "warp_l1_noc",
                     "warp_psnr", "warp_psnr_noc", "n_valid", "n_inside", "n_noc", "n_occ", "n_out", "n_nonfinite")


def flow_consistency_cost(shape, images=True, maps=False):
    """(HBM bytes, flops) the algorithm needs for one flow_consistency call on [N,C,*spatial] flow pairs: both flows
    read once (the 2^C corner reads of flow_b overlap between neighbours: each of its elements is needed about once),
    both frames once if given, the uint8 class map and the fp32 residual map written once if asked.  Flops per element:
    the 2^C corner weights (C - 1 products each), 2 per corner and gathered plane, ~8 C for the sums and the test."""
    n = 1
    for s in shape:
        n *= int(s)
    C = int(shape[1])
    elems = n // C
    planes = C + (1 if images else 0)
    flops = (1 << C) * (C - 1) + 2 * (1 << C) * planes + 8 * C + (6 if images else 0)
    return 2 * 4 * n + (2 * 4 * elems if images else 0) + (5 * elems if maps else 0), flops * elems


def _flow_image(name, t, shape, device):
    if not isinstance(t, torch.Tensor):
        raise ValueError("%s must be a tensor or None" % name)
    if not t.is_cuda:
        raise ValueError("%s must live on a GPU (the HIP hot path has no CPU fallback); got %s" % (name, t.device))
    if t.device != device:
        raise ValueError("%s must be on the flows' device %s, got %s" % (name, device, t.device))
    if t.dim() == len(shape) + 1 and t.shape[1] == 1:
        t = t[:, 0]
    if tuple(t.shape) != tuple(shape):
        raise ValueError("%s must be [N,*spatial] = %s, got %s" % (name, tuple(shape), tuple(t.shape)))
    return t.to(torch.float32).contiguous()


def flow_consistency(flow_f, flow_b, img0=None, img1=None, valid=None, alpha=(0.01, 0.5), return_maps=False):
    """Label-free quality of N flow pairs, one launch (fs_flow_consistency{2,3}d): the forward-backward residual, the
    occluded / outgoing / consistent classes it implies and the photometric error of the flow-warped frame.

    flow_f, flow_b: [N,2,H,W] or [N,3,D,H,W] displacements in elements (channel 0 along W, 1 along H, 2 along D) on a
    GPU, operands as flow_metrics takes them (a channel slice is read in place).  flow_f maps frame a to frame b on
    a's grid, flow_b maps b to a on b's grid; the other direction is the same call with flows and frames swapped.
    img0, img1: optional frames a and b, [N,*sp] (or [N,1,*sp]), both or neither.  valid: optional bool / uint8 [N,*sp].
    alpha = (alpha1, alpha2): with Fbw = flow_b sampled (bi- / trilinearly) at x + flow_f(x), an element is occluded
    when |flow_f + Fbw|^2 > alpha1 (|flow_f|^2 + |Fbw|^2) + alpha2 (UnFlow's test and thresholds), consistent (noc)
    otherwise; it is outgoing when x + flow_f(x) leaves the grid (border inclusive) and nonfinite when flow_f(x), Fbw or
    (with images) img0(x) or the sampled img1 is not finite.  inside = occluded + consistent.

    Returns a dict of fp64 [N] tensors: fb_mean, fb_rmse, fb_max (the residual |flow_f + Fbw| over inside), fb_mean_noc,
    occ_frac = n_occ / n_inside, out_frac = n_out / n_valid, warp_l1, warp_l1_noc (mean |img1 warped - img0| over inside /
    noc), warp_psnr, warp_psnr_noc (-10 log10 of the mean squared error: frames in [0,1]; the four are NaN without
    images), n_valid, n_inside, n_noc, n_occ, n_out, n_nonfinite.  A ratio with an empty denominator is NaN.  With
    return_maps=True also class_map (uint8 [N,*sp]: 0 not valid, 1 consistent, 2 occluded, 3 outgoing, 4 nonfinite),
    res_map (fp32 [N,*sp]: the residual at every element, NaN where outgoing or nonfinite) and noc (bool,
    class_map == 1: the mask flow_metrics takes as `noc`).  A measurement on detached values: nothing is differentiated."""
    if not isinstance(flow_f, torch.Tensor) or flow_f.dim() not in (4, 5):
        raise ValueError("flow_f must be [N,2,H,W] or [N,3,D,H,W], got %s" %
                         (tuple(flow_f.shape) if isinstance(flow_f, torch.Tensor) else type(flow_f).__name__,))
    nd = flow_f.dim() - 2
    flow_f = _flow_operand("flow_f", flow_f.detach(), nd)
    flow_b = _flow_operand("flow_b", flow_b.detach() if isinstance(flow_b, torch.Tensor) else flow_b, nd)
    if flow_f.shape != flow_b.shape:
        raise ValueError("flow_f and flow_b differ in shape: %s vs %s" % (tuple(flow_f.shape), tuple(flow_b.shape)))
    if flow_f.device != flow_b.device:
        raise ValueError("flow_f and flow_b are on different devices")
    if (img0 is None) != (img1 is None):
        raise ValueError("img0 and img1 go together: pass both or neither")
    a1, a2 = (float(v) for v in alpha)
    if not (0 <= a1 < float("inf") and 0 <= a2 < float("inf")):
        raise ValueError("alpha must be two finite values >= 0, got %r" % (alpha,))
    sp = tuple(int(s) for s in flow_f.shape[2:])
    N = int(flow_f.shape[0])
    mshape = (N,) + sp
    dev = flow_f.device
    images = img0 is not None
    if images:
        img0 = _flow_image("img0", img0.detach() if isinstance(img0, torch.Tensor) else img0, mshape, dev)
        img1 = _flow_image("img1", img1.detach() if isinstance(img1, torch.Tensor) else img1, mshape, dev)
    valid = _flow_mask("valid", valid, mshape, dev)
    cmap = torch.empty(mshape, dtype=torch.uint8, device=dev) if return_maps else None
    rmap = torch.empty(mshape, dtype=torch.float32, device=dev) if return_maps else None
    if N == 0:
        res = {k: torch.empty(0, dtype=torch.float64, device=dev) for k in _CONSISTENCY_KEYS}
    else:
        lib = _lib.lib()
        nb = getattr(lib, "fs_flow_consistency%dd_ws_bytes" % nd)(N, nd, *sp)
        if nb < 0:
            _lib.check(int(-nb), "fs_flow_consistency%dd_ws_bytes" % nd)
        ws = torch.empty((nb + 7) // 8, dtype=torch.float64, device=dev)
        out = torch.empty(N, FLOW_CONSISTENCY_K, dtype=torch.float64, device=dev)
        nbytes, flops = flow_consistency_cost(flow_f.shape, images, return_maps)
        P = 1
        for v in sp:
            P *= v
        fbs = flow_f.stride(0) if N > 1 else nd * P  # (a single flow's batch stride is never used)
        bbs = flow_b.stride(0) if N > 1 else nd * P
        args = (flow_f.data_ptr(), flow_b.data_ptr(), N, nd) + sp + (fbs, bbs, _ptr(img0), _ptr(img1), _ptr(valid),
                                                                      a1, a2, _ptr(cmap), _ptr(rmap), ws.data_ptr(),
                                                                      out.data_ptr(), _stream(flow_f))
        with torch.cuda.device(dev):
            _call("fs_flow_consistency%dd" % nd, *args, algo_bytes=nbytes, algo_flops=flops)
        res = _consistency_stats(out, images)
    if return_maps:
        res.update(class_map=cmap, res_map=rmap, noc=cmap == FC_CONSISTENT)
    return res


def _consistency_stats(out, images):
    """The per-pair statistics from the kernel's sums `out` [N, K] (fp64)."""
    nan = torch.tensor(float("nan"), dtype=torch.float64, device=out.device)

    def div(a, b):
        return torch.where(b > 0, a / torch.where(b > 0, b, torch.ones_like(b)), nan)

    n, nf, nout, nocc, nnoc = (out[:, k] for k in range(5))
    nin = nocc + nnoc
    res = {"fb_mean": div(out[:, 5], nin), "fb_rmse": torch.sqrt(div(out[:, 6], nin)),
           "fb_max": torch.where(nin > 0, out[:, 7], nan), "fb_mean_noc": div(out[:, 8], nnoc),
           "occ_frac": div(nocc, nin), "out_frac": div(nout, n),
           "n_valid": n, "n_inside": nin, "n_noc": nnoc, "n_occ": nocc, "n_out": nout, "n_nonfinite": nf}
    if images:
        res.update(warp_l1=div(out[:, 9], nin), warp_l1_noc=div(out[:, 11], nnoc),
                   warp_psnr=-10.0 * torch.log10(div(out[:, 10], nin)),
                   warp_psnr_noc=-10.0 * torch.log10(div(out[:, 12], nnoc)))
    else:
        res.update({k: torch.full_like(n, float("nan")) for k in ("warp_l1", "warp_l1_noc", "warp_psnr", "warp_psnr_noc")})
    return res


# --------------------------------------------------------------------------------------------
# Pathlines: particles advected through consecutive displacement fields (fs_advect{2,3}d)
# --------------------------------------------------------------------------------------------
ADV_ALIVE, ADV_OUT, ADV_NONFINITE = 0, 1, 2  # FS_ADV_*: status codes
_ADV_METHODS = {"euler": (0, 1), "rk2": (1, 2), "rk4": (2, 4)}  # name -> (FS_ADV_*, samples per substep)


def advect_cost(shape, P, K, method="euler", substeps=1, record=False):
    """(HBM bytes, flops) the algorithm needs for one advect call of P particles through K fields of spatial `shape`:
    every field element the gathers can reach read once (at most the whole fields, at most what the
    K * substeps * stages samples of 2^C corners x C planes ask for), pos_in read and the positions written once (per
    step with record), status and steps read and written.  Flops per sample: the 2^C corner weights (C - 1 products
    each), 2 per corner and plane, ~4 C for clamp / floor / fractions, 2 C for the stage point; ~4 C per substep for
    the update and its classification (RK4: 5 C more for the stage sum)."""
    if method not in _ADV_METHODS:
        raise ValueError("method must be one of %s, got %r" % (sorted(_ADV_METHODS), method))
    C = len(shape)
    plane = 1
    for s in shape:
        plane *= int(s)
    stages = _ADV_METHODS[method][1]
    samples = int(P) * int(K) * int(substeps) * stages
    field = 4 * min(int(K) * C * plane, samples * (1 << C) * C)
    nbytes = field + 4 * C * int(P) * (1 + (int(K) if record else 1)) + 2 * int(P) + 8 * int(P)
    per_sample = (1 << C) * (C - 1) + 2 * (1 << C) * C + 4 * C + 2 * C
    flops = samples * per_sample + int(P) * int(K) * int(substeps) * (4 * C + (5 * C if method == "rk4" else 0))
    return nbytes, flops


def grid_seeds(shape, stride=1, offset=0, device="cuda"):
    """[C, P] fp32 positions of every `stride`-th element of a grid of spatial `shape` ((H,W) or (D,H,W)), starting at
    `offset` along every axis, x fastest: component 0 is x (along W).  With stride 1 and offset 0,
    seeds.view(C, *shape) is the identity field and a [C, P] result views as a [C, *shape] displacement."""
    shape = tuple(int(s) for s in shape)
    if len(shape) not in (2, 3) or min(shape) < 1:
        raise ValueError("shape must be (H,W) or (D,H,W) with every extent >= 1, got %r" % (shape,))
    stride, offset = int(stride), int(offset)
    if stride < 1 or offset < 0:
        raise ValueError("stride must be >= 1 and offset >= 0, got %d and %d" % (stride, offset))
    axes = [torch.arange(offset, s, stride, dtype=torch.float32, device=device) for s in shape]  # slowest first
    mesh = torch.meshgrid(*axes, indexing="ij")
    return torch.stack([m.reshape(-1) for m in mesh[::-1]], 0).contiguous()


def _advect_flows(flows):
    """[K,C,*sp] fp32 on a GPU whose [C,*sp] block per step is contiguous: the step stride may be anything from
    C * prod(sp) up (a stack's every other field, flows[::2], passes as it is); anything else is copied once."""
    if not isinstance(flows, torch.Tensor) or flows.dim() not in (4, 5):
        raise ValueError("flows must be [K,2,H,W] or [K,3,D,H,W], got %s" %
                         (tuple(flows.shape) if isinstance(flows, torch.Tensor) else type(flows).__name__,))
    nd = flows.dim() - 2
    if flows.shape[0] < 1:
        raise ValueError("flows must hold at least one field, got shape %s" % (tuple(flows.shape),))
    return _flow_operand("flows", flows.detach(), nd), nd


def advect(pos, flows, status=None, steps=None, method="euler", substeps=1, scale=1.0, record=False):
    """Move P particles through K consecutive displacement fields in one launch (fs_advect{2,3}d).

    pos: [C,P] fp32 on a GPU, component 0 = x (along W), 1 = y, 2 = z, in elements; rows may be strided (a [C,P] slice
    of a trajectory passes as it is), elements of a row are contiguous.  flows: [K,2,H,W] or [K,3,D,H,W] displacements
    in elements (channel 0 along W), field k being the motion over step k on that step's grid; the step stride may be
    anything.  status: optional uint8 [P] of an earlier call (ADV_ALIVE 0, ADV_OUT 1, ADV_NONFINITE 2); None = all
    ALIVE.  steps: optional int32 [P] counts to continue, None to start from 0, False to count nothing (None comes back).
    Neither is modified: the returned tensors are new.  method: "euler", "rk2" (midpoint) or "rk4", each step in
    `substeps` equal parts through the step's own (steady) field; the update is p + (scale / substeps) * velocity.

    All arithmetic is fp64 (include/flowsci_hip.h states the order of operations; tests/advect_ref.py restates it and
    agrees bit for bit); positions are stored as fp32 once per step.  A particle ends when it leaves the box (OUT: it
    keeps its exit point; the border is inside) or meets a non-finite value (NONFINITE: it keeps its last finite
    position); a seed outside the box or not finite ends without moving.

    Returns (pos_out [C,P], status, steps), or with record=True (traj [K+1,C,P] with traj[0] = pos, status, steps).
    Never synchronises.  A measurement on detached values: nothing is differentiated."""
    if method not in _ADV_METHODS:
        raise ValueError("method must be one of %s, got %r" % (sorted(_ADV_METHODS), method))
    substeps = int(substeps)
    if substeps < 1:
        raise ValueError("substeps must be >= 1, got %d" % substeps)
    scale = float(scale)
    if not (-float("inf") < scale < float("inf")):
        raise ValueError("scale must be finite, got %r" % (scale,))
    flows, nd = _advect_flows(flows)
    dev = flows.device
    if not isinstance(pos, torch.Tensor):
        raise ValueError("pos must be a tensor")
    if not pos.is_cuda:
        raise ValueError("pos must live on a GPU (the HIP hot path has no CPU fallback); got %s" % (pos.device,))
    if pos.device != dev:
        raise ValueError("pos must be on the flows' device %s, got %s" % (dev, pos.device))
    if pos.dim() != 2 or pos.shape[0] != nd:
        raise ValueError("pos must be [%d,P] for %d-D flows, got shape %s" % (nd, nd, tuple(pos.shape)))
    pos = pos.detach()
    if pos.dtype != torch.float32:
        pos = pos.to(torch.float32)
    K, P = int(flows.shape[0]), int(pos.shape[1])
    if P > 0 and (pos.stride(1) != 1 or pos.stride(0) < P):
        pos = pos.contiguous()

    def state(name, t, dtype):
        if t is None:
            return torch.zeros(P, dtype=dtype, device=dev)
        if not isinstance(t, torch.Tensor) or t.dtype != dtype or tuple(t.shape) != (P,):
            raise ValueError("%s must be a %s tensor of shape (%d,), got %s" % (
                name, dtype, P, (t.dtype, tuple(t.shape)) if isinstance(t, torch.Tensor) else type(t).__name__))
        if t.device != dev:
            raise ValueError("%s must be on the flows' device %s, got %s" % (name, dev, t.device))
        return t.clone(memory_format=torch.contiguous_format)

    status = state("status", status, torch.uint8)
    steps = None if steps is False else state("steps", steps, torch.int32)
    if record:
        traj = torch.empty(K + 1, nd, P, dtype=torch.float32, device=dev)
        traj[0].copy_(pos)
        out, tss = traj[1:], nd * P
    else:
        traj = out = torch.empty(nd, P, dtype=torch.float32, device=dev)
        tss = 0  # every step overwrites the one slot
    if P == 0:
        return traj, status, steps
    sp = tuple(int(s) for s in flows.shape[2:])
    plane = 1
    for v in sp:
        plane *= v
    fss = flows.stride(0) if K > 1 else nd * plane  # (a single field's step stride is never used)
    nbytes, flops = advect_cost(sp, P, K, method, substeps, record)
    args = (flows.data_ptr(), K, nd) + sp + (fss, pos.data_ptr(), pos.stride(0), P,
                                             out.data_ptr(), tss, P, status.data_ptr(), _ptr(steps),
                                             _ADV_METHODS[method][0], substeps, scale, _stream(flows))
    with torch.cuda.device(dev):
        _call("fs_advect%dd" % nd, *args, algo_bytes=nbytes, algo_flops=flops)
    return traj, status, steps


# --------------------------------------------------------------------------------------------
# FTLE: the flow map of lattice seeds differentiated and reduced to Lyapunov exponents (fs_ftle{2,3}d)
# --------------------------------------------------------------------------------------------
FTLE_NOT_VALID, FTLE_OK, FTLE_ENDED, FTLE_NONFINITE, FTLE_COLLAPSED = 0, 1, 2, 3, 4  # FS_FTLE_*: class codes
FTLE_K = 9  # FS_FTLE_K: the five class counts, then sum, sum of squares, minimum and maximum of the stored FTLE
FTLE_CLASSES = ("not_valid", "ok", "ended", "nonfinite", "collapsed")


def _lattice(lattice):
    lattice = tuple(int(s) for s in lattice)
    if len(lattice) not in (2, 3) or min(lattice) < 2:
        raise ValueError("lattice must be (Gh,Gw) or (Gd,Gh,Gw) with every extent >= 2, got %r" % (lattice,))
    P = 1
    for s in lattice:
        P *= s
    if P > 2 ** 31 - 1:
        raise ValueError("a lattice holds at most 2^31 - 1 nodes, got %r" % (lattice,))
    return lattice, P


def ftle_cost(lattice, with_cg=False):
    """(HBM bytes, flops) the algorithm needs for one ftle call on a lattice (Gh,Gw) or (Gd,Gh,Gw): the C map planes and
    the status read once (neighbours come from the cache), the fp32 exponent and the uint8 class written, with_cg the
    C (C + 1) / 2 tensor planes too.  Flops per node: 2 per entry of J, 2 C - 1 per entry of G, ~30 for the logarithm,
    ~10 for the 2-D closed form or ~45 per Jacobi rotation at a nominal two sweeps of three in 3-D."""
    lattice, P = _lattice(lattice)
    C = len(lattice)
    NG = C * (C + 1) // 2
    nbytes = P * (4 * C + 1 + 5 + (4 * NG if with_cg else 0))
    flops = P * (2 * C * C + NG * (2 * C - 1) + 30 + (10 if C == 2 else 2 * 3 * 45))
    return nbytes, flops


def lattice_seeds(shape, refine=1, device="cuda"):
    """(seeds [C,P] fp32, lattice extents, spacing) of the lattice that refines a grid of spatial `shape` ((H,W) or
    (D,H,W)) `refine` times: (S_c - 1) * refine + 1 nodes per axis at the fp32 of i / refine, x fastest (component 0
    is x, along W, as grid_seeds has it); the extents come slowest first, as `shape` does; spacing = 1 / refine in
    elements.  What ops.advect returns for these seeds is the flow map ops.ftle differentiates."""
    shape = tuple(int(s) for s in shape)
    refine = int(refine)
    if len(shape) not in (2, 3) or min(shape) < 2:
        raise ValueError("shape must be (H,W) or (D,H,W) with every extent >= 2, got %r" % (shape,))
    if refine < 1:
        raise ValueError("refine must be >= 1, got %d" % refine)
    lattice = tuple((s - 1) * refine + 1 for s in shape)
    _lattice(lattice)
    axes = [(torch.arange(n, dtype=torch.float64, device=device) / refine).to(torch.float32) for n in lattice]
    mesh = torch.meshgrid(*axes, indexing="ij")
    return torch.stack([m.reshape(-1) for m in mesh[::-1]], 0).contiguous(), lattice, 1.0 / refine


def ftle(pos, status, lattice, spacing, T, valid=None, accept_out=False, with_cg=False, summary=True):
    """Finite-time Lyapunov exponents of a flow map sampled on a lattice, one launch (fs_ftle{2,3}d).

    pos: [C,P] fp32 on a GPU, the end positions ops.advect returns for lattice_seeds (component 0 = x); rows may be
    strided (a [C,P] slice of a recorded trajectory passes as it is), elements of a row are contiguous.  status: uint8
    [P], advect's.  lattice: (Gh,Gw) or (Gd,Gh,Gw) with P nodes, x fastest.  spacing: the seed spacing in elements, one
    value or one per lattice axis (in the lattice's order).  T: the integration time; only |T| enters.  valid: optional
    bool / uint8 [P] or [*lattice]; nodes outside it get class FTLE_NOT_VALID (they still serve as neighbours).
    accept_out: particles that left the box count with their exit point instead of ending their neighbourhood.

    Per node the map is differentiated along every axis by a central difference where both neighbours are usable, a
    one-sided one where only one is, in fp64; G = J^T J; ftle = ln(sqrt(lambda_max(G))) / |T|, stored as fp32
    (include/flowsci_hip.h states the order of operations; tests/ftle_ref.py restates it).  Classes: FTLE_OK,
    FTLE_ENDED (no difference along some axis), FTLE_NONFINITE (a used map value or the result is not finite),
    FTLE_COLLAPSED (lambda_max == 0); ftle is NaN off FTLE_OK.

    Returns a dict: ftle (fp32 [*lattice]), cls (uint8 [*lattice]); with_cg: cg (fp32 [C(C+1)/2, *lattice], planes xx,
    xy, yy, xz, yz, zz; NaN off OK and COLLAPSED); summary: summary (fp64 [FTLE_K] on the device: the five class
    counts, then sum, sum of squares, minimum and maximum of the stored ftle over the OK nodes -- ftle_stats reads it).
    Never synchronises.  A measurement on detached values: nothing is differentiated."""
    lattice, P = _lattice(lattice)
    nd = len(lattice)
    try:
        hs = [float(v) for v in spacing] if hasattr(spacing, "__len__") else [float(spacing)] * nd
    except TypeError:
        raise ValueError("spacing must be a number or one per lattice axis, got %r" % (spacing,))
    if len(hs) != nd or not all(0 < h < float("inf") for h in hs):
        raise ValueError("spacing must be one or %d finite positive values, got %r" % (nd, spacing))
    T = abs(float(T))
    if not (0 < T < float("inf")):
        raise ValueError("T must be finite and non-zero, got %r" % (T,))
    if not isinstance(pos, torch.Tensor) or not isinstance(status, torch.Tensor):
        raise ValueError("pos and status must be tensors")
    if not pos.is_cuda:
        raise ValueError("pos must live on a GPU (the HIP hot path has no CPU fallback); got %s" % (pos.device,))
    dev = pos.device
    if pos.dim() != 2 or tuple(pos.shape) != (nd, P):
        raise ValueError("pos must be [%d,%d] for the lattice %s, got shape %s" % (nd, P, lattice, tuple(pos.shape)))
    if status.dtype != torch.uint8 or status.numel() != P or status.device != dev:
        raise ValueError("status must be a uint8 tensor of %d elements on %s, got %s %s on %s" % (
            P, dev, status.dtype, tuple(status.shape), status.device))
    pos = pos.detach()
    if pos.dtype != torch.float32:
        pos = pos.to(torch.float32)
    if pos.stride(1) != 1 or pos.stride(0) < P:
        pos = pos.contiguous()
    status = status.reshape(-1).contiguous()
    if valid is not None:
        if not isinstance(valid, torch.Tensor) or valid.dtype not in (torch.bool, torch.uint8) or valid.numel() != P:
            raise ValueError("valid must be a bool / uint8 tensor of %d elements or None" % P)
        if valid.device != dev:
            raise ValueError("valid must be on pos's device %s, got %s" % (dev, valid.device))
        valid = valid.reshape(-1).to(torch.uint8).contiguous()
    out = {"ftle": torch.empty(lattice, dtype=torch.float32, device=dev),
           "cls": torch.empty(lattice, dtype=torch.uint8, device=dev)}
    if with_cg:
        out["cg"] = torch.empty((nd * (nd + 1) // 2,) + lattice, dtype=torch.float32, device=dev)
    ws = None
    if summary:
        lib = _lib.lib()
        nb = getattr(lib, "fs_ftle%dd_ws_bytes" % nd)(nd, *lattice)
        if nb < 0:
            _lib.check(int(-nb), "fs_ftle%dd_ws_bytes" % nd)
        ws = torch.empty((nb + 7) // 8, dtype=torch.float64, device=dev)
        out["summary"] = torch.empty(FTLE_K, dtype=torch.float64, device=dev)
    # component 0 and axis 0 run along x: the lattice's last axis
    inv_h = (ctypes.c_double * nd)(*[1.0 / h for h in hs[::-1]])
    inv_2h = (ctypes.c_double * nd)(*[1.0 / (2.0 * h) for h in hs[::-1]])
    nbytes, flops = ftle_cost(lattice, with_cg)
    args = (pos.data_ptr(), pos.stride(0), status.data_ptr(), _ptr(valid), nd) + lattice + (
        inv_h, inv_2h, 1.0 / T, int(bool(accept_out)), out["ftle"].data_ptr(), out["cls"].data_ptr(),
        _ptr(out.get("cg")), _ptr(ws), _ptr(out.get("summary")), _stream(pos))
    with torch.cuda.device(dev):
        _call("fs_ftle%dd" % nd, *args, algo_bytes=nbytes, algo_flops=flops)
    return out


def ftle_stats(summary):
    """A summary of ops.ftle as plain numbers (synchronises): {"counts": {class name: n}, "mean", "std", "min", "max"}
    of the stored FTLE over the OK nodes; the four are NaN when there is none."""
    s = [float(v) for v in summary.cpu().tolist()]
    n = s[FTLE_OK]
    nan = float("nan")
    mean = s[5] / n if n else nan
    var = max(0.0, s[6] / n - mean * mean) if n else nan
    return {"counts": {name: int(s[k]) for k, name in enumerate(FTLE_CLASSES)}, "mean": mean,
            "std": var ** 0.5 if n else nan, "min": s[7] if n else nan, "max": s[8] if n else nan}


# --------------------------------------------------------------------------------------------
# Velocity gradient: divergence, vorticity, Q and lambda2 of step flows (fs_velgrad{2,3}d)
# --------------------------------------------------------------------------------------------
VG_FIELDS = {"div": 1, "vort": 2, "vmag": 4, "q": 8, "l2": 16, "grad": 32}  # FS_VG_*: in the order of the planes
VG_DEFAULT = ("div", "vmag", "q", "l2")
VG_K = 20  # FS_VG_K: four counts, then sum / sum of squares / min / max of div, vmag, q and l2
VG_FLAG_Q, VG_FLAG_L2, VG_FLAG_NONFINITE = 1, 2, 128  # FS_VG_FLAG_*
_VG_STATS = ("div", "vmag", "q", "l2")  # the fields the summary covers, at 4 + 4 n


def _vg_fields(fields):
    """The bitmask of a field selection: names (a list, or comma-separated in a string), or the mask itself."""
    if isinstance(fields, int) and not isinstance(fields, bool):
        mask = fields
    else:
        names = [n.strip() for n in fields.split(",")] if isinstance(fields, str) else list(fields)
        unknown = [n for n in names if n not in VG_FIELDS]
        if unknown:
            raise ValueError("unknown field(s) %r: choose among %s" % (unknown, ", ".join(VG_FIELDS)))
        mask = 0
        for n in names:
            mask |= VG_FIELDS[n]
    if mask <= 0 or mask & ~63:
        raise ValueError("fields must select at least one of %s, got %r" % (", ".join(VG_FIELDS), fields))
    return mask


def velgrad_planes(fields, nd):
    """name -> slice of the NP planes ops.velgrad writes for `fields` in nd dimensions, in the kernel's order: div (1),
    vort (1 in 2-D, 3 in 3-D), vmag (1), q (1), l2 (1), grad (nd * nd, plane r * nd + c = d u_r / d x_c)."""
    mask = _vg_fields(fields)
    if nd not in (2, 3):
        raise ValueError("nd must be 2 or 3, got %r" % (nd,))
    width = {"div": 1, "vort": 3 if nd == 3 else 1, "vmag": 1, "q": 1, "l2": 1, "grad": nd * nd}
    planes, p = {}, 0
    for name, bit in VG_FIELDS.items():
        if mask & bit:
            planes[name] = slice(p, p + width[name])
            p += width[name]
    return planes


def velgrad_cost(shape, K=1, fields=VG_DEFAULT, with_flags=True):
    """(HBM bytes, flops) the algorithm needs for one velgrad call on K step flows of spatial `shape` ((H,W) or
    (D,H,W)): the C planes read once (neighbours come from the cache), the NP selected planes and the flag byte
    written: 4 C + 4 NP (+ 1) per node.  Flops per node: 3 per entry of J, C - 1 for div, C for vort, 2 C for vmag,
    ~25 (3-D) / ~10 (2-D) for S, Omega and q, and for l2 ~45 for M plus ~45 per Jacobi rotation at a nominal two
    sweeps of three in 3-D, ~15 for the closed form in 2-D."""
    shape, P = _lattice(shape)
    C = len(shape)
    mask = _vg_fields(fields)
    NP = sum(s.stop - s.start for s in velgrad_planes(mask, C).values())
    K = int(K)
    if K < 1:
        raise ValueError("K must be >= 1, got %d" % K)
    nbytes = K * P * (4 * C + 4 * NP + (1 if with_flags else 0))
    per = 3 * C * C
    per += (C - 1) if mask & 1 else 0
    per += C if mask & 6 else 0
    per += 2 * C if mask & 4 else 0
    per += (25 if C == 3 else 10) if mask & 24 else 0
    per += (45 + 2 * 3 * 45 if C == 3 else 15) if mask & 16 else 0
    return nbytes, K * P * per


def velgrad(flows, fields=VG_DEFAULT, spacing=1.0, scale=1.0, with_flags=True, summary=True):
    """Divergence, vorticity, the Q criterion and lambda2 of K step flows, one launch (fs_velgrad{2,3}d).

    flows: [K,2,H,W] or [K,3,D,H,W] fp32 displacements on a GPU, in elements, channel 0 along W; the step stride may be
    anything (stack[1::2] is read in place).  fields: names out of div, vort, vmag, q, l2, grad (a list or a
    comma-separated string).  spacing: the node spacing, one value or one per axis in the tensor's axis order
    ((D,)H,W).  scale: the reciprocal of the time a step spans, one value or K: velocity = displacement * scale.

    Per node the velocity is differentiated along every axis by a central difference where both neighbours exist, a
    one-sided one at the border, in fp64: J[r][c] = d u_r / d x_c; div = tr J; vort = curl u (a scalar in 2-D), vmag
    its magnitude; q = (||Omega||^2 - ||S||^2) / 2; l2 = the median eigenvalue of S^2 + Omega^2 (2-D: of the planar field
    embedded in 3-D).  include/flowsci_hip.h states the order of operations; tests/velgrad_ref.py restates it and
    agrees bit for bit on div, vort, q and grad.  A node at which a used value or a selected result is not finite is NaN
    in every plane.

    Returns a dict: out (fp32 [K,NP,*sp]), planes (name -> slice of the NP planes, velgrad_planes), with_flags: flags
    (uint8 [K,*sp]: VG_FLAG_Q q > 0, VG_FLAG_L2 l2 < 0, VG_FLAG_NONFINITE), summary: summary (fp64 [K,VG_K] on the
    device -- velgrad_stats reads it).  Never synchronises.  A measurement on detached values: nothing is
    differentiated."""
    mask = _vg_fields(fields)
    flows, nd = _advect_flows(flows)
    sp, P = _lattice(flows.shape[2:])
    K = int(flows.shape[0])
    try:
        hs = [float(v) for v in spacing] if hasattr(spacing, "__len__") else [float(spacing)] * nd
        ss = [float(v) for v in scale] if hasattr(scale, "__len__") else [float(scale)] * K
    except TypeError:
        raise ValueError("spacing and scale must be numbers or sequences of numbers, got %r and %r" % (spacing, scale))
    if len(hs) != nd or not all(0 < h < float("inf") for h in hs):
        raise ValueError("spacing must be one or %d finite positive values, got %r" % (nd, spacing))
    if len(ss) != K or not all(0 < s < float("inf") for s in ss):
        raise ValueError("scale must be one or %d finite positive values, got %r" % (K, scale))
    dev = flows.device
    planes = velgrad_planes(mask, nd)
    NP = sum(s.stop - s.start for s in planes.values())
    res = {"out": torch.empty((K, NP) + sp, dtype=torch.float32, device=dev), "planes": planes}
    if with_flags:
        res["flags"] = torch.empty((K,) + sp, dtype=torch.uint8, device=dev)
    ws = None
    if summary:
        nb = getattr(_lib.lib(), "fs_velgrad%dd_ws_bytes" % nd)(K, nd, *sp)
        if nb < 0:
            _lib.check(int(-nb), "fs_velgrad%dd_ws_bytes" % nd)
        ws = torch.empty((nb + 7) // 8, dtype=torch.float64, device=dev)
        res["summary"] = torch.empty((K, VG_K), dtype=torch.float64, device=dev)
    # component 0 and axis 0 run along x: the tensor's last axis
    inv_h = (ctypes.c_double * nd)(*[1.0 / h for h in hs[::-1]])
    inv_2h = (ctypes.c_double * nd)(*[1.0 / (2.0 * h) for h in hs[::-1]])
    fss = flows.stride(0) if K > 1 else nd * P  # (a single field's step stride is never used)
    nbytes, flops = velgrad_cost(sp, K, mask, with_flags)
    args = (flows.data_ptr(), K, nd) + sp + (fss, inv_h, inv_2h, (ctypes.c_double * K)(*ss), mask,
                                             res["out"].data_ptr(), _ptr(res.get("flags")), _ptr(ws),
                                             _ptr(res.get("summary")), _stream(flows))
    with torch.cuda.device(dev):
        _call("fs_velgrad%dd" % nd, *args, algo_bytes=nbytes, algo_flops=flops)
    return res


def velgrad_stats(summary, nodes):
    """The summary of ops.velgrad as plain numbers (synchronises): one dict per step with n_finite, n_nonfinite,
    frac_q_pos, frac_l2_neg, frac_both (vortex volume fractions of the `nodes` nodes of a step), rms_div, enstrophy (the
    mean of vmag^2 / 2) and, per field of div, vmag, q, l2, NAME_mean, NAME_std, NAME_min, NAME_max over the finite
    nodes.  What depends on a field that was not selected, or on finite nodes when there is none, is NaN."""
    rows = summary.cpu().tolist()
    nodes = int(nodes)
    nan = float("nan")
    out = []
    for s in (rows if summary.dim() == 2 else [rows]):
        n = nodes - int(s[0])
        r = {"n_finite": n, "n_nonfinite": int(s[0]), "frac_q_pos": s[1] / nodes, "frac_l2_neg": s[2] / nodes,
             "frac_both": s[3] / nodes}
        for i, name in enumerate(_VG_STATS):
            s1, s2, mn, mx = s[4 + 4 * i:8 + 4 * i]
            mean = s1 / n if n else nan
            var = max(0.0, s2 / n - mean * mean) if n and s2 == s2 else nan
            r.update({name + "_mean": mean, name + "_std": var ** 0.5, name + "_min": mn if n else nan,
                      name + "_max": mx if n else nan})
        r["rms_div"] = (s[5] / n) ** 0.5 if n else nan
        r["enstrophy"] = 0.5 * s[9] / n if n else nan
        out.append(r)
    return out


# --------------------------------------------------------------------------------------------
# Regions: connected components of flag maps, their table, and where the flow carries them
# (fs_label_regions{2,3}d, fs_region_stats{2,3}d, fs_region_follow{2,3}d)
# --------------------------------------------------------------------------------------------
REGION_TILE = {2: (32, 64), 3: (8, 8, 32)}  # FS_REGION_TILE*: the tile one workgroup labels in LDS
REGION_OUT, REGION_TO_BACKGROUND = -1, -2   # FS_REGION_*: codes of fs_region_follow's dst
REGION_MAX_WEIGHTS = 8                      # FS_REGION_MAX_WEIGHTS
_REGION_CONN = {"face": 0, "full": 1}


def _region_grid(sp):
    sp = tuple(int(s) for s in sp)
    P = 1
    for s in sp:
        P *= s
    if len(sp) not in (2, 3) or min(sp) < 1:
        raise ValueError("a region grid is (H,W) or (D,H,W) with every extent >= 1, got %r" % (sp,))
    if P >= 2 ** 31 - 1:
        raise ValueError("a step holds fewer than 2^31 - 1 nodes, got %r" % (sp,))
    return sp, P


def regions_cost(shape, K=1, op="label", F=0, fg_fraction=1.0):
    """(HBM bytes, flops) the algorithm needs for one call of a region op ("label", "stats" or "follow") on K maps of
    spatial `shape`.  label: the mask byte read and the label written per node (the parent array's traffic between the
    launches is the algorithm's own, not compulsory).  stats: the label and F weights read per node.  follow (K - 1
    steps): the label and the C flow planes read and dst written per node, one gathered label per foreground node
    (fg_fraction of them).  The work is integer work: flops 0."""
    sp, P = _region_grid(shape)
    C = len(sp)
    K, F = int(K), int(F)
    if K < 1 or not 0 <= F <= REGION_MAX_WEIGHTS:
        raise ValueError("K must be >= 1 and F in 0..%d, got %d and %d" % (REGION_MAX_WEIGHTS, K, F))
    if op == "label":
        return K * P * (1 + 4), 0
    if op == "stats":
        return K * P * (4 + 4 * F), 0
    if op == "follow":
        return max(0, K - 1) * (P * (4 + 4 * C + 4) + 4 * int(round(float(fg_fraction) * P))), 0
    raise ValueError("op must be 'label', 'stats' or 'follow', got %r" % (op,))


def label_regions(mask, require=VG_FLAG_Q, reject=VG_FLAG_NONFINITE, connectivity="face"):
    """Connected components of K flag maps in one call (fs_label_regions{2,3}d).

    mask: uint8 [K,H,W] or [K,D,H,W] on a GPU; the step stride may be anything (mask[1::2] is read in place).  A node is
    foreground iff (m & require) == require and (m & reject) == 0: with the defaults ops.velgrad's flags go in as they
    are (q > 0 and finite).  connectivity: "face" (4 / 6 neighbours) or "full" (8 / 26).

    Returns a dict on the device: labels (int32 [K,*sp]; background 0, a foreground node carries 1 + the smallest linear
    index, within its step, of any node of its component: the result does not depend on the order of merges),
    n_regions (int32 [K]) and status (int32 [1]: 0, or bit 0 when a loop ran into its iteration cap -- region_table
    checks it).  Never synchronises."""
    if not isinstance(mask, torch.Tensor):
        raise ValueError("mask must be a tensor")
    if not mask.is_cuda:
        raise ValueError("mask must live on a GPU (the HIP hot path has no CPU fallback); got %s" % (mask.device,))
    if mask.dtype != torch.uint8 or mask.dim() not in (3, 4):
        raise ValueError("mask must be uint8 [K,H,W] or [K,D,H,W], got %s %s" % (mask.dtype, tuple(mask.shape)))
    if min(mask.shape) < 1:
        raise ValueError("mask must have no empty axis, got shape %s" % (tuple(mask.shape),))
    if connectivity not in _REGION_CONN:
        raise ValueError("connectivity must be 'face' or 'full', got %r" % (connectivity,))
    require, reject = int(require), int(reject)
    if not (0 <= require <= 255 and 0 <= reject <= 255):
        raise ValueError("require and reject are bytes, got %r and %r" % (require, reject))
    sp, P = _region_grid(mask.shape[1:])
    nd = len(sp)
    K = int(mask.shape[0])
    mask = mask.detach()
    if not mask[0].is_contiguous() or (K > 1 and mask.stride(0) < P):
        mask = mask.contiguous()
    dev = mask.device
    res = {"labels": torch.empty((K,) + sp, dtype=torch.int32, device=dev),
           "n_regions": torch.empty(K, dtype=torch.int32, device=dev),
           "status": torch.empty(1, dtype=torch.int32, device=dev)}
    nb = getattr(_lib.lib(), "fs_label_regions%dd_ws_bytes" % nd)(K, *sp)
    if nb < 0:
        _lib.check(int(-nb), "fs_label_regions%dd_ws_bytes" % nd)
    ws = torch.empty((nb + 3) // 4, dtype=torch.int32, device=dev)
    nbytes, flops = regions_cost(sp, K, "label")
    with torch.cuda.device(dev):
        _call("fs_label_regions%dd" % nd, mask.data_ptr(), K, *sp, mask.stride(0) if K > 1 else P, require, reject,
              _REGION_CONN[connectivity], res["labels"].data_ptr(), res["n_regions"].data_ptr(),
              res["status"].data_ptr(), ws.data_ptr(), _stream(mask), algo_bytes=nbytes, algo_flops=flops)
    return res


def _region_labels(labels):
    """(labels tensor, status or None) of label_regions' dict or a bare int32 [K,*sp] GPU tensor."""
    status = None
    if isinstance(labels, dict):
        labels, status = labels["labels"], labels.get("status")
    if not isinstance(labels, torch.Tensor):
        raise ValueError("labels must be a tensor or label_regions' result")
    if not labels.is_cuda:
        raise ValueError("labels must live on a GPU (the HIP hot path has no CPU fallback); got %s" % (labels.device,))
    if labels.dtype != torch.int32 or labels.dim() not in (3, 4) or min(labels.shape) < 1:
        raise ValueError("labels must be int32 [K,H,W] or [K,D,H,W], got %s %s" % (labels.dtype, tuple(labels.shape)))
    return labels.contiguous(), status


def region_ranks(labels):
    """(roots, rank, offsets) on the device, by a prefix sum over labels == index + 1 (plumbing: torch): roots bool
    [K,P], rank int32 [K,*sp] -- at a root node its region's dense id within the step, in increasing label order --
    and offsets int64 [K+1], the prefix sums of the regions per step.  Never synchronises."""
    K = int(labels.shape[0])
    P = labels[0].numel()
    roots = labels.view(K, P) == torch.arange(1, P + 1, dtype=torch.int32, device=labels.device)
    csum = torch.cumsum(roots, 1, dtype=torch.int32)
    offsets = torch.zeros(K + 1, dtype=torch.int64, device=labels.device)
    offsets[1:] = torch.cumsum(csum[:, -1].to(torch.int64), 0)
    return roots, (csum - 1).view(labels.shape), offsets


def region_stats(labels, rank, offsets, R, weights=None):
    """The launch behind region_table (fs_region_stats{2,3}d), on device tensors and without a synchronisation: labels
    int32 [K,*sp], rank int32 [K,*sp] (the dense id at every root node), offsets int64 [K+1] on the device, R their last
    entry as a host int, weights fp32 [K,F,*sp] or None.  Returns count (int64 [R]), coord_sum (int64 [R,nd]), bbox (int32
    [R,2,nd]), wsum (fp64 [R,F]), wmin, wmax (fp32 [R,F]) on the device."""
    K, sp = int(labels.shape[0]), tuple(int(s) for s in labels.shape[1:])
    nd = len(sp)
    dev = labels.device
    F = 0 if weights is None else int(weights.shape[1])
    R = int(R)
    count = torch.empty(R, dtype=torch.int64, device=dev)
    coord = torch.empty((R, nd), dtype=torch.int64, device=dev)
    bbox = torch.empty((R, 2, nd), dtype=torch.int32, device=dev)
    wsum = torch.empty((R, F), dtype=torch.float64, device=dev)
    wmin = torch.empty((R, F), dtype=torch.float32, device=dev)
    wmax = torch.empty((R, F), dtype=torch.float32, device=dev)
    nbytes, flops = regions_cost(sp, K, "stats", F)
    if R > 0:
        with torch.cuda.device(dev):
            _call("fs_region_stats%dd" % nd, labels.data_ptr(), rank.data_ptr(), offsets.data_ptr(), _ptr(weights), K, F,
                  *sp, R, count.data_ptr(), coord.data_ptr(), bbox.data_ptr(), wsum.data_ptr(), wmin.data_ptr(),
                  wmax.data_ptr(), _stream(labels), algo_bytes=nbytes, algo_flops=flops)
    return count, coord, bbox, wsum, wmin, wmax


def region_table(labels, weights=None, names=None):
    """One row per region of K label maps (fs_region_stats{2,3}d).

    labels: label_regions' result (its status is checked: FlowsciKernelError when set) or its int32 labels.  weights:
    optional fp32 [K,F,*sp] on the same device, F <= 8, finite on foreground nodes (ops.velgrad's planes are, under the
    default reject bit); names: F names for the columns (default w0, w1, ...).

    The number of rows R depends on the data, so this SYNCHRONISES: once, to learn the regions' offsets (and the status);
    the finished rows then come to the host in one integer transfer (and one floating-point one with weights).  Ranking the roots is a prefix sum over
    labels == index + 1 (torch); everything per node is the kernel's.

    Returns host numpy arrays over the R rows, step by step in increasing label order: step, label (int32), count
    (int64), centroid (fp64 [R,nd], exact: integer sums / count), bbox (int32 [R,2,nd], inclusive), per weight
    NAME_sum, NAME_mean (fp64), NAME_min, NAME_max (fp32); offsets (int64 [K+1]: rows offsets[k] .. offsets[k+1] are
    step k's); and rank, the int32 [K,*sp] DEVICE tensor of dense ids at root nodes, for region_links."""
    labels, status = _region_labels(labels)
    K, sp = int(labels.shape[0]), tuple(int(s) for s in labels.shape[1:])
    sp, P = _region_grid(sp)
    nd = len(sp)
    dev = labels.device
    F = 0
    if weights is not None:
        weights = _need_cuda_f32("weights", weights, nd + 2)
        F = int(weights.shape[1])
        if tuple(weights.shape) != (K, F) + sp or not 1 <= F <= REGION_MAX_WEIGHTS or weights.device != dev:
            raise ValueError("weights must be [K,F,*sp] = [%d, 1..%d, %s] on %s, got %s on %s" %
                             (K, REGION_MAX_WEIGHTS, sp, dev, tuple(weights.shape), weights.device))
    names = ["w%d" % i for i in range(F)] if names is None else [str(n) for n in names]
    if len(names) != F or len(set(names)) != F:
        raise ValueError("names must be %d distinct names, got %r" % (F, names))
    roots, rank, offsets = region_ranks(labels)
    head = torch.cat([offsets, (status if status is not None else offsets[:1]).to(torch.int64).view(-1)[:1]]).cpu()
    if status is not None and int(head[-1]) != 0:
        raise _lib.FlowsciKernelError("fs_label_regions: a union-find loop ran into its iteration cap (status %d)"
                                      % int(head[-1]))
    off = head[:K + 1].numpy().copy()
    R = int(off[-1])
    count, coord, bbox, wsum, wmin, wmax = region_stats(labels, rank, offsets, R, weights)
    # every region's label, scattered to its row from its root node (the other nodes write a spare row): no second sync
    rows = torch.where(roots, offsets[:K, None] + rank.view(K, P), R)
    label = torch.empty(R + 1, dtype=torch.int32, device=dev)
    label.scatter_(0, rows.view(-1), torch.arange(1, P + 1, dtype=torch.int32, device=dev).expand(K, P).reshape(-1))
    del rows
    ints = torch.cat([count, coord.reshape(-1), bbox.reshape(-1).to(torch.int64),
                      label[:R].to(torch.int64)]).cpu().numpy()  # one transfer
    cnt = ints[:R].copy()
    c1, c2 = R + R * nd, R + 3 * R * nd
    tab = {"step": _np.repeat(_np.arange(K, dtype=_np.int32), _np.diff(off)), "label": ints[c2:].astype(_np.int32),
           "count": cnt, "centroid": ints[R:c1].reshape(R, nd).astype(_np.float64) / _np.maximum(cnt, 1)[:, None],
           "bbox": ints[c1:c2].reshape(R, 2, nd).astype(_np.int32), "offsets": off, "rank": rank}
    if F:
        flo = torch.cat([wsum.reshape(-1), wmin.reshape(-1).double(), wmax.reshape(-1).double()]).cpu().numpy()  # fp32 -> fp64 is exact
        ws_ = flo[:R * F].reshape(R, F)
        mn_, mx_ = (flo[i * R * F:(i + 1) * R * F].reshape(R, F).astype(_np.float32) for i in (1, 2))
        for i, n in enumerate(names):
            tab[n + "_sum"] = ws_[:, i].copy()
            tab[n + "_mean"] = ws_[:, i] / _np.maximum(cnt, 1)
            tab[n + "_min"] = mn_[:, i].copy()
            tab[n + "_max"] = mx_[:, i].copy()
    return tab


def region_follow(labels, flows):
    """dst (int32 [K-1,*sp] on the device) of fs_region_follow{2,3}d: for every foreground node of map j the label of map
    j + 1 its step flow carries it onto (x + u(x) in fp32, rounded half to even), REGION_OUT (-1) when that leaves the
    grid or is not finite, REGION_TO_BACKGROUND (-2) when it lands on background; 0 on background.  flows: [K-1 or
    more, C, *sp] fp32, channel 0 along W, any step stride.  Never synchronises."""
    labels, _ = _region_labels(labels)
    K, sp = int(labels.shape[0]), tuple(int(s) for s in labels.shape[1:])
    sp, P = _region_grid(sp)
    nd = len(sp)
    if K < 2:
        raise ValueError("following needs at least two label maps, got %d" % K)
    if not isinstance(flows, torch.Tensor) or flows.dim() != nd + 2 or flows.shape[0] < K - 1 or \
            tuple(flows.shape[2:]) != sp:
        raise ValueError("flows must be [>= %d, %d, %s], got %s" %
                         (K - 1, nd, sp, tuple(flows.shape) if isinstance(flows, torch.Tensor) else type(flows).__name__))
    flows = _flow_operand("flows", flows.detach(), nd)
    if flows.device != labels.device:
        raise ValueError("labels and flows must be on one device, got %s and %s" % (labels.device, flows.device))
    dst = torch.empty((K - 1,) + sp, dtype=torch.int32, device=labels.device)
    nbytes, flops = regions_cost(sp, K, "follow")
    with torch.cuda.device(labels.device):
        _call("fs_region_follow%dd" % nd, labels.data_ptr(), flows.data_ptr(), K, nd, *sp,
              flows.stride(0) if flows.shape[0] > 1 else nd * P, dst.data_ptr(), _stream(labels), algo_bytes=nbytes,
              algo_flops=flops)
    return dst


def region_links(labels, flows, table):
    """Flow-guided links between consecutive label maps: fs_region_follow, then equal (source region, destination)
    pairs counted on the device (integer plumbing: torch.unique over one int64 key per foreground node).

    table: region_table's result for the same labels (its rank and offsets are used).  Returns a list with one dict of
    host arrays per step pair j -> j + 1: src, dst (dense ids within their steps) and count (nodes of src carried onto
    dst), and per source region of step j n_out (nodes leaving the grid) and n_to_background.  Synchronises."""
    labels, _ = _region_labels(labels)
    K = int(labels.shape[0])
    P = labels[0].numel()
    dst = region_follow(labels, flows).view(K - 1, P)
    off = table["offsets"]
    rank = table["rank"].view(K, P)
    sizes = [int(off[k + 1] - off[k]) for k in range(K)]
    M = max(sizes) + 2
    if int(off[K]) * M >= 2 ** 63:  # the key below: (global row of the source) * M + destination code
        raise ValueError("%d regions with up to %d per step overflow the 64-bit link key" % (int(off[K]), M - 2))
    base = torch.from_numpy(_np.asarray(off[:K], dtype=_np.int64)).to(labels.device)
    src_lab = labels.view(K, P)[:K - 1]
    fg = src_lab > 0
    jj, ii = fg.nonzero(as_tuple=True)
    src = rank[jj, (src_lab[jj, ii] - 1).long()].long()
    d = dst[jj, ii].long()
    to = torch.where(d > 0, rank[jj + 1, (d - 1).clamp(min=0)].long() + 2, d + 2)  # 0: background, 1: out, 2 + id
    keys, counts = torch.unique((base[jj] + src) * M + to, return_counts=True)
    keys, counts = keys.cpu().numpy(), counts.cpu().numpy()
    grow, kt = keys // M, keys % M
    kj = _np.searchsorted(_np.asarray(off[1:K], dtype=_np.int64), grow, side="right")  # the step of a global row
    ks = grow - _np.asarray(off, dtype=_np.int64)[kj]
    out = []
    for j in range(K - 1):
        sel = kj == j
        s, t, c = ks[sel], kt[sel], counts[sel]
        n_out = _np.zeros(sizes[j], dtype=_np.int64)
        n_bg = _np.zeros(sizes[j], dtype=_np.int64)
        n_out[s[t == 1]] = c[t == 1]
        n_bg[s[t == 0]] = c[t == 0]
        lk = t >= 2
        out.append({"src": s[lk].astype(_np.int64), "dst": (t[lk] - 2).astype(_np.int64), "count": c[lk].astype(_np.int64),
                    "n_out": n_out, "n_to_background": n_bg})
    return out


# --------------------------------------------------------------------------------------------
# Ray casting: volumes to images through a transfer function (fs_raycast3d, fs_brick_range3d)
# --------------------------------------------------------------------------------------------
RC_MODES = {"dvr": 0, "mip": 1}  # FS_RC_DVR, FS_RC_MIP
RC_BRICK = 8                     # FS_RC_BRICK: cells per brick and axis
RC_MAX_TF = 1024                 # FS_RC_MAX_TF
RC_MAX_STEPS = 4194304           # FS_RC_MAX_STEPS


def _rc_volumes(volumes):
    """(volumes, K, (D,H,W), nodes) of fp32 GPU volumes [K,D,H,W]; the step stride is kept where the kernel can use it."""
    if not isinstance(volumes, torch.Tensor):
        raise ValueError("volumes must be a tensor")
    if not volumes.is_cuda:
        raise ValueError("volumes must live on a GPU (the HIP hot path has no CPU fallback); got %s" % (volumes.device,))
    if volumes.dtype != torch.float32 or volumes.dim() != 4:
        raise ValueError("volumes must be float32 [K,D,H,W], got %s %s" % (volumes.dtype, tuple(volumes.shape)))
    K = int(volumes.shape[0])
    sp = tuple(int(s) for s in volumes.shape[1:])
    P = sp[0] * sp[1] * sp[2]
    if K < 1 or K > 65535 or min(sp) < 2 or P > 2 ** 31 - 1:
        raise ValueError("volumes must be 1..65535 volumes with every extent >= 2 and at most 2^31 - 1 nodes, got %s" %
                         (tuple(volumes.shape),))
    volumes = volumes.detach()
    if not volumes[0].is_contiguous() or (K > 1 and volumes.stride(0) < P):
        volumes = volumes.contiguous()
    return volumes, K, sp, P


def _rc_spacing(spacing):
    try:
        hs = [float(v) for v in spacing] if hasattr(spacing, "__len__") else [float(spacing)] * 3
    except TypeError:
        raise ValueError("spacing must be a number or three numbers, got %r" % (spacing,))
    if len(hs) != 3 or not all(0 < h < float("inf") for h in hs):
        raise ValueError("spacing must be one or 3 finite positive values (D,H,W), got %r" % (spacing,))
    return hs


def _rc_bricks(sp):
    return tuple((s - 1 + RC_BRICK - 1) // RC_BRICK for s in sp)


def _rc_image(image):
    try:
        Hi, Wi = (int(v) for v in image)
    except (TypeError, ValueError):
        raise ValueError("image must be (rows, columns), got %r" % (image,))
    if not (1 <= Hi <= 16 * 65535 and 1 <= Wi <= 16 * 65535):
        raise ValueError("image must be (rows, columns) within 1..%d, got %r" % (16 * 65535, image))
    return Hi, Wi


def raycast_cost(shape, image, K=1, dt=None, spacing=1.0, samples=None):
    """(gathered bytes, flops) of one raycast call: every sample gathers the eight corners of its cell (32 bytes; most
    come from lines a neighbouring ray or sample already fetched, so this is the gather traffic of the algorithm, not
    HBM traffic) and costs about 60 flops (position, coverage, seven interpolations, the table, the exponential, the
    blend); a pixel writes 16 bytes.  samples: the samples actually taken (the sum of `counts`); without it the upper
    bound of one box diagonal of steps `dt` per pixel."""
    sp = tuple(int(s) for s in shape)
    if len(sp) != 3 or min(sp) < 2:
        raise ValueError("shape must be (D,H,W) with every extent >= 2, got %r" % (shape,))
    Hi, Wi = _rc_image(image)
    hs = _rc_spacing(spacing)
    K = int(K)
    if K < 1:
        raise ValueError("K must be >= 1, got %d" % K)
    if samples is None:
        step = 0.5 * min(hs) if dt is None else float(dt)
        if not (0 < step < float("inf")):
            raise ValueError("dt must be finite and positive, got %r" % (dt,))
        diag = sum(((n + 1) * h) ** 2 for n, h in zip(sp, hs)) ** 0.5
        samples = K * Hi * Wi * (int(diag / step) + 1)
    samples = int(samples)
    return 32 * samples + 16 * K * Hi * Wi, 60 * samples


def brick_ranges(volumes):
    """The value range of every brick of 8^3 cells (9^3 nodes) of K volumes, one launch (fs_brick_range3d).

    volumes: fp32 [K,D,H,W] on a GPU, every extent >= 2.  Returns a dict on the device: range (fp32 [K,nbz,nby,nbx,2]: the
    minimum and maximum over the brick's finite nodes; +inf, -inf when it has none) and nonfinite (uint8 [K,nbz,nby,nbx]:
    1 when a node of the brick is NaN or +-inf), nb = ceil((N - 1) / 8) per axis.  ops.raycast takes the dict as `bricks`
    and jumps over bricks that cannot contribute under its transfer function.  Never synchronises."""
    volumes, K, sp, P = _rc_volumes(volumes)
    nb = _rc_bricks(sp)
    dev = volumes.device
    res = {"range": torch.empty((K,) + nb + (2,), dtype=torch.float32, device=dev),
           "nonfinite": torch.empty((K,) + nb, dtype=torch.uint8, device=dev)}
    with torch.cuda.device(dev):
        _call("fs_brick_range3d", volumes.data_ptr(), K, *sp, volumes.stride(0) if K > 1 else P, res["range"].data_ptr(),
              res["nonfinite"].data_ptr(), _stream(volumes), algo_bytes=4 * K * P + 9 * K * nb[0] * nb[1] * nb[2])
    return res


def _rc_table(name, t, cols, dev):
    """A small fp32 table given as a tensor, an array or nested lists -> (contiguous fp32 tensor on dev, its fp32 copy
    in host memory or None when it already lived on a device)."""
    host = not (isinstance(t, torch.Tensor) and t.is_cuda)
    try:
        t = t if isinstance(t, torch.Tensor) else torch.tensor(t)  # (a copy: an array may be read-only)
    except Exception:
        raise ValueError("%s must be a tensor or an array of numbers" % name)
    if not t.dtype.is_floating_point and t.dtype not in (torch.int32, torch.int64):
        raise ValueError("%s must hold numbers, got %s" % (name, t.dtype))
    if t.dim() == 1 and cols == 18:
        t = t[None]
    if t.dim() != 2 or t.shape[1] != cols:
        raise ValueError("%s must be [n,%d], got %s" % (name, cols, tuple(t.shape)))
    t = t.detach().to(torch.float32).contiguous()
    return t.to(dev), t if host else None


def raycast(volumes, cameras, tf, lo, hi, dt=None, spacing=1.0, mode="dvr", t_min=0.0, bricks=None, counts=False,
            image=None):
    """K volumes through K cameras and one transfer function to K RGBA images, one launch (fs_raycast3d).

    volumes: fp32 [K,D,H,W] on a GPU; the step stride may be anything (stack[1::2] is read in place).  cameras: [K,18] (or
    one camera [18] for all K), the 3-vectors o, ou, ov, d, du, dv in (x, y, z): pixel (i, j) -- column i of row j -- has the
    origin o + i ou + j ov and the direction normalize(d + i du + j dv); render.orbit_camera makes them.  tf: [n,4] RGBA,
    2 <= n <= RC_MAX_TF, spread uniformly over the values [lo, hi]; finite with A >= 0 (checked when it comes from the
    host).  image: (rows, columns) of the pictures -- required.  spacing: the node spacing, one value or (D,H,W); node i of
    an axis sits at i * spacing.  dt: the sample distance, half the smallest spacing by default.

    A ray is sampled at (k + 1/2) dt from its origin, k = 0, 1, ...; a sample at index position q weighs
    c = prod_a max(0, 1 - max(0, -q_a, q_a - (N_a - 1))) (1 inside, fading to 0 one cell outside), reads the trilinear value
    v at q clamped to the box, and looks up the table at u = clamp((v - lo) / (hi - lo), 0, 1); a v that is not finite
    contributes nothing.  mode "dvr": sigma = A c, e = exp(-sigma dt), C += T (1 - e) RGB, T *= e; the pixel is (C, 1 - T)
    and the ray ends once T < t_min (0: never).  mode "mip": the pixel is the table's row at max_k c u.
    include/flowsci_hip.h states the order of operations; tests/raycast_ref.py restates it.

    bricks: ops.brick_ranges(volumes) -- rays jump over bricks in which the table's A is 0 (dvr) or nothing exceeds lo
    (mip); the image is the same bit for bit.  counts: also return the samples every pixel gathered.

    Returns a dict on the device: image (fp32 [K,Hi,Wi,4]) and, with counts, counts (int32 [K,Hi,Wi]).  Never
    synchronises.  Nothing is differentiated."""
    volumes, K, sp, P = _rc_volumes(volumes)
    dev = volumes.device
    if image is None:
        raise ValueError("image=(rows, columns) is required")
    Hi, Wi = _rc_image(image)
    if mode not in RC_MODES:
        raise ValueError("mode must be 'dvr' or 'mip', got %r" % (mode,))
    hs = _rc_spacing(spacing)
    try:
        lo, hi, t_min = float(lo), float(hi), float(t_min)
        dt = 0.5 * min(hs) if dt is None else float(dt)
    except (TypeError, ValueError):
        raise ValueError("lo, hi, dt and t_min must be numbers, got %r, %r, %r and %r" % (lo, hi, dt, t_min))
    inf = float("inf")
    if not (-inf < lo < hi < inf):
        raise ValueError("the table spans lo < hi, both finite; got %r and %r" % (lo, hi))
    if not (0 < dt < inf) or not (0 <= t_min < 1):
        raise ValueError("dt must be finite and positive and t_min in [0, 1), got %r and %r" % (dt, t_min))
    if sum((n + 1) * h for n, h in zip(sp, hs)) / dt > RC_MAX_STEPS:
        raise ValueError("dt = %r takes more than %d samples through the volume" % (dt, RC_MAX_STEPS))
    cams, _ = _rc_table("cameras", cameras, 18, dev)
    if cams.shape[0] == 1 and K > 1:
        cams = cams.expand(K, 18).contiguous()
    if cams.shape[0] != K:
        raise ValueError("cameras must be [%d,18] (or one camera), got %s" % (K, tuple(cams.shape)))
    table, cpu = _rc_table("tf", tf, 4, dev)
    if not 2 <= table.shape[0] <= RC_MAX_TF:
        raise ValueError("the transfer function has 2..%d rows, got %d" % (RC_MAX_TF, table.shape[0]))
    if cpu is not None:  # (a table that already lives on the device is not read back)
        if not bool(torch.isfinite(cpu).all() and (cpu[:, 3] >= 0).all()):
            raise ValueError("the transfer function must be finite with A >= 0")
    if table.data_ptr() % 16:
        table = table.clone()
    nb = _rc_bricks(sp)
    rng = flg = ws = None
    if bricks is not None:
        try:
            rng, flg = bricks["range"], bricks["nonfinite"]
        except (TypeError, KeyError, IndexError):
            raise ValueError("bricks must be what ops.brick_ranges returned")
        if (not isinstance(rng, torch.Tensor) or not isinstance(flg, torch.Tensor) or rng.device != dev or flg.device != dev
                or rng.dtype != torch.float32 or flg.dtype != torch.uint8 or tuple(rng.shape) != (K,) + nb + (2,)
                or tuple(flg.shape) != (K,) + nb):
            raise ValueError("bricks must be ops.brick_ranges of these volumes: range fp32 %s and nonfinite uint8 %s on %s" %
                             ((K,) + nb + (2,), (K,) + nb, dev))
        rng, flg = rng.contiguous(), flg.contiguous()
        n_ws = _lib.lib().fs_raycast3d_ws_bytes(K, *sp)
        if n_ws < 0:
            _lib.check(int(-n_ws), "fs_raycast3d_ws_bytes")
        ws = torch.empty(n_ws, dtype=torch.uint8, device=dev)
    res = {"image": torch.empty((K, Hi, Wi, 4), dtype=torch.float32, device=dev)}
    if counts:
        res["counts"] = torch.empty((K, Hi, Wi), dtype=torch.int32, device=dev)
    nbytes, flops = raycast_cost(sp, (Hi, Wi), K, dt, hs)
    with torch.cuda.device(dev):
        _call("fs_raycast3d", volumes.data_ptr(), K, *sp, volumes.stride(0) if K > 1 else P, cams.data_ptr(),
              table.data_ptr(), int(table.shape[0]), lo, hi, dt, (ctypes.c_double * 3)(*hs[::-1]), RC_MODES[mode], t_min,
              Hi, Wi, _ptr(rng), _ptr(flg), _ptr(ws), res["image"].data_ptr(), _ptr(res.get("counts")), _stream(volumes),
              algo_bytes=nbytes, algo_flops=flops)
    return res


# --------------------------------------------------------------------------------------------
# Isosurfaces: volumes to indexed triangle meshes by marching tetrahedra (fs_iso_count3d, fs_iso_emit3d)
# --------------------------------------------------------------------------------------------
ISO_MAX_VALUES = 8  # FS_ISO_MAX_VALUES


def isosurface_cost(shape, K=1, V=0, T=0, F=0, normals=True, op="count"):
    """(HBM bytes, flops) the algorithm needs for one pass of ops.isosurface over K volumes of spatial `shape`.  "count":
    every node read once (4 bytes), its mask byte written, two int32 per row.  "emit": the mask bytes read, the V vertices
    (12 bytes, 12 more with normals, 4 F with values) and the T faces (12 bytes) written; the nodes, gradients and value
    planes gathered around cut cells are on top and depend on the surface.  The work is integer work: flops 0."""
    sp = tuple(int(s) for s in shape)
    if len(sp) != 3 or min(sp) < 2:
        raise ValueError("shape must be (D,H,W) with every extent >= 2, got %r" % (shape,))
    K, V, T, F = int(K), int(V), int(T), int(F)
    if K < 1 or V < 0 or T < 0 or not 0 <= F <= ISO_MAX_VALUES:
        raise ValueError("K >= 1, V, T >= 0 and F in 0..%d, got %d, %d, %d, %d" % (ISO_MAX_VALUES, K, V, T, F))
    P = sp[0] * sp[1] * sp[2]
    if op == "count":
        return K * (5 * P + 8 * sp[0] * sp[1]), 0
    if op == "emit":
        return K * P + V * (12 + (12 if normals else 0) + 4 * F) + 12 * T, 0
    raise ValueError("op must be 'count' or 'emit', got %r" % (op,))


def isosurface_count(volumes, iso):
    """The first pass of ops.isosurface on its own (fs_iso_count3d): the workspace (uint8, the per-row counts and the
    per-node masks of active edges) and row_offsets, int64 [2, K*D*H + 1] on the device: the exclusive prefix sums of the
    rows' vertex and triangle counts (plumbing: torch.cumsum).  Never synchronises."""
    volumes, K, sp, P = _rc_volumes(volumes)
    try:
        iso = float(iso)
    except (TypeError, ValueError):
        raise ValueError("iso must be a number, got %r" % (iso,))
    if not -float("inf") < iso < float("inf"):
        raise ValueError("iso must be finite, got %r" % (iso,))
    dev = volumes.device
    R = K * sp[0] * sp[1]
    nb = _lib.lib().fs_iso3d_ws_bytes(K, *sp)
    if nb < 0:
        _lib.check(int(-nb), "fs_iso3d_ws_bytes")
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    nbytes, flops = isosurface_cost(sp, K, op="count")
    with torch.cuda.device(dev):
        _call("fs_iso_count3d", volumes.data_ptr(), K, *sp, volumes.stride(0) if K > 1 else P, iso, ws.data_ptr(),
              _stream(volumes), algo_bytes=nbytes, algo_flops=flops)
    off = torch.zeros((2, R + 1), dtype=torch.int64, device=dev)
    off[:, 1:] = torch.cumsum(ws[:8 * R].view(torch.int32).view(2, R), 1, dtype=torch.int64)
    return ws, off


def isosurface_emit(volumes, iso, spacing, ws, row_offsets, V, T, normals=True, values=None):
    """The second pass of ops.isosurface on its own (fs_iso_emit3d), on what isosurface_count returned and the totals V
    and T as host ints.  Returns (vertices, normals or None, values or None, faces, status) on the device.  Never
    synchronises."""
    volumes, K, sp, P = _rc_volumes(volumes)
    hs = _rc_spacing(spacing)
    dev = volumes.device
    V, T = int(V), int(T)
    F = 0 if values is None else int(values.shape[1])
    vert = torch.empty((V, 3), dtype=torch.float32, device=dev)
    nrm = torch.empty((V, 3), dtype=torch.float32, device=dev) if normals else None
    vout = torch.empty((V, F), dtype=torch.float32, device=dev) if F else None
    faces = torch.empty((T, 3), dtype=torch.int32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    if V or T:
        nbytes, flops = isosurface_cost(sp, K, V, T, F, normals, op="emit")
        with torch.cuda.device(dev):
            _call("fs_iso_emit3d", volumes.data_ptr(), K, *sp, volumes.stride(0) if K > 1 else P, float(iso),
                  (ctypes.c_double * 3)(*hs[::-1]), ws.data_ptr(), row_offsets.data_ptr(), V, T, _ptr(values), F,
                  vert.data_ptr(), _ptr(nrm), _ptr(vout), faces.data_ptr(), status.data_ptr(), _stream(volumes),
                  algo_bytes=nbytes, algo_flops=flops)
    return vert, nrm, vout, faces, status


def isosurface(volumes, iso, spacing=1.0, normals=True, values=None):
    """K volumes and one isovalue to K indexed triangle meshes, two launches (fs_iso_count3d, fs_iso_emit3d): marching
    tetrahedra on the Kuhn split of every cell -- watertight and consistently oriented by construction.

    volumes: fp32 [K,D,H,W] on a GPU, every extent >= 2; the step stride may be anything (stack[::2] is read in place).
    A finite node is inside iff f >= fp32(iso); a cell with a corner that is not finite emits nothing.  spacing: the node
    spacing, one value or (D,H,W); node i of an axis sits at i * spacing.  values: optional fp32 [K,F,D,H,W] on the same
    device, F <= 8, interpolated to the vertices.  include/flowsci_hip.h states the definition; tests/isosurface_ref.py
    restates it.

    The numbers of vertices and faces depend on the data, so this SYNCHRONISES: exactly once, between the two launches, to
    learn the steps' offsets (the prefix sum over the rows' counts is torch's).  `status` is therefore returned, not read:
    ops.isosurface_check(result) reads it and raises FlowsciKernelError when it is set (isosurface.isosurface_series does
    so with the download it makes anyway).  ValueError when a step has 2^31 - 1 or more vertices or faces.

    Returns a dict on the device: vertices (fp32 [V,3], (x, y, z), a step's in the order of owner node, then edge), normals
    (fp32 [V,3], unit, towards lower values, from the interpolated central-difference gradient; only with normals), values
    (fp32 [V,F]; only with values), faces (int32 [T,3], indices local to their step, by cell, tetrahedron, triangle),
    vertex_offsets and face_offsets (int64 [K+1]: step k owns rows offsets[k] .. offsets[k+1]) and status (int32 [1]).
    Bitwise reproducible.  Nothing is differentiated."""
    volumes, K, sp, P = _rc_volumes(volumes)
    dev = volumes.device
    _rc_spacing(spacing)
    if values is not None:
        values = _need_cuda_f32("values", values, 5)
        F = int(values.shape[1])
        if tuple(values.shape) != (K, F) + sp or not 1 <= F <= ISO_MAX_VALUES or values.device != dev:
            raise ValueError("values must be [K,F,D,H,W] = [%d, 1..%d, %s] on %s, got %s on %s" %
                             (K, ISO_MAX_VALUES, sp, dev, tuple(values.shape), values.device))
    ws, off = isosurface_count(volumes, iso)
    steps = off[:, ::sp[0] * sp[1]].contiguous()  # [2, K+1]
    host = steps.cpu().numpy()  # the one synchronisation
    per_step = _np.diff(host, axis=1)
    if per_step.size and int(per_step.max()) >= 2 ** 31 - 1:
        raise ValueError("a step has %d vertices or faces: the limit is 2^31 - 2" % int(per_step.max()))
    V, T = int(host[0, -1]), int(host[1, -1])
    vert, nrm, vout, faces, status = isosurface_emit(volumes, iso, spacing, ws, off, V, T, normals, values)
    res = {"vertices": vert, "faces": faces, "vertex_offsets": steps[0], "face_offsets": steps[1], "status": status}
    if normals:
        res["normals"] = nrm
    if values is not None:
        res["values"] = vout
    return res


def isosurface_check(result):
    """Raises FlowsciKernelError when ops.isosurface's `status` is set (the masks and offsets of its two passes
    disagreed: the arrays are then not a mesh).  Synchronises."""
    st = int(result["status"].view(-1)[0]) if isinstance(result["status"], torch.Tensor) else int(result["status"])
    if st != 0:
        raise _lib.FlowsciKernelError("fs_iso_emit3d: the masks and the row offsets disagree (status %d)" % st)


# --------------------------------------------------------------------------------------------
# Critical points: where step flows vanish, and what kind of zero each is (fs_critical_count{2,3}d, fs_critical_emit{2,3}d)
# --------------------------------------------------------------------------------------------
CP_NPOS_MASK, CP_SPIRAL, CP_DEGENERATE, CP_MARGINAL = 3, 4, 8, 16  # FS_CP_*: the bits of `cls`
CP_MASK_DEGENERATE, CP_MASK_NONFINITE = 64, 128                    # FS_CP_MASK_*: of a cell's mask byte (bit t: simplex t)
_CP_BASE = {2: ("sink", "saddle", "source"), 3: ("sink", "saddle1", "saddle2", "source")}


def critical_class_names(cls, nd):
    """The report name of every class byte in `cls` (a tensor, an array or a sequence) in nd dimensions: by n_pos, the
    eigenvalues with a positive real part -- sink (0), saddle (2-D: 1), saddle1 / saddle2 (3-D: 1 / 2), source (nd) --
    with the prefix "focus_" (2-D) / "spiral_" (3-D) when CP_SPIRAL is set; "degenerate" when CP_DEGENERATE is set, and
    in 2-D "center" when CP_MARGINAL is (a purely rotating zero)."""
    if nd not in (2, 3):
        raise ValueError("nd must be 2 or 3, got %r" % (nd,))
    vals = cls.reshape(-1).tolist() if hasattr(cls, "reshape") else list(cls)
    names = []
    for c in vals:
        c = int(c)
        if c & CP_DEGENERATE:
            names.append("degenerate")
        elif nd == 2 and c & CP_MARGINAL:
            names.append("center")
        else:
            n = c & CP_NPOS_MASK
            if n > nd:
                raise ValueError("class %d has n_pos = %d in %d dimensions" % (c, n, nd))
            names.append((("focus_" if nd == 2 else "spiral_") if c & CP_SPIRAL else "") + _CP_BASE[nd][n])
    return names


def critical_class_list(nd):
    """Every name critical_class_names can give in nd dimensions, in report order."""
    pre = "focus_" if nd == 2 else "spiral_"
    names = list(_CP_BASE[nd]) + [pre + n for n in _CP_BASE[nd] if nd == 3 or n != "saddle"]
    return names + (["center"] if nd == 2 else []) + ["degenerate"]


def critical_points_cost(shape, K=1, N=0, op="count"):
    """(HBM bytes, flops) the algorithm needs for one pass of ops.critical_points over K step flows of spatial `shape`
    ((H,W) or (D,H,W)).  "count": every node's C components read once (4 C bytes), its mask byte written, two int32 per
    row.  "emit": the mask bytes read and the N rows written (4 cell + 1 simplex + 4 C pos + 8 C^2 jac + 32 inv + 1 cls +
    4 vmax); the corners gathered around flagged cells are on top and depend on the field.  The streaming work is
    compares and integer work: flops count the fp64 minors and invariants of the N points only (~100 C per point)."""
    sp, P = _lattice(shape)
    C = len(sp)
    K, N = int(K), int(N)
    if K < 1 or N < 0:
        raise ValueError("K >= 1 and N >= 0, got %d, %d" % (K, N))
    rows = P // sp[-1]
    if op == "count":
        return K * (P * (4 * C + 1) + 8 * rows), 0
    if op == "emit":
        return K * P + N * (4 + 1 + 4 * C + 8 * C * C + 32 + 1 + 4), N * 100 * C
    raise ValueError("op must be 'count' or 'emit', got %r" % (op,))


def _cp_vmin(vmin):
    try:
        vmin = float(vmin)
    except (TypeError, ValueError):
        raise ValueError("vmin must be a number, got %r" % (vmin,))
    if not 0 <= vmin < float("inf"):
        raise ValueError("vmin must be finite and >= 0, got %r" % (vmin,))
    return vmin


def _cp_spacing_scale(spacing, scale, nd, K):
    try:
        hs = [float(v) for v in spacing] if hasattr(spacing, "__len__") else [float(spacing)] * nd
        ss = [float(v) for v in scale] if hasattr(scale, "__len__") else [float(scale)] * K
    except TypeError:
        raise ValueError("spacing and scale must be numbers or sequences of numbers, got %r and %r" % (spacing, scale))
    if len(hs) != nd or not all(0 < h < float("inf") for h in hs):
        raise ValueError("spacing must be one or %d finite positive values, got %r" % (nd, spacing))
    if len(ss) != K or not all(0 < v < float("inf") for v in ss):
        raise ValueError("scale must be one or %d finite positive values, got %r" % (K, scale))
    return hs, ss


def critical_points_count(flows, vmin=0.0):
    """The first pass of ops.critical_points on its own (fs_critical_count{2,3}d): the workspace (uint8: the per-row
    counts of points and of degenerate simplices, then one mask byte per node) and row_offsets, int64 [K*D*H + 1] on the
    device: the exclusive prefix sum of the rows' point counts (plumbing: torch.cumsum).  Never synchronises."""
    vmin = _cp_vmin(vmin)
    flows, nd = _advect_flows(flows)
    sp, P = _lattice(flows.shape[2:])
    K = int(flows.shape[0])
    dev = flows.device
    R = K * (P // sp[-1])
    nb = getattr(_lib.lib(), "fs_critical%dd_ws_bytes" % nd)(K, *sp)
    if nb < 0:
        _lib.check(int(-nb), "fs_critical%dd_ws_bytes" % nd)
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    nbytes, flops = critical_points_cost(sp, K, op="count")
    with torch.cuda.device(dev):
        _call("fs_critical_count%dd" % nd, flows.data_ptr(), K, nd, *sp, flows.stride(0) if K > 1 else nd * P, vmin,
              ws.data_ptr(), _stream(flows), algo_bytes=nbytes, algo_flops=flops)
    off = torch.zeros(R + 1, dtype=torch.int64, device=dev)
    off[1:] = torch.cumsum(ws[:4 * R].view(torch.int32), 0, dtype=torch.int64)
    return ws, off


def critical_points_emit(flows, spacing, scale, vmin, ws, row_offsets, N):
    """The second pass of ops.critical_points on its own (fs_critical_emit{2,3}d), on what critical_points_count returned
    and the total N as a host int.  Returns a dict on the device: cell, simplex, pos, jac, inv, cls, vmax, status.
    Never synchronises; launches nothing when N is 0."""
    vmin = _cp_vmin(vmin)
    flows, nd = _advect_flows(flows)
    sp, P = _lattice(flows.shape[2:])
    K = int(flows.shape[0])
    hs, ss = _cp_spacing_scale(spacing, scale, nd, K)
    dev = flows.device
    N = int(N)
    if N < 0:
        raise ValueError("N must be >= 0, got %d" % N)
    res = {"cell": torch.empty(N, dtype=torch.int32, device=dev), "simplex": torch.empty(N, dtype=torch.uint8, device=dev),
           "pos": torch.empty((N, nd), dtype=torch.float32, device=dev),
           "jac": torch.empty((N, nd * nd), dtype=torch.float64, device=dev),
           "inv": torch.empty((N, 4), dtype=torch.float64, device=dev), "cls": torch.empty(N, dtype=torch.uint8, device=dev),
           "vmax": torch.empty(N, dtype=torch.float32, device=dev), "status": torch.zeros(1, dtype=torch.int32, device=dev)}
    if N:
        nbytes, flops = critical_points_cost(sp, K, N, op="emit")
        # component 0 and axis 0 run along x: the tensor's last axis
        inv_h = (ctypes.c_double * nd)(*[1.0 / h for h in hs[::-1]])
        with torch.cuda.device(dev):
            _call("fs_critical_emit%dd" % nd, flows.data_ptr(), K, nd, *sp, flows.stride(0) if K > 1 else nd * P, inv_h,
                  (ctypes.c_double * K)(*ss), vmin, ws.data_ptr(), row_offsets.data_ptr(), N, res["cell"].data_ptr(),
                  res["simplex"].data_ptr(), res["pos"].data_ptr(), res["jac"].data_ptr(), res["inv"].data_ptr(),
                  res["cls"].data_ptr(), res["vmax"].data_ptr(), res["status"].data_ptr(), _stream(flows),
                  algo_bytes=nbytes, algo_flops=flops)
    return res


def critical_points(flows, spacing=1.0, scale=1.0, vmin=0.0):
    """The critical points of K step flows -- where the field vanishes -- with their kind, two launches
    (fs_critical_count{2,3}d, fs_critical_emit{2,3}d).

    flows: [K,2,H,W] or [K,3,D,H,W] fp32 displacements on a GPU, in elements, channel 0 along W, every extent >= 2; the
    step stride may be anything (stack[::2] is read in place).  spacing: the node spacing, one value or one per axis in
    the tensor's axis order ((D,)H,W).  scale: the reciprocal of the time a step spans, one value or K: velocity =
    displacement * scale.  vmin: a simplex whose corners all move at most this fast (in elements per step, before
    `scale`) is quiet and holds no point.

    Every cell is cut into its Kuhn simplices (3-D: the six tetrahedra of ops.isosurface; 2-D: two triangles) and the
    field taken as affine on each: a simplex holds a point when the signed face minors of its corner values all have one
    sign, and the point's class follows from the invariants of the affine piece's Jacobian (Routh-Hurwitz: no
    eigenvalue is computed).  A simplex with a minor that is exactly 0 is reported as degenerate, not resolved.
    include/flowsci_hip.h states the order of operations; tests/critical_ref.py restates it and agrees bit for bit.

    The number of points depends on the data, so this SYNCHRONISES: exactly once, between the two launches, to learn the
    steps' offsets (the prefix sum over the rows' counts is torch's).  `status` is therefore returned, not read:
    ops.critical_points_check(result) reads it.  ValueError when a step has 2^31 - 1 or more points.

    Returns a dict on the device: cell (int32 [N]: the node index of the cell's origin within its step), simplex (uint8
    [N]: t), pos (fp32 [N,C]: (x, y(, z)) in physical units), jac (fp64 [N,C*C]: d u_r / d x_c at r * C + c), inv (fp64
    [N,4]: 3-D P, Q, R, Delta of the characteristic polynomial; 2-D tr, det, disc, 0), cls (uint8 [N]: n_pos in bits
    0-1, CP_SPIRAL, CP_DEGENERATE, CP_MARGINAL; critical_class_names names it), vmax (fp32 [N]: the largest corner speed
    of the simplex), offsets (int64 [K+1]: step k owns the rows offsets[k] .. offsets[k+1], ordered by cell, then t),
    counts (int64 [K,4]: points, degenerate simplices, cells with a corner that is not finite, cells with a point) and
    status (int32 [1]).  Bitwise reproducible.  Nothing is differentiated."""
    vmin = _cp_vmin(vmin)
    flows, nd = _advect_flows(flows)
    sp, P = _lattice(flows.shape[2:])
    K = int(flows.shape[0])
    _cp_spacing_scale(spacing, scale, nd, K)
    ws, off = critical_points_count(flows, vmin)
    rows = P // sp[-1]
    R = K * rows
    steps = off[::rows].contiguous()  # [K+1]
    host = steps.cpu().numpy()  # the one synchronisation
    per_step = _np.diff(host)
    if per_step.size and int(per_step.max()) >= 2 ** 31 - 1:
        raise ValueError("a step has %d critical points: the limit is 2^31 - 2" % int(per_step.max()))
    res = critical_points_emit(flows, spacing, scale, vmin, ws, off, int(host[-1]))
    mask = ws[ws.numel() - K * P:].view(K, P)
    res["offsets"] = steps
    res["counts"] = torch.stack([steps[1:] - steps[:-1],
                                 ws[4 * R:8 * R].view(torch.int32).view(K, rows).sum(1, dtype=torch.int64),
                                 (mask & CP_MASK_NONFINITE).ne(0).sum(1), (mask & 63).ne(0).sum(1)], 1)
    return res


def critical_points_check(result):
    """Raises FlowsciKernelError when ops.critical_points' `status` is set (the masks and offsets of its two passes
    disagreed: the arrays are then not a table).  Synchronises."""
    st = int(result["status"].view(-1)[0]) if isinstance(result["status"], torch.Tensor) else int(result["status"])
    if st != 0:
        raise _lib.FlowsciKernelError("fs_critical_emit: the masks and the row offsets disagree (status %d)" % st)


# --------------------------------------------------------------------------------------------
# Parallel vectors: the segments of the locus v || w -- vortex core lines (fs_pv_count3d, fs_pv_emit3d)
# --------------------------------------------------------------------------------------------
PV_MASK_AMBIGUOUS, PV_MASK_NONFINITE, PV_NODE_NONFINITE = 64, 128, 1 << 24  # FS_PV_*
PV_COLUMNS = ("cell", "simplex", "face", "key", "pos", "mu", "vel")          # and "aux" when one is carried along


def parallel_vectors_cost(shape, K=1, N=0, op="count", aux=False):
    """(HBM bytes, flops) the algorithm needs for one pass of ops.parallel_vectors over K steps of spatial `shape`
    (D,H,W).  "count": the 6 (7 with aux) values of every node read once, its face word written and read (4 + 4), its
    mask byte written, four int32 per row; ~1100 fp64 flops of screening per node (12 faces: 18 cross-product
    coefficients each).  "emit": the mask bytes read and the N rows written (4 cell + 1 simplex + 2 face + 16 key + 24 pos
    + 16 mu + 24 vel (+ 8 aux)); flops: ~2000 per re-solved endpoint.  The solves of surviving faces depend on the field
    and are on top."""
    sp, P = _lattice(shape)
    K, N = int(K), int(N)
    if len(sp) != 3 or K < 1 or N < 0:
        raise ValueError("a (D,H,W) shape, K >= 1 and N >= 0, got %r, %d, %d" % (shape, K, N))
    rows = P // sp[-1]
    if op == "count":
        return K * (P * (4 * (7 if aux else 6) + 8 + 1) + 16 * rows), K * P * 1100
    if op == "emit":
        return K * P + N * (87 + (8 if aux else 0)), N * 4000
    raise ValueError("op must be 'count' or 'emit', got %r" % (op,))


def _pv_operands(v, w, aux):
    v, nd = _advect_flows(v)
    if nd != 3:
        raise ValueError("parallel vectors are 3-D only ([K,3,D,H,W]), got shape %s" % (tuple(v.shape),))
    if not isinstance(w, torch.Tensor) or tuple(w.shape) != tuple(v.shape) or w.device != v.device:
        raise ValueError("w must be a tensor of v's shape %s on v's device" % (tuple(v.shape),))
    w = _flow_operand("w", w.detach(), 3)
    K = int(v.shape[0])
    if aux is not None:
        if not isinstance(aux, torch.Tensor) or tuple(aux.shape) != (K,) + tuple(v.shape[2:]) or aux.device != v.device:
            raise ValueError("aux must be a tensor [K,D,H,W] = %s on v's device" % ((K,) + tuple(v.shape[2:]),))
        aux = aux.detach().to(torch.float32)
        if not aux[0].is_contiguous() or (K > 1 and aux.stride(0) < aux[0].numel()):
            aux = aux.contiguous()
    return v, w, aux


def _pv_field_args(v, w, aux, K, P):
    return (v.data_ptr(), v.stride(0) if K > 1 else 3 * P, w.data_ptr(), w.stride(0) if K > 1 else 3 * P, _ptr(aux),
            (aux.stride(0) if K > 1 else P) if aux is not None else 0)


def _pv_min(name, m):
    try:
        m = float(m)
    except (TypeError, ValueError):
        raise ValueError("%s must be a number, got %r" % (name, m))
    if not 0 <= m < float("inf"):
        raise ValueError("%s must be finite and >= 0, got %r" % (name, m))
    return m


def parallel_vectors_count(v, w, aux=None, vmin=0.0, wmin=0.0):
    """The first pass of ops.parallel_vectors on its own (fs_pv_count3d): the workspace (uint8: four int32 counts per
    row, one uint32 of face counts per node, one mask byte per node) and row_offsets, int64 [K*D*H + 1] on the device:
    the exclusive prefix sum of the rows' segment counts (plumbing: torch.cumsum).  Never synchronises."""
    vmin, wmin = _pv_min("vmin", vmin), _pv_min("wmin", wmin)
    v, w, aux = _pv_operands(v, w, aux)
    sp, P = _lattice(v.shape[2:])
    K = int(v.shape[0])
    dev = v.device
    R = K * (P // sp[-1])
    nb = _lib.lib().fs_pv3d_ws_bytes(K, *sp)
    if nb < 0:
        _lib.check(int(-nb), "fs_pv3d_ws_bytes")
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    nbytes, flops = parallel_vectors_cost(sp, K, op="count", aux=aux is not None)
    with torch.cuda.device(dev):
        _call("fs_pv_count3d", *_pv_field_args(v, w, aux, K, P), K, *sp, vmin, wmin, ws.data_ptr(), _stream(v),
              algo_bytes=nbytes, algo_flops=flops)
    off = torch.zeros(R + 1, dtype=torch.int64, device=dev)
    off[1:] = torch.cumsum(ws[:4 * R].view(torch.int32), 0, dtype=torch.int64)
    return ws, off


def parallel_vectors_emit(v, w, aux, spacing, vmin, wmin, ws, row_offsets, N):
    """The second pass of ops.parallel_vectors on its own (fs_pv_emit3d), on what parallel_vectors_count returned and
    the total N as a host int.  Returns a dict on the device: cell, simplex, face, key, pos, mu, vel, (aux,) status.
    Never synchronises; launches nothing when N is 0."""
    vmin, wmin = _pv_min("vmin", vmin), _pv_min("wmin", wmin)
    v, w, aux = _pv_operands(v, w, aux)
    sp, P = _lattice(v.shape[2:])
    K = int(v.shape[0])
    hs, _ = _cp_spacing_scale(spacing, 1.0, 3, K)
    dev = v.device
    N = int(N)
    if N < 0:
        raise ValueError("N must be >= 0, got %d" % N)
    res = {"cell": torch.empty(N, dtype=torch.int32, device=dev), "simplex": torch.empty(N, dtype=torch.uint8, device=dev),
           "face": torch.empty((N, 2), dtype=torch.uint8, device=dev), "key": torch.empty((N, 2), dtype=torch.int64, device=dev),
           "pos": torch.empty((N, 2, 3), dtype=torch.float32, device=dev),
           "mu": torch.empty((N, 2), dtype=torch.float64, device=dev),
           "vel": torch.empty((N, 2, 3), dtype=torch.float32, device=dev)}
    if aux is not None:
        res["aux"] = torch.empty((N, 2), dtype=torch.float32, device=dev)
    res["status"] = torch.zeros(1, dtype=torch.int32, device=dev)
    if N:
        nbytes, flops = parallel_vectors_cost(sp, K, N, op="emit", aux=aux is not None)
        # component 0 and axis 0 run along x: the tensor's last axis
        inv_h = (ctypes.c_double * 3)(*[1.0 / h for h in hs[::-1]])
        with torch.cuda.device(dev):
            _call("fs_pv_emit3d", *_pv_field_args(v, w, aux, K, P), K, *sp, inv_h, vmin, wmin, ws.data_ptr(),
                  row_offsets.data_ptr(), N, res["cell"].data_ptr(), res["simplex"].data_ptr(), res["face"].data_ptr(),
                  res["key"].data_ptr(), res["pos"].data_ptr(), res["mu"].data_ptr(), res["vel"].data_ptr(),
                  _ptr(res.get("aux")), res["status"].data_ptr(), _stream(v), algo_bytes=nbytes, algo_flops=flops)
    return res


def parallel_vectors(v, w, aux=None, spacing=1.0, vmin=0.0, wmin=0.0):
    """The parallel-vectors operator of Peikert and Roth: the locus where the fields v and w of K steps are parallel, as
    line segments (fs_pv_count3d, fs_pv_emit3d).  With w = J v these are the vortex core lines of Sujudi and Haimes,
    with w = curl v those of Levy et al. (cores.core_fields forms both).  3-D only: in 2-D the locus is a curve.

    v, w: [K,3,D,H,W] fp32 on a GPU, channel 0 along W, every extent >= 2; the step stride may be anything (stack[::2]
    is read in place).  aux: optional [K,D,H,W] fp32, a scalar interpolated to every point (Q, lambda2: what segments
    are filtered by).  spacing: the node spacing, one value or one per axis in the tensor's axis order (D,H,W).  vmin,
    wmin: a node with |v| <= vmin or |w| <= wmin is quiet, and a face whose three corners are quiet holds nothing.

    Every cell is cut into its six Kuhn tetrahedra and both fields taken as linear on each triangular face: the points
    of a face where v || w are the real eigenvalues of a 3 x 3 pencil with an eigenvector inside the triangle.  A
    tetrahedron with exactly two such points holds one segment; one with any other number but 0 is counted as
    ambiguous and emits nothing, as is a face whose pencil is singular (degenerate).  A face is solved once, by the node
    that owns it, so the two tetrahedra that share it agree bit for bit: segments that meet carry equal `key`s, and
    cores.link_segments joins them into lines by key alone.  include/flowsci_hip.h states the order of operations;
    tests/pv_ref.py restates it and agrees bit for bit.

    The number of segments depends on the data, so this SYNCHRONISES: exactly once, between the two passes.  `status`
    is returned, not read: ops.parallel_vectors_check(result) reads it.

    Returns a dict on the device: cell (int32 [N]: the cell's node index within its step), simplex (uint8 [N]: t), face
    (uint8 [N,2]: the face of t each endpoint lies on), key (int64 [N,2]: 4 * global face id + root rank), pos (fp32
    [N,2,3]: (x, y, z) in physical units), mu (fp64 [N,2]: w = mu * v at the point), vel (fp32 [N,2,3]: v at the point),
    aux (fp32 [N,2], only when given), offsets (int64 [K+1]: step k owns the rows offsets[k] .. offsets[k+1], ordered by
    cell, then t), counts (int64 [K,4]: segments, ambiguous tetrahedra, degenerate faces, cells with a value that is not
    finite) and status (int32 [1]).  Bitwise reproducible.  Nothing is differentiated."""
    vmin, wmin = _pv_min("vmin", vmin), _pv_min("wmin", wmin)
    v, w, aux = _pv_operands(v, w, aux)
    sp, P = _lattice(v.shape[2:])
    K = int(v.shape[0])
    _cp_spacing_scale(spacing, 1.0, 3, K)
    ws, off = parallel_vectors_count(v, w, aux, vmin, wmin)
    rows = P // sp[-1]
    R = K * rows
    steps = off[::rows].contiguous()  # [K+1]
    host = steps.cpu().numpy()  # the one synchronisation
    res = parallel_vectors_emit(v, w, aux, spacing, vmin, wmin, ws, off, int(host[-1]))
    per_row = ws[4 * R:16 * R].view(torch.int32).view(3, K, rows).sum(2, dtype=torch.int64)  # namb, ndeg, nnf
    res["offsets"] = steps
    res["counts"] = torch.cat([(steps[1:] - steps[:-1])[None], per_row], 0).t().contiguous()
    return res


def parallel_vectors_check(result):
    """Raises FlowsciKernelError when ops.parallel_vectors' `status` is set (its two passes disagreed: the arrays are
    then not a table).  Synchronises."""
    st = int(result["status"].view(-1)[0]) if isinstance(result["status"], torch.Tensor) else int(result["status"])
    if st != 0:
        raise _lib.FlowsciKernelError("fs_pv_emit3d: the two passes disagree (status %d)" % st)


# --------------------------------------------------------------------------------------------
# Ridge surfaces: the height ridges (of an FTLE field: the LCS) and valleys of scalar volumes as triangle meshes
# (fs_ridge_nodes3d, fs_ridge_count3d, fs_ridge_emit3d)
# --------------------------------------------------------------------------------------------
RIDGE_BORDER, RIDGE_NONFINITE, RIDGE_WEAK, RIDGE_LOW, RIDGE_ELIGIBLE = 0, 1, 2, 3, 4  # FS_RIDGE_*: a node's class
RIDGE_CLASS_NAMES = ("border", "nonfinite", "weak", "low", "eligible")
RIDGE_SWEEPS = 4  # FS_RIDGE_SWEEPS


def ridge_cost(shape, K=1, V=0, T=0, op="nodes", values=True):
    """(HBM bytes, flops) the algorithm needs for one pass of ops.ridge_surfaces over K volumes of spatial `shape`.
    "nodes": every node read once (4 bytes; its 18 neighbours come out of the caches), five fp32 operands and a class
    byte written; ~600 fp64 flops per interior node (19-point differences, 4 sweeps of 3 rotations of ~45 flops, 15 of
    them divisions and square roots counted as one).  "count": four operands and the class of every node read (17
    bytes), its mask byte written, four int32 per row; 19 fp64 dot products per eligible cell.  "emit": the mask bytes
    read, the V vertices (12 bytes, 8 more with values) and T faces (12 bytes) written; the operands gathered around
    cut cells are on top and depend on the surface."""
    sp = tuple(int(s) for s in shape)
    if len(sp) != 3 or min(sp) < 2:
        raise ValueError("shape must be (D,H,W) with every extent >= 2, got %r" % (shape,))
    K, V, T = int(K), int(V), int(T)
    if K < 1 or V < 0 or T < 0:
        raise ValueError("K >= 1 and V, T >= 0, got %d, %d, %d" % (K, V, T))
    P = sp[0] * sp[1] * sp[2]
    if op == "nodes":
        return K * 25 * P, K * 600 * max(sp[0] - 2, 0) * max(sp[1] - 2, 0) * max(sp[2] - 2, 0)
    if op == "count":
        return K * (18 * P + 16 * sp[0] * sp[1]), K * 95 * P
    if op == "emit":
        return K * P + V * (12 + (8 if values else 0)) + 12 * T, 0
    raise ValueError("op must be 'nodes', 'count' or 'emit', got %r" % (op,))


def _ridge_filters(strength, fmin):
    try:
        strength, fmin = float(strength), float(fmin)
    except (TypeError, ValueError):
        raise ValueError("strength and fmin must be numbers, got %r and %r" % (strength, fmin))
    if not 0 <= strength < float("inf"):
        raise ValueError("strength must be finite and >= 0, got %r" % (strength,))
    if not fmin < float("inf"):
        raise ValueError("fmin must be a number below +inf (-inf: no filter), got %r" % (fmin,))
    return strength, fmin


def _ridge_operands(operands, cls):
    if not (isinstance(operands, torch.Tensor) and isinstance(cls, torch.Tensor) and operands.is_cuda and
            operands.dtype == torch.float32 and cls.dtype == torch.uint8 and operands.dim() == 5 and cls.dim() == 4 and
            operands.shape[1] == 5 and tuple(operands.shape[2:]) == tuple(cls.shape[1:]) and
            operands.shape[0] == cls.shape[0] and cls.device == operands.device):
        raise ValueError("operands must be float32 [K,5,D,H,W] and cls uint8 [K,D,H,W] on one GPU, as ops.ridge_nodes "
                         "returns them")
    K = int(cls.shape[0])
    sp = tuple(int(s) for s in cls.shape[1:])
    if K < 1 or min(sp) < 2:
        raise ValueError("every extent must be >= 2, got %s" % (tuple(cls.shape),))
    return operands.detach().contiguous(), cls.detach().contiguous(), K, sp, sp[0] * sp[1] * sp[2]


def ridge_nodes(volumes, spacing=1.0, strength=0.0, fmin=-float("inf"), valley=False):
    """The node pass of ops.ridge_surfaces on its own (fs_ridge_nodes3d, one launch): per node of fp32 volumes [K,D,H,W]
    the gradient and Hessian by central differences and the Hessian's smallest eigenvalue lam with its eigenvector e, in
    fp64.  Returns (operands fp32 [K,5,D,H,W] = e_x, e_y, e_z, d = e . grad f, lam -- NaN where the node is not eligible
    -- and cls uint8 [K,D,H,W], RIDGE_*: border, a stencil value that is not finite, weak (!(lam <= -strength)), low
    (!(f >= fmin)), eligible).  valley: the same of -f.  Never synchronises."""
    volumes, K, sp, P = _rc_volumes(volumes)
    hs = _rc_spacing(spacing)[::-1]  # along x, y, z
    strength, fmin = _ridge_filters(strength, fmin)
    dev = volumes.device
    operands = torch.empty((K, 5) + sp, dtype=torch.float32, device=dev)
    cls = torch.empty((K,) + sp, dtype=torch.uint8, device=dev)
    inv_2h = (ctypes.c_double * 3)(*[1.0 / (2.0 * h) for h in hs])
    inv_hh = (ctypes.c_double * 3)(*[1.0 / (h * h) for h in hs])
    inv_4hh = (ctypes.c_double * 3)(1.0 / (4.0 * hs[0] * hs[1]), 1.0 / (4.0 * hs[0] * hs[2]), 1.0 / (4.0 * hs[1] * hs[2]))
    nbytes, flops = ridge_cost(sp, K, op="nodes")
    with torch.cuda.device(dev):
        _call("fs_ridge_nodes3d", volumes.data_ptr(), K, *sp, volumes.stride(0) if K > 1 else P, 1 if valley else 0,
              inv_2h, inv_hh, inv_4hh, strength, fmin, operands.data_ptr(), cls.data_ptr(), _stream(volumes),
              algo_bytes=nbytes, algo_flops=flops)
    return operands, cls


def ridge_count(operands, cls):
    """The first marching pass on its own (fs_ridge_count3d) on what ops.ridge_nodes returned: the workspace (uint8: per
    row its vertices, triangles, twisted and all-eligible tetrahedra as int32, then the per-node masks of active edges)
    and row_offsets, int64 [2, K*D*H + 1] on the device (plumbing: torch.cumsum).  Never synchronises."""
    operands, cls, K, sp, P = _ridge_operands(operands, cls)
    dev = operands.device
    R = K * sp[0] * sp[1]
    nb = _lib.lib().fs_ridge3d_ws_bytes(K, *sp)
    if nb < 0:
        _lib.check(int(-nb), "fs_ridge3d_ws_bytes")
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    nbytes, flops = ridge_cost(sp, K, op="count")
    with torch.cuda.device(dev):
        _call("fs_ridge_count3d", operands.data_ptr(), cls.data_ptr(), K, *sp, ws.data_ptr(), _stream(operands),
              algo_bytes=nbytes, algo_flops=flops)
    off = torch.zeros((2, R + 1), dtype=torch.int64, device=dev)
    off[:, 1:] = torch.cumsum(ws[:8 * R].view(torch.int32).view(2, R), 1, dtype=torch.int64)
    return ws, off


def ridge_emit(volumes, operands, cls, spacing, valley, ws, row_offsets, V, T, values=True):
    """The second marching pass on its own (fs_ridge_emit3d), on what ridge_nodes and ridge_count returned and the
    totals V and T as host ints.  Returns (vertices, values or None, faces, status) on the device.  Never synchronises;
    launches nothing when V and T are 0."""
    volumes, K, sp, P = _rc_volumes(volumes)
    operands, cls, K2, sp2, _ = _ridge_operands(operands, cls)
    if (K2, sp2) != (K, sp) or operands.device != volumes.device:
        raise ValueError("operands and cls must be those of these volumes (%d x %s), got %d x %s" % (K, sp, K2, sp2))
    hs = _rc_spacing(spacing)
    dev = volumes.device
    V, T = int(V), int(T)
    vert = torch.empty((V, 3), dtype=torch.float32, device=dev)
    vout = torch.empty((V, 2), dtype=torch.float32, device=dev) if values else None
    faces = torch.empty((T, 3), dtype=torch.int32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    if V or T:
        nbytes, flops = ridge_cost(sp, K, V, T, op="emit", values=values)
        with torch.cuda.device(dev):
            _call("fs_ridge_emit3d", volumes.data_ptr(), K, *sp, volumes.stride(0) if K > 1 else P, 1 if valley else 0,
                  operands.data_ptr(), cls.data_ptr(), (ctypes.c_double * 3)(*hs[::-1]), ws.data_ptr(),
                  row_offsets.data_ptr(), V, T, vert.data_ptr(), _ptr(vout), faces.data_ptr(), status.data_ptr(),
                  _stream(volumes), algo_bytes=nbytes, algo_flops=flops)
    return vert, vout, faces, status


def ridge_surfaces(volumes, spacing=1.0, strength=0.0, fmin=-float("inf"), valley=False, values=True):
    """The height-ridge surfaces of K scalar volumes as K indexed triangle meshes, three launches (fs_ridge_nodes3d,
    fs_ridge_count3d, fs_ridge_emit3d): the points where the gradient is orthogonal to the eigenvector e of the Hessian's
    smallest eigenvalue lam and lam <= -strength (Eberly), extracted by Marching Ridges on the Kuhn split of every cell.
    Of an FTLE field (ops.ftle) these are the Lagrangian coherent structures -- repelling ones of a forward field,
    attracting ones of a backward field; valley=True gives the valley surfaces (of lambda2, of a density).  3-D only: in
    2-D ridges are curves.

    volumes: fp32 [K,D,H,W] on a GPU, every extent >= 2; the step stride may be anything.  spacing: the node spacing, one
    value or (D,H,W).  strength >= 0: the least -lam of a ridge node, in units of f / spacing^2.  fmin: nodes with
    f < fmin carry no ridge (-inf: no filter); under valley it applies to -f.  Border nodes carry none either: the
    surface stops one node inside, and next to nodes that are not finite.

    The sign of an eigenvector is arbitrary, so d = e . grad f has no sign of its own: it is oriented per edge from the
    edge's two ends, which makes every cell around an edge agree on its vertex.  A tetrahedron over which e cannot be
    oriented consistently (near degenerate eigenvalues; most of white noise) is TWISTED: it emits nothing and is
    counted -- a hole, not an error.  include/flowsci_hip.h states the definition; tests/ridge_ref.py restates it and
    agrees bit for bit.

    The numbers of vertices and faces depend on the data, so this SYNCHRONISES: exactly once, between the last two
    launches.  `status` is returned, not read: ops.ridge_surfaces_check(result) reads it.  ValueError when a step has
    2^31 - 1 or more vertices or faces.

    Returns a dict on the device: vertices (fp32 [V,3], (x, y, z)), values (fp32 [V,2]: f -- negated under valley -- and
    lam at the vertex; only with values), faces (int32 [T,3], indices local to their step; the winding means nothing: a
    ridge surface need not be orientable), vertex_offsets and face_offsets (int64 [K+1]), counts (int64 [K,4]: vertices,
    faces, twisted tetrahedra, tetrahedra with four eligible corners), classes (int64 [K,5]: nodes per RIDGE_* class),
    operands and cls (what ops.ridge_nodes returned) and status (int32 [1]).  Bitwise reproducible.  Nothing is
    differentiated."""
    volumes, K, sp, P = _rc_volumes(volumes)
    _rc_spacing(spacing)
    operands, cls = ridge_nodes(volumes, spacing, strength, fmin, valley)
    ws, off = ridge_count(operands, cls)
    rows = sp[0] * sp[1]
    R = K * rows
    steps = off[:, ::rows].contiguous()  # [2, K+1]
    host = steps.cpu().numpy()  # the one synchronisation
    per_step = _np.diff(host, axis=1)
    if per_step.size and int(per_step.max()) >= 2 ** 31 - 1:
        raise ValueError("a step has %d vertices or faces: the limit is 2^31 - 2" % int(per_step.max()))
    V, T = int(host[0, -1]), int(host[1, -1])
    vert, vout, faces, status = ridge_emit(volumes, operands, cls, spacing, valley, ws, off, V, T, values)
    per_row = ws[:16 * R].view(torch.int32).view(4, K, rows).sum(2, dtype=torch.int64)
    flat = cls.view(K, -1)
    res = {"vertices": vert, "faces": faces, "vertex_offsets": steps[0], "face_offsets": steps[1],
           "counts": per_row.t().contiguous(),
           "classes": torch.stack([(flat == c).sum(1) for c in range(5)], 1), "operands": operands, "cls": cls,
           "status": status}
    if values:
        res["values"] = vout
    return res


def ridge_surfaces_check(result):
    """Raises FlowsciKernelError when ops.ridge_surfaces' `status` is set (its marching passes disagreed: the arrays are
    then not a mesh).  Synchronises."""
    st = int(result["status"].view(-1)[0]) if isinstance(result["status"], torch.Tensor) else int(result["status"])
    if st != 0:
        raise _lib.FlowsciKernelError("fs_ridge_emit3d: the marching passes disagree (status %d)" % st)


# --------------------------------------------------------------------------------------------
# Line integral convolution: a texture averaged along the streamlines of step flows (fs_lic{2,3}d)
# --------------------------------------------------------------------------------------------
LIC_FULL, LIC_OUT, LIC_STAGNANT, LIC_NONFINITE = 0, 1, 2, 3  # FS_LIC_*: how a side of a line ended
LIC_MAX_L = 1024  # FS_LIC_MAX_L
_LIC_METHODS = {"euler": (0, 1), "rk2": (1, 2)}  # name -> (FS_ADV_*, field samples per step)
_LIC_KERNELS = ("box", "hann")


def _lic_length(L):
    if isinstance(L, bool) or int(L) != L or not (0 <= int(L) <= LIC_MAX_L):
        raise ValueError("length must be an integer in 0..%d, got %r" % (LIC_MAX_L, L))
    return int(L)


def lic_weights(L, kernel="box", device="cuda"):
    """fp64 [L+1] weights of ops.lic on `device`: w[0] for the node, w[i] for the i-th sample on either side.  "box":
    all 1; "hann": 0.5 * (1 + cos(pi * i / (L + 1))), computed on the host in fp64."""
    import math
    L = _lic_length(L)
    if kernel == "box":
        w = [1.0] * (L + 1)
    elif kernel == "hann":
        w = [0.5 * (1.0 + math.cos(math.pi * i / (L + 1))) for i in range(L + 1)]
    else:
        raise ValueError("kernel must be one of %s, got %r" % (list(_LIC_KERNELS), kernel))
    return torch.tensor(w, dtype=torch.float64).to(device)


def lic_noise(shape, seed=0, device="cuda"):
    """fp32 white noise, uniform in [0,1), of spatial `shape`: drawn by a CPU generator seeded with `seed` and copied
    to `device`, so a seed names the same texture on every device."""
    shape = tuple(int(s) for s in shape)
    if len(shape) < 1 or min(shape) < 1:
        raise ValueError("shape must have every extent >= 1, got %r" % (shape,))
    g = torch.Generator(device="cpu")
    g.manual_seed(int(seed))
    return torch.rand(shape, generator=g, dtype=torch.float32).to(device)


def lic_cost(shape, K, L, method="rk2", with_ends=True, with_count=True, shared_tex=False):
    """(HBM bytes, flops) the algorithm needs for one lic call on K fields of spatial `shape` with L steps each way,
    every line at full length (lines that leave the grid or stagnate do less): the fields and the textures read once,
    out / ends / count written once, the weights read once (the packed image the kernel samples from, 16 bytes per
    node written and read again, is the implementation's and not counted).  Flops per field sample as in advect_cost (2^C corner
    weights of C - 1 products, 2 per corner and plane, ~4 C for clamp / floor / fractions), plus 2 C for n2 and its root
    and C divisions, 2 C for the point it is taken at; per texture sample the same with one plane, plus 3 for the two
    sums and ~2 C for the classification; 5 for the node's quotient."""
    if method not in _LIC_METHODS:
        raise ValueError("method must be one of %s, got %r" % (sorted(_LIC_METHODS), method))
    L = _lic_length(L)
    shape = tuple(int(s) for s in shape)
    C = len(shape)
    if C not in (2, 3) or min(shape) < 1:
        raise ValueError("shape must be (H,W) or (D,H,W) with every extent >= 1, got %r" % (shape,))
    K = int(K)
    plane = 1
    for s in shape:
        plane *= s
    nbytes = 4 * K * C * plane + 4 * (1 if shared_tex else K) * plane + 4 * K * plane + 8 * (L + 1)
    nbytes += (K * plane if with_ends else 0) + (4 * K * plane if with_count else 0)
    corners = 1 << C
    vsample = corners * (C - 1) + 2 * corners * C + 4 * C + 3 * C + 2 * C
    tsample = corners * (C - 1) + 2 * corners + 4 * C + 3 + 2 * C
    per_node = 2 * L * _LIC_METHODS[method][1] * vsample + (2 * L + 1) * tsample + 5
    return nbytes, K * plane * per_node


def lic(flows, tex, length=16, h=0.5, method="rk2", kernel="box", vmin=0.0, with_ends=True, with_count=True):
    """Line integral convolution of K steady fields in one launch (fs_lic{2,3}d): every node's value is `tex` averaged
    along the streamline of the normalised field through that node, `length` steps of `h` elements each way.

    flows: [K,2,H,W] or [K,3,D,H,W] fp32 on a GPU (channel 0 along W); the step stride may be anything (flows[::2]
    passes as it is).  tex: [*sp] (one texture for every step) or [K,*sp] (a pass's output fed back).  method: "euler"
    or "rk2" (midpoint) on the unit direction field.  kernel: "box", "hann" or an fp64-convertible weight tensor
    [length+1] (w[0] the node's, w[i] the i-th sample's on either side), which is validated on the host -- all finite,
    w[0] > 0, the others >= 0 -- with ONE synchronisation when it lives on a device; the named kernels never
    synchronise.  vmin: a side ends STAGNANT where the speed is not above vmin (0: only where it is exactly 0).

    All arithmetic is fp64 (include/flowsci_hip.h states the order of operations; tests/lic_ref.py restates it and
    agrees bit for bit).  A side also ends where the next point would leave the grid (OUT: the border is inside, the
    exit point is not sampled) or the field is not finite (NONFINITE); a non-finite texture value propagates.

    Returns a dict: out fp32 [K,*sp]; ends uint8 [K,*sp] (LIC_* of the forward side | the backward side's << 2) or
    None; count int32 [K,*sp] (the samples averaged, the node's included) or None.  The call allocates the kernel's
    workspace, 16 bytes per node and step, for its own duration.  A measurement on detached values: nothing is
    differentiated."""
    if method not in _LIC_METHODS:
        raise ValueError("method must be one of %s, got %r" % (sorted(_LIC_METHODS), method))
    L = _lic_length(length)
    h, vmin = float(h), float(vmin)
    if not (0.0 < h < float("inf")):
        raise ValueError("h must be finite and > 0, got %r" % (h,))
    if not (0.0 <= vmin < float("inf")):
        raise ValueError("vmin must be finite and >= 0, got %r" % (vmin,))
    flows, nd = _advect_flows(flows)
    dev = flows.device
    K = int(flows.shape[0])
    sp = tuple(int(s) for s in flows.shape[2:])
    if not isinstance(tex, torch.Tensor):
        raise ValueError("tex must be a tensor")
    if not tex.is_cuda:
        raise ValueError("tex must live on a GPU (the HIP hot path has no CPU fallback); got %s" % (tex.device,))
    if tex.device != dev:
        raise ValueError("tex must be on the flows' device %s, got %s" % (dev, tex.device))
    if tuple(tex.shape) not in (sp, (K,) + sp):
        raise ValueError("tex must be %s or %s, got %s" % (sp, (K,) + sp, tuple(tex.shape)))
    tex = tex.detach()
    if tex.dtype != torch.float32:
        tex = tex.to(torch.float32)
    tex = tex.contiguous()
    plane = 1
    for v in sp:
        plane *= v
    shared = tex.dim() == nd
    if isinstance(kernel, str):
        w = lic_weights(L, kernel, dev)
    else:
        w = torch.as_tensor(kernel).detach().to(torch.float64).reshape(-1)
        if w.numel() != L + 1:
            raise ValueError("a weight tensor must hold length + 1 = %d values, got %d" % (L + 1, w.numel()))
        wh = w.cpu()  # the one synchronisation
        if not bool(torch.isfinite(wh).all()) or not float(wh[0]) > 0.0 or bool((wh[1:] < 0).any()):
            raise ValueError("weights must be finite with w[0] > 0 and the others >= 0")
        w = w.to(dev).contiguous()
    out = torch.empty((K,) + sp, dtype=torch.float32, device=dev)
    ends = torch.empty((K,) + sp, dtype=torch.uint8, device=dev) if with_ends else None
    count = torch.empty((K,) + sp, dtype=torch.int32, device=dev) if with_count else None
    fss = flows.stride(0) if K > 1 else nd * plane  # (a single field's step stride is never used)
    nbytes, flops = lic_cost(sp, K, L, method, with_ends, with_count, shared)
    wsb = getattr(_lib.lib(), "fs_lic%dd_ws_bytes" % nd)(K, *sp)
    if wsb < 0:
        _lib.check(int(-wsb), "fs_lic%dd_ws_bytes" % nd)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)  # the packed (field, texture) image: 16 bytes per node and step
    args = (flows.data_ptr(), K, nd) + sp + (fss, tex.data_ptr(), 0 if shared else plane, w.data_ptr(), L, h, vmin,
                                             _LIC_METHODS[method][0], out.data_ptr(), _ptr(ends), _ptr(count),
                                             ws.data_ptr(), _stream(flows))
    with torch.cuda.device(dev):
        _call("fs_lic%dd" % nd, *args, algo_bytes=nbytes, algo_flops=flops)
    return {"out": out, "ends": ends, "count": count}


# --------------------------------------------------------------------------------------------
# Streamlines: lines through step flows kept as geometry (fs_streamlines{2,3}d)
# --------------------------------------------------------------------------------------------
SL_FULL, SL_OUT, SL_STAGNANT, SL_NONFINITE, SL_CAPTURED, SL_INVALID = 0, 1, 2, 3, 4, 5  # FS_SL_*: how a line ended
streamline_end_names = ("full", "out", "stagnant", "nonfinite", "captured", "invalid")  # by FS_SL_* code


def _sl_steps(M):
    if isinstance(M, bool) or int(M) != M or int(M) < 1:
        raise ValueError("max_steps must be an integer >= 1, got %r" % (M,))
    return int(M)


def streamlines_cost(shape, S, M, method="rk4"):
    """(HBM bytes, flops) the algorithm needs for one streamlines call of S lines of M steps on fields of spatial
    `shape`, every line at full length: every field element the gathers can reach read once (at most what the
    S * M * stages samples of 2^C corners x C planes ask for; the fields a call does not visit are not known here, so no
    whole-field cap applies), seeds (8 C), step, sign and home (9) read, the M + 1 slots (4 C each), length, end and hit
    (9) written, one capture byte read per step.  Flops per sample as in lic_cost: the field sample of advect_cost plus
    2 C for n2 and its root, C divisions and 2 C for the stage point; ~4 C per step for the update, its classification
    and the cell (RK4: 5 C more for the stage sum)."""
    if method not in _ADV_METHODS:
        raise ValueError("method must be one of %s, got %r" % (sorted(_ADV_METHODS), method))
    M = _sl_steps(M)
    shape = tuple(int(s) for s in shape)
    C = len(shape)
    if C not in (2, 3) or min(shape) < 2:
        raise ValueError("shape must be (H,W) or (D,H,W) with every extent >= 2, got %r" % (shape,))
    S = int(S)
    if S < 0:
        raise ValueError("S must be >= 0, got %d" % S)
    stages = _ADV_METHODS[method][1]
    samples = S * M * stages
    corners = 1 << C
    nbytes = 4 * samples * corners * C + S * (8 * C + 9 + 4 * C * (M + 1) + 9 + M)
    per_sample = corners * (C - 1) + 2 * corners * C + 4 * C + 3 * C + 2 * C
    return nbytes, samples * per_sample + S * M * (4 * C + (5 * C if method == "rk4" else 0))


def streamlines(flows, seeds, step, sign, home=None, capture=None, max_steps=256, h=0.5, vmin=0.0, method="rk4"):
    """Streamlines of steady step flows as geometry, one launch (fs_streamlines{2,3}d): line s starts at seeds[s] and
    follows the NORMALISED field flows[step[s]] -- with it, or against it where sign[s] < 0 -- for up to `max_steps`
    steps of `h` elements of arc length; every vertex is kept.

    flows: [K,2,H,W] or [K,3,D,H,W] fp32 on a GPU (channel 0 along W), every extent >= 2; the step stride may be
    anything.  seeds: fp64 [S,C] on the flows' device, (x, y(, z)) in elements.  step: int32 [S].  sign: int8 [S].
    home: int32 [S] or None: the cell (its origin node's linear index within the step) a line may start in without being
    captured there, -1 for none.  capture: uint8 [K,*sp] or None: a nonzero byte at a cell's origin node ends a line that
    steps into that cell (CAPTURED) once it has left its home.  method: "euler", "rk2" (midpoint) or "rk4" on the unit
    direction field.  vmin: a line ends STAGNANT where the speed is not above vmin.

    All arithmetic is fp64 and positions stay fp64 for the whole line (include/flowsci_hip.h states the order of
    operations; tests/streamline_ref.py restates it and agrees bit for bit).  A line also ends where the next point
    would leave the grid (OUT: the border is inside, the exit point is not stored), where the field is not finite
    (NONFINITE) or after max_steps (FULL); a seed outside the grid (OUT), a seed that is not finite (NONFINITE) and a
    step outside 0..K-1 (INVALID) end a line of length 0.

    Returns a dict on the device: verts fp32 [max_steps+1, C, S] (allocated uninitialised: of line s only
    verts[0 .. length[s], :, s] are defined; slot 0 is the seed), length int32 [S], end uint8 [S] (SL_*; names in
    streamline_end_names), hit int32 [S] (the capturing cell, else -1).  Never synchronises.  A measurement on detached
    values: nothing is differentiated."""
    if method not in _ADV_METHODS:
        raise ValueError("method must be one of %s, got %r" % (sorted(_ADV_METHODS), method))
    M = _sl_steps(max_steps)
    h, vmin = float(h), float(vmin)
    if not (0.0 < h < float("inf")):
        raise ValueError("h must be finite and > 0, got %r" % (h,))
    if not (0.0 <= vmin < float("inf")):
        raise ValueError("vmin must be finite and >= 0, got %r" % (vmin,))
    flows, nd = _advect_flows(flows)
    dev = flows.device
    K = int(flows.shape[0])
    sp = tuple(int(s) for s in flows.shape[2:])
    if min(sp) < 2:
        raise ValueError("every extent of flows must be >= 2, got %s" % (sp,))
    plane = 1
    for v in sp:
        plane *= v

    def operand(name, t, dtype, shape):
        if not isinstance(t, torch.Tensor):
            raise ValueError("%s must be a tensor" % name)
        if not t.is_cuda:
            raise ValueError("%s must live on a GPU (the HIP hot path has no CPU fallback); got %s" % (name, t.device))
        if t.device != dev:
            raise ValueError("%s must be on the flows' device %s, got %s" % (name, dev, t.device))
        if t.dtype != dtype or tuple(t.shape) != shape:
            raise ValueError("%s must be a %s tensor of shape %s, got %s %s" % (name, dtype, shape, t.dtype, tuple(t.shape)))
        return t.detach().contiguous()

    if not isinstance(seeds, torch.Tensor) or seeds.dim() != 2 or seeds.shape[1] != nd:
        raise ValueError("seeds must be an fp64 tensor [S,%d] for %d-D flows, got %s" %
                         (nd, nd, tuple(seeds.shape) if isinstance(seeds, torch.Tensor) else type(seeds).__name__))
    S = int(seeds.shape[0])
    seeds = operand("seeds", seeds, torch.float64, (S, nd))
    step = operand("step", step, torch.int32, (S,))
    sign = operand("sign", sign, torch.int8, (S,))
    home = None if home is None else operand("home", home, torch.int32, (S,))
    capture = None if capture is None else operand("capture", capture, torch.uint8, (K,) + sp)
    res = {"verts": torch.empty((M + 1, nd, S), dtype=torch.float32, device=dev),
           "length": torch.empty(S, dtype=torch.int32, device=dev), "end": torch.empty(S, dtype=torch.uint8, device=dev),
           "hit": torch.empty(S, dtype=torch.int32, device=dev)}
    if S == 0:
        return res
    sc = seeds.t().contiguous()  # [C,S]: a wave's loads of a component are coalesced
    fss = flows.stride(0) if K > 1 else nd * plane  # (a single field's step stride is never used)
    nbytes, flops = streamlines_cost(sp, S, M, method)
    args = (flows.data_ptr(), K, nd) + sp + (fss, sc.data_ptr(), S, S, step.data_ptr(), sign.data_ptr(), _ptr(home),
                                             _ptr(capture), plane, M, h, vmin, _ADV_METHODS[method][0],
                                             res["verts"].data_ptr(), nd * S, S, res["length"].data_ptr(),
                                             res["end"].data_ptr(), res["hit"].data_ptr(), _stream(flows))
    with torch.cuda.device(dev):
        _call("fs_streamlines%dd" % nd, *args, algo_bytes=nbytes, algo_flops=flops)
    return res


# --------------------------------------------------------------------------------------------
# Training batches out of a device-resident stored series (fs_triplet_gather, fs_series_stats)
# --------------------------------------------------------------------------------------------
import numpy as _np

SERIES_DTYPES = {torch.uint8: 0, torch.uint16: 1, torch.float16: 2, torch.float32: 3}  # FS_SERIES_*
# include/flowsci_hip.h `FsTripletJob`: one 64-byte record per sample
TRIPLET_JOB = _np.dtype([("off", "<i8", (3,)), ("z0", "<i4"), ("y0", "<i4"), ("x0", "<i4"), ("flip", "<u4"),
                         ("lo", "<f4"), ("inv", "<f4"), ("reserved", "<i4", (4,))])
assert TRIPLET_JOB.itemsize == 64


def triplet_gather_cost(batch, crop, itemsize):
    """(HBM bytes, flops) one triplet_gather needs: three frames' crops read once in the stored type, the fp32 tensor
    written once; a subtract and a multiply per element."""
    n = 3 * int(batch)
    for s in crop:
        n *= int(s)
    return n * (int(itemsize) + 4), 2 * n


def _stored_operand(stored):
    if not isinstance(stored, torch.Tensor):
        raise ValueError("stored must be a tensor")
    if stored.dtype not in SERIES_DTYPES:
        raise ValueError("stored must be uint8, uint16, float16 or float32, got %s" % stored.dtype)
    if not stored.is_cuda:
        raise ValueError("stored must live on a GPU (the HIP hot path has no CPU fallback); got %s" % stored.device)
    if not stored.is_contiguous():
        raise ValueError("stored must be contiguous")
    return stored


def check_triplet_jobs(jobs, n_elems, frame, crop):
    """Host-side validation of a plan (numpy records of TRIPLET_JOB) against a stored array of `n_elems` elements with
    frames of `frame` = (Ds, Hs, Ws), cropped to `crop` = (Do, Ho, Wo): every frame inside the array, every crop inside
    its frame, known flip bits, finite normalisation.  ValueError names the first offending record."""
    jobs = _np.asarray(jobs)
    if jobs.dtype != TRIPLET_JOB or jobs.ndim != 1:
        raise ValueError("jobs must be a 1-D numpy array of ops.TRIPLET_JOB records")
    F = int(frame[0]) * int(frame[1]) * int(frame[2])
    bad = ((jobs["off"] < 0) | (jobs["off"] > n_elems - F)).any(axis=1)
    for k, (f, c) in zip(("z0", "y0", "x0"), zip(frame, crop)):
        bad |= (jobs[k] < 0) | (jobs[k] > int(f) - int(c))
    bad |= jobs["flip"] > 7
    bad |= ~(_np.isfinite(jobs["lo"]) & _np.isfinite(jobs["inv"]))
    if bad.any():
        i = int(_np.flatnonzero(bad)[0])
        raise ValueError("triplet job %d leaves the stored array (%d elements, frames %s, crop %s) or is malformed: %r"
                         % (i, n_elems, tuple(frame), tuple(crop), jobs[i]))
    return jobs


def upload_triplet_jobs(jobs, stored, crop, checked=False):
    """Validate numpy TRIPLET_JOB records against `stored` (frames = its trailing len(crop) axes) and copy them to its
    device in one transfer: an int64 [n, 8] tensor, one row per record, of which triplet_gather takes slices.
    checked=True: the caller has run check_triplet_jobs on these records against this array already."""
    stored = _stored_operand(stored)
    frame, crop3 = _series_frame(stored, crop)
    if not checked:
        jobs = check_triplet_jobs(jobs, stored.numel(), frame, crop3)
    host = torch.from_numpy(_np.ascontiguousarray(jobs).view("<i8").reshape(-1, 8))
    return host.to(stored.device)


def _series_frame(stored, crop):
    nd = len(crop)
    if nd not in (2, 3) or stored.dim() < nd + 1:
        raise ValueError("crop must have 2 or 3 extents and stored at least one more axis, got crop %s, stored %s" %
                         (tuple(crop), tuple(stored.shape)))
    frame = (1,) * (3 - nd) + tuple(int(s) for s in stored.shape[-nd:])
    crop3 = (1,) * (3 - nd) + tuple(int(s) for s in crop)
    if any(c < 1 or c > f for c, f in zip(crop3, frame)):
        raise ValueError("crop %s does not fit frames of %s" % (tuple(crop), frame[3 - nd:]))
    return frame, crop3


def triplet_gather(stored, jobs, out_shape, out=None):
    """One training batch [B,3,*crop] (fp32; channels img0, img1, gt) out of a stored series on the GPU, one launch
    (fs_triplet_gather): per sample a TRIPLET_JOB record names three frames, a crop origin, mirrors and (lo, inv);
    out = (float(v) - lo) * inv with non-finite v read as 0.

    stored: contiguous uint8 / uint16 / float16 / float32 GPU tensor whose trailing 3 (2) axes are a frame.
    jobs: numpy TRIPLET_JOB records (validated here, then uploaded), or rows of the tensor upload_triplet_jobs
    returned (validated there; nothing is copied or synchronised).  An int64 [B,8] tensor from anywhere else is NOT
    validated -- it is device memory -- only guarded: the kernel reads 0 wherever such a record leaves the frame or
    the array.  out_shape: (B, 3, Do, Ho, Wo) or (B, 3, Ho, Wo)."""
    stored = _stored_operand(stored)
    out_shape = tuple(int(s) for s in out_shape)
    if len(out_shape) not in (4, 5) or out_shape[1] != 3 or out_shape[0] < 1:
        raise ValueError("out_shape must be (B,3,Do,Ho,Wo) or (B,3,Ho,Wo), got %s" % (out_shape,))
    frame, crop3 = _series_frame(stored, out_shape[2:])
    B = out_shape[0]
    if isinstance(jobs, _np.ndarray):
        jobs = upload_triplet_jobs(jobs, stored, out_shape[2:])
    if (not isinstance(jobs, torch.Tensor) or jobs.dtype != torch.int64 or jobs.dim() != 2 or jobs.shape[1] != 8 or
            not jobs.is_contiguous() or jobs.device != stored.device):
        raise ValueError("jobs must be numpy TRIPLET_JOB records or a contiguous int64 [B,8] tensor on stored's device")
    if jobs.shape[0] != B:
        raise ValueError("%d job records for a batch of %d" % (jobs.shape[0], B))
    if out is None:
        out = torch.empty(out_shape, dtype=torch.float32, device=stored.device)
    elif (not isinstance(out, torch.Tensor) or out.dtype != torch.float32 or tuple(out.shape) != out_shape or
          not out.is_contiguous() or out.device != stored.device):
        raise ValueError("out must be a contiguous float32 %s tensor on stored's device" % (out_shape,))
    nbytes, flops = triplet_gather_cost(B, crop3, stored.element_size())
    with torch.cuda.device(stored.device):
        _call("fs_triplet_gather", stored.data_ptr(), SERIES_DTYPES[stored.dtype], stored.numel(), *frame,
              jobs.data_ptr(), B, *crop3, out.data_ptr(), _stream(stored), algo_bytes=nbytes, algo_flops=flops)
    return out


def series_stats(stored):
    """Per frame stored[t] (uint8 / uint16 / float16 / float32 on a GPU, contiguous): an fp64 [T,3] tensor of the
    minimum and maximum over its finite elements (+inf / -inf if none) and the count of non-finite elements
    (fs_series_stats: two deterministic launches, nothing synchronised)."""
    stored = _stored_operand(stored)
    if stored.dim() < 2 or stored.numel() == 0:
        raise ValueError("stored must be [T, ...] with at least one element, got %s" % (tuple(stored.shape),))
    T = int(stored.shape[0])
    F = stored.numel() // T
    nb = _lib.lib().fs_series_stats_ws_bytes(T, F)
    if nb < 0:
        _lib.check(int(-nb), "fs_series_stats_ws_bytes")
    ws = torch.empty(nb // 8, dtype=torch.float64, device=stored.device)
    out = torch.empty(T, 3, dtype=torch.float64, device=stored.device)
    with torch.cuda.device(stored.device):
        _call("fs_series_stats", stored.data_ptr(), SERIES_DTYPES[stored.dtype], T, F, ws.data_ptr(), out.data_ptr(),
              _stream(stored), algo_bytes=stored.numel() * stored.element_size())
    return out


def series_encode_cost(shape_out, itemsize):
    """(HBM bytes, flops) one series_encode needs by the algorithm: every kept element read once as fp32 and written
    once in the stored type (the padding is never touched); a multiply and an add per element."""
    n = 1
    for s in shape_out:
        n *= int(s)
    return n * (4 + int(itemsize)), 2 * n


def _series_dtype(dtype):
    if isinstance(dtype, torch.dtype):
        t = dtype
    else:
        t = getattr(torch, _np.dtype(dtype).name, None)
    if t not in SERIES_DTYPES:
        raise ValueError("dtype must be uint8, uint16, float16 or float32, got %r" % (dtype,))
    return t


def series_encode(x, dtype, spatial, lo=0.0, span=1.0, out=None, stats=True):
    """The inverse of the gather's decode, one launch (fs_series_encode): the corner [:D,:H,:W] ([:H,:W]) of the padded
    fp32 planes x [N,C,*padded] written as a contiguous `dtype` [N,C,*spatial] tensor, y = x * span + lo (two rounded
    fp32 operations); uint8 / uint16 clamp and round to nearest even, float16 saturates at +-65504, a non-finite y is
    stored as 0.  Returns (stored tensor, stats): stats an fp64 [N,5] tensor {min y, max y over the finite y before
    clamping, n_low, n_high, n_nonfinite} per item (a second, fixed-order launch; nothing synchronises), or None with
    stats=False.  out: a contiguous `dtype` [N,C,*spatial] tensor on x's device to write into, e.g. a view into a
    larger staging buffer."""
    if not isinstance(x, torch.Tensor):
        raise ValueError("x must be a tensor")
    if not x.is_cuda:
        raise ValueError("x must live on a GPU (the HIP hot path has no CPU fallback); got %s" % x.device)
    spatial = tuple(int(s) for s in spatial)
    nd = len(spatial)
    if nd not in (2, 3) or x.dtype != torch.float32 or x.dim() != nd + 2:
        raise ValueError("x must be float32 [N,C,*padded] with %d padded extents for spatial %s, got %s %s" %
                         (nd, spatial, x.dtype, tuple(x.shape)))
    tdt = _series_dtype(dtype)
    x = x.contiguous()
    N, C = int(x.shape[0]), int(x.shape[1])
    padded = tuple(int(s) for s in x.shape[2:])
    if N < 1 or C < 1 or any(s < 1 or s > p for s, p in zip(spatial, padded)):
        raise ValueError("spatial %s does not fit the planes of x %s" % (spatial, tuple(x.shape)))
    shape = (N, C) + spatial
    if out is None:
        out = torch.empty(shape, dtype=tdt, device=x.device)
    elif (not isinstance(out, torch.Tensor) or out.dtype != tdt or tuple(out.shape) != shape or
          not out.is_contiguous() or out.device != x.device):
        raise ValueError("out must be a contiguous %s %s tensor on x's device" % (tdt, shape))
    p3, s3 = (1,) * (3 - nd) + padded, (1,) * (3 - nd) + spatial
    ws = st = None
    if stats:
        nb = _lib.lib().fs_series_encode_ws_bytes(N, C, *s3)
        if nb < 0:
            _lib.check(int(-nb), "fs_series_encode_ws_bytes")
        ws = torch.empty(nb // 8, dtype=torch.float64, device=x.device)
        st = torch.empty(N, 5, dtype=torch.float64, device=x.device)
    nbytes, flops = series_encode_cost(shape, out.element_size())
    with torch.cuda.device(x.device):
        _call("fs_series_encode", x.data_ptr(), N, C, *p3, out.data_ptr(), SERIES_DTYPES[tdt], *s3, float(lo),
              float(span), _ptr(ws), _ptr(st), _stream(x), algo_bytes=nbytes, algo_flops=flops)
    return out, st
