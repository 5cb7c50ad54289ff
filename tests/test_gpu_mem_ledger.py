"""GPU (-m gpu): every row of the ledger of the warp and resize kernels (tests/mem_ledger.py) on the device.

Per row: one raw ctypes call of the C-ABI entry point with the row's inputs at the row's misalignments and batch strides;
the launched kernels recorded with torch.profiler must contain the row's compute kernel(s) and no other kernel of
warp3d.hip / interp.hip; status 0; every output (both warps, flow_out, grad_flow / grad_flow_total, grad_img*, grad_delta,
the resizes) within the row's band of the fp64 reference at EVERY element; every output, workspace and zero-filled
accumulator lives inside 4096-float guard bands of a NaN bit pattern that must be bitwise unchanged afterwards.  Fully
overwritten outputs start as that pattern (an unwritten element fails the comparison), grad_in / grad_img* start at zero
as the ABI requires.  Aliasing rows compare against warp gradient + a snapshot of add0.  Row-cache rows run the same
operands again through the gather kernels (forward: a duplicated channel, C = 2; backward: grad_in asked for), witness
those by name and require equal bits.  A summary line per row (kernels, errors over band, time) is printed.

The argument errors these entry points define are refused with their status before anything is launched or written."""
import ctypes
import os
import sys
import time

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mem_ledger as LG  # noqa: E402
from ledger_harness import DEV, Guarded, kernels_launched, load_lib, on_device, stream as _stream  # noqa: E402
import mem_ledger_inputs as I  # noqa: E402

pytestmark = pytest.mark.gpu

FS_ERR_NULLPTR, FS_ERR_ARG = 1, 3
WIDE = 11  # channels of the wider tensors the strided operands are slices of
# how the kernels of the two sources are named: a launched kernel of that kind that is not a ledger symbol is an error
PREFIXES = ("warp3d_", "upsample3d_", "downsample3d_", "interp3d_", "interp_axis_", "up_adjoint_", "resize2d_")
KNOWN = {k for r in LG.ROWS for k in LG.kernels_of(r)} | set(LG.UNREACHABLE_IN_PRODUCT) | LG.HELPERS


@pytest.fixture(scope="module")
def lib():
    return load_lib()


def slice_of_wide(t, c0, mis=0, odd_stride=False):
    """`t` [B, c, ...] on the GPU as channels c0 .. c0 + c of a WIDE-channel tensor (seeded noise elsewhere); the wide
    tensor starts `mis` floats past a 16-byte boundary; odd_stride: one spare float per sample, so its batch stride is
    not a multiple of 4.  Returns (view, batch stride in floats)."""
    B, c = t.shape[:2]
    vol = I.numel(t.shape[2:])
    bs = WIDE * vol + (1 if odd_stride else 0)
    buf = torch.randn(B * bs + 4, generator=torch.Generator().manual_seed(vol + c0)).to(DEV)
    wide = buf[mis:mis + B * bs].as_strided((B, WIDE) + tuple(t.shape[2:]), (bs, vol) + tuple(t.stride()[2:]))
    v = wide[:, c0:c0 + c]
    v.copy_(t)
    assert (v.data_ptr() - 4 * c0 * vol) % 16 == 4 * mis
    return v, bs


def _kernels_launched(fn):
    """(fn's return value, normalized names of the warp3d.hip / interp.hip kernels it launched); one the ledger does not
    know is an error."""
    return kernels_launched(fn, LG.normalize, lambda n: n in KNOWN or n.startswith(PREFIXES), KNOWN)


def _dhw(ext):
    return (ctypes.c_int * 3)(*ext)


# ---- one row --------------------------------------------------------------------------------------------------------
class Call:
    """Device operands, guarded outputs and the launch of one row.  `variant`: None, "c2" (forward with the image
    channel duplicated) or "gin" (backward with grad_in asked for) -- the gather-kernel twins of a row-cache row."""

    def __init__(self, lib, r, T, variant=None):
        self.lib, self.r, self.variant = lib, r, variant
        op, m = r["op"], r["mis"]
        self.C = 2 if variant == "c2" else r["C"]
        self.with_gin = r["with_grad_in"] or variant == "gin"
        self.bufs, self.D, self.bs = {}, {}, {}
        self.snap0 = None
        B, C = r["B"], self.C
        for name, t in T.items():
            if name in ("in0", "in1") and variant == "c2":
                t = torch.cat((t, t), 1)
            if name.startswith("gout") and op in LG.BWD_OPS and r["gout_strided"]:
                self.D[name], self.bs[name] = slice_of_wide(t, 2 + int(name[-1]), m.get(name, 0), r["stride_mis"] == name)
            elif name.startswith("add") and r["add_strided"][int(name[-1])]:
                self.D[name], self.bs[name] = slice_of_wide(t, 5, m.get(name, 0), r["stride_mis"] == name)
            elif op == "down_ms" and name == "in":
                self.D["planes"] = []
                for c in range(C):  # channel c as plane 0 of its own 2-channel tensor (a spare channel)
                    vol = I.numel(t.shape[2:])
                    odd = r["stride_mis"] == "src%d" % c
                    bs = 2 * vol + (1 if odd else 0)
                    mm = m.get("src%d" % c, 0)
                    buf = torch.zeros(B * bs + 4, device=DEV)
                    pl = buf[mm:mm + B * bs].as_strided((B,) + tuple(t.shape[2:]), (bs,) + tuple(t[:, 0].stride()[1:]))
                    pl.copy_(t[:, c])
                    self.D["planes"].append((pl, bs))
            else:
                self.D[name] = on_device(t, m.get(name, 0))
                if name.startswith("add"):
                    self.bs[name] = 6 * I.numel(t.shape[2:])
                if name.startswith("gout") and op in LG.BWD_OPS:
                    self.bs[name] = 0
        fe = I.flow_ext(r)
        nf, ni = I.numel(fe), I.numel(I.img_ext(r))
        npair = 2 if op in LG.PAIR_OPS else 1
        if op in ("w_fwd", "wp_fwd", "uw_fwd"):
            for i in range(npair):
                self.bufs["out%d" % i] = Guarded(B * C * nf, mis=m.get("out%d" % i, 0))
            if op == "uw_fwd":
                self.bufs["fout"] = Guarded(B * 6 * nf, mis=m.get("fout", 0))
        elif op in LG.BWD_OPS:
            if r["with_grad_flow"]:
                self.bufs["gflow"] = Guarded(B * 3 * npair * nf, mis=m.get("gflow", 0))
                if r["alias"]:  # add0 IS grad_flow6
                    self.bufs["gflow"].t.copy_(T["add0"].reshape(-1))
                    self.snap0 = T["add0"].double()
            if self.with_gin:
                for i in range(npair):
                    self.bufs["gin%d" % i] = Guarded(B * C * ni, zero=True, mis=m.get("gin%d" % i, 0))
            if op.startswith("uw_"):
                self.bufs["gdelta"] = Guarded(B * 6 * I.numel(r["ext"]))
                self.bufs["ws"] = Guarded(I.ws_floats(r))
        elif op in ("up_add", "down", "down_ms", "r2_fwd"):
            f = r["factor"]
            up = op == "up_add" or (op == "r2_fwd" and r["upsample"])
            self.oe = tuple(n * f if up else n // f for n in r["ext"])
            self.bufs["out"] = Guarded(B * C * I.numel(self.oe), mis=m.get("out", 0))
        else:
            self.bufs["gin"] = Guarded(B * C * I.numel(r["ext"]), mis=m.get("gin", 0))
            if r["with_ws"]:
                self.bufs["ws"] = Guarded(I.ws_floats(r))

    def p(self, name):
        if name in self.bufs:
            return self.bufs[name].ptr()
        return self.D[name].data_ptr() if name in self.D else None

    def add_args(self):
        out = []
        for i in range(3):
            name = "add%d" % i
            if i == 0 and self.r["alias"]:
                out += [self.p("gflow"), 6 * I.numel(I.flow_ext(self.r))]
            elif name in self.D:
                out += [self.p(name), self.bs[name]]
            else:
                out += [None, 0]
        return out

    def launch(self):
        lib, r, p, st = self.lib, self.r, self.p, _stream()
        op, B, C, f = r["op"], r["B"], self.C, r["factor"]
        dhw = _dhw(r["inp"]) if r["inp"] else None
        fe = I.flow_ext(r)
        if op == "w_fwd":
            return lib.fs_warp3d_fwd(p("in0"), p("flow"), p("out0"), B, C, dhw, *fe, st)
        if op == "w_bwd":
            return lib.fs_warp3d_bwd(p("in0"), p("flow"), p("gout0"), p("gin0"), p("gflow"), B, C, dhw, *fe, st)
        if op == "wp_fwd":
            return lib.fs_warp3d_pair_fwd(p("in0"), p("in1"), p("flow"), p("out0"), p("out1"), B, C, dhw, *fe, st)
        if op == "wp_bwd":
            return lib.fs_warp3d_pair_bwd(p("in0"), p("in1"), p("flow"), p("gout0"), p("gout1"), p("gin0"), p("gin1"),
                                          p("gflow"), B, C, dhw, *fe, st)
        if op == "wp_acc":
            return lib.fs_warp3d_pair_bwd_acc(p("in0"), p("in1"), p("flow"), p("gout0"), p("gout1"), p("gin0"), p("gin1"),
                                              self.add_args()[0], p("gflow"), B, C, dhw, *fe, st)
        if op == "wp_acc3":
            return lib.fs_warp3d_pair_bwd_acc3(p("in0"), p("in1"), p("flow"), p("gout0"), self.bs["gout0"], p("gout1"),
                                               self.bs["gout1"], p("gin0"), p("gin1"), *self.add_args(), p("gflow"), B, C,
                                               dhw, *fe, st)
        if op == "uw_fwd":
            return lib.fs_upsample_warp3d_pair_fwd(p("in0"), p("in1"), p("delta"), p("prev"), p("fout"), p("out0"),
                                                   p("out1"), B, C, dhw, *r["ext"], f, r["scale"], st)
        if op == "uw_bwd":
            return lib.fs_upsample_warp3d_pair_bwd(p("in0"), p("in1"), p("flow"), p("gout0"), p("gout1"),
                                                   self.add_args()[0], p("gflow"), p("gdelta"), p("ws"), B, C, dhw,
                                                   *r["ext"], f, r["scale"], st)
        if op == "uw_bwd3":
            return lib.fs_upsample_warp3d_pair_bwd3(p("in0"), p("in1"), p("flow"), p("gout0"), self.bs["gout0"],
                                                    p("gout1"), self.bs["gout1"], *self.add_args(), p("gflow"),
                                                    p("gdelta"), p("ws"), B, C, dhw, *r["ext"], f, r["scale"], st)
        if op == "up_add":
            return lib.fs_upsample3d_scale_add(p("small"), p("prev"), p("out"), B, C, *r["ext"], f, r["scale"], st)
        if op == "down":
            return lib.fs_downsample3d_fwd(p("in"), p("out"), B, C, *r["ext"], f, r["scale"], st)
        if op == "down_ms":
            ptrs = (ctypes.c_void_p * C)(*[pl.data_ptr() for pl, _ in self.D["planes"]])
            strides = (ctypes.c_longlong * C)(*[bs for _, bs in self.D["planes"]])
            return lib.fs_downsample3d_fwd_ms(ptrs, strides, p("out"), B, C, *r["ext"], f, r["scale"], st)
        if op in ("ibwd", "ibwd_s"):
            oe = tuple(n * f if r["upsample"] else n // f for n in r["ext"])
            if op == "ibwd":
                return lib.fs_interp3d_bwd(p("gout"), p("gin"), p("ws"), B, C, *r["ext"], *oe, f, r["upsample"], st)
            return lib.fs_interp3d_bwd_scaled(p("gout"), p("gin"), p("ws"), B, C, *r["ext"], *oe, f, r["upsample"],
                                              r["scale"], st)
        oe = tuple(n * f if r["upsample"] else n // f for n in r["ext"])
        fn = lib.fs_resize2d_fwd if op == "r2_fwd" else lib.fs_resize2d_bwd
        return fn(p("in") if op == "r2_fwd" else p("gout"), p("out") if op == "r2_fwd" else p("gin"), B, C, *r["ext"], *oe,
                  f, r["upsample"], r["scale"], st)

    def got(self, name, shape):
        return self.bufs[name].t.view(shape)


def _row_cache_twin(lib, r, T, call):
    """The gather-kernel twin of a row-cache row on the same operands: (witnessed kernels, expected kernel, bits equal)."""
    fwd = r["op"] in ("w_fwd", "wp_fwd")
    twin = Call(lib, r, T, "c2" if fwd else "gin")
    rc, launched = _kernels_launched(twin.launch)
    assert rc == 0, "twin status %d" % rc
    want = LG.RING_V if fwd else LG.BWD_VG
    same = True
    if fwd:
        for name in call.bufs:
            a = call.bufs[name].t.view(r["B"], 1, -1).view(torch.int32)
            b = twin.bufs[name].t.view(r["B"], 2, -1).view(torch.int32)
            same = same and torch.equal(a[:, 0], b[:, 0]) and torch.equal(a[:, 0], b[:, 1])
    else:
        same = torch.equal(call.bufs["gflow"].t.view(torch.int32), twin.bufs["gflow"].t.view(torch.int32))
    assert all(b.intact() for b in twin.bufs.values()), "twin wrote outside its buffers"
    return launched, want, same


@pytest.mark.parametrize("r", LG.ROWS, ids=[LG.row_id(r) for r in LG.ROWS])
def test_ledger_row(lib, r):
    t0 = time.perf_counter()
    T = I.data(r)
    ref = I.results(r, T, torch.float64)
    call = Call(lib, r, T)
    rc, launched = _kernels_launched(call.launch)
    assert rc == 0, "status %d" % rc
    compute = [n for n in launched if n not in LG.HELPERS]
    want = LG.kernels_of(r)
    assert set(want) <= set(compute), "expected %s, launched %s" % (want, launched)
    assert set(compute) == set(want), "other kernels of these sources ran: %s" % launched
    errs = {}
    for name, (rf, tol) in ref.items():
        if name == "gflow" and call.snap0 is not None:  # aliased add0: T["add0"] is the snapshot the reference added
            assert torch.equal(call.snap0.float(), T["add0"])
        g = call.got(name, rf.shape).detach().cpu().double()
        bad = ~torch.isfinite(g)
        errs[name] = float("inf") if bool(bad.any()) else float((g - rf).abs().max()) / I.band(rf, tol)
    twin = None
    if len(want) == 1 and want[0] in (LG.RC_F, LG.RC_B) and not r["mis"]:
        twin = _row_cache_twin(lib, r, T, call)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    print("LEDGER %-8s %-62s err/band %s  %.2fs  %s" % (r["op"], "+".join(want), " ".join("%s=%.3f" % kv for kv in
                                                                                         sorted(errs.items())), dt, r["why"]))
    bad_guard = [name for name, b in call.bufs.items() if not b.intact()]
    assert not bad_guard, "writes outside %s" % bad_guard
    if "ws" in call.bufs and want[-1] == LG.ADJ_FUSED:
        assert call.bufs["ws"].untouched(), "the fused adjoint wrote its workspace"
    assert errs and all(e <= 1.0 for e in errs.values()), errs
    if twin is not None:
        launched2, want2, same = twin
        assert set(launched2) - LG.HELPERS == {want2}, "twin: expected %s, launched %s" % (want2, launched2)
        assert same, "row-cache kernel and %s differ in bits" % want2


# ---- argument errors are refused before anything is launched or written ---------------------------------------------
def _refusals():
    base = dict(B=1, C=1, ext=(5, 8, 8), inp=None, factor=0, scale=1.0, upsample=0, with_ws=False, prev=False, nadd=0,
                add_strided=(False, False, False), gout_strided=False, alias=False, with_grad_in=False, with_grad_flow=True,
                flow=("smooth", "shift"), mis={}, stride_mis=None, kernel="-", plan=None, why="refusal")
    return [
        ("factor 3", dict(base, op="up_add", ext=(4, 4, 8), factor=3, C=2), FS_ERR_ARG, None),
        ("factor 3, fused", dict(base, op="uw_fwd", ext=(3, 4, 4), factor=3), FS_ERR_ARG, None),
        ("stride below the dense size", dict(base, op="wp_acc3", nadd=1), FS_ERR_ARG, "short_stride"),
        ("grad_out stride below the dense size", dict(base, op="wp_acc3", C=2), FS_ERR_ARG, "short_gout"),
        ("scale != 1 without workspace", dict(base, op="ibwd_s", ext=(3, 5, 7), factor=2, upsample=1, scale=2.0, C=2),
         FS_ERR_ARG, None),
        ("scale != 1 on floor extents", dict(base, op="ibwd_s", ext=(5, 7, 9), factor=2, scale=0.5, C=2), FS_ERR_ARG, None),
        ("grad_img0 without grad_img1", dict(base, op="wp_bwd", with_grad_in=True), FS_ERR_NULLPTR, "one_gin"),
    ]


@pytest.mark.parametrize("case", _refusals(), ids=lambda c: c[0].replace(" ", "_"))
def test_argument_errors_are_refused(lib, case):
    _, r, status, tweak = case
    if r["factor"] == 3:  # inputs of a legal factor: only the argument is wrong
        T = I.data(dict(r, factor=2))
        call = Call(lib, dict(r, factor=2), T)
        call.r = r
    else:
        T = I.data(r)
        call = Call(lib, r, T)
    if tweak == "short_stride":
        call.bs["add0"] -= 4
    elif tweak == "short_gout":
        call.bs["gout0"] = r["C"] * I.numel(r["ext"]) - 4
    elif tweak == "one_gin":
        held = call.bufs.pop("gin1")
    rc, launched = _kernels_launched(call.launch)
    assert rc == status, rc
    assert launched == [], launched
    if tweak == "one_gin":
        call.bufs["gin1"] = held
    for name, b in call.bufs.items():
        if name.startswith("gin") and r["op"] == "wp_bwd":
            assert b.intact() and bool((b.t == 0).all()), "%s was written" % name
        else:
            assert b.untouched(), "%s was written" % name
