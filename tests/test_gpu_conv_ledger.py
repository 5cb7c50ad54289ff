"""GPU (-m gpu): every row of the convolution ledger (tests/conv_ledger.py) on the device.

Per row: one call of the C-ABI entry point with seeded O(1) inputs and weights scaled by 1/sqrt(fan_in); the launched
kernels recorded with torch.profiler must contain the row's compute kernel and no other convolution compute kernel;
every output (y, z, the PReLU-backward outputs, dw) must match an fp64 CPU reference of the same operation within
2e-5 x max|ref|; every output, workspace and partial-sum buffer lives inside 4096-float guard bands of a NaN bit
pattern that must be bitwise unchanged afterwards.  Deterministic weight-gradient rows also give the same bits twice
and agree with the atomic form.  A summary line per row (kernel, error, time) is printed.

Misaligned outputs: every fs_conv3d_fwd* / fs_conv3d_tr* entry point refuses a y / z / addend / act_y that is not 16-byte
aligned with FS_ERR_ARG, and nothing is written (the refusal is host code in front of every launch)."""
import ctypes
import math
import os
import sys
import time

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_ledger as LG  # noqa: E402
from ledger_harness import DEV, Guarded, kernels_launched, load_lib, on_device, stream as _stream  # noqa: E402

pytestmark = pytest.mark.gpu

TOL = 2e-5
FS_ERR_ARG = 3


@pytest.fixture(scope="module")
def lib():
    return load_lib()


def _conv_kernels_launched(fn):
    """(fn's return value, normalized names of the convolution kernels it launched)."""
    return kernels_launched(fn, LG.normalize,
                            lambda n: n.startswith("conv3d_") or n.startswith("convtr_") or n in LG.HELPERS)


def _rel(got, ref):
    return float((got.detach().cpu().double() - ref).abs().max() / ref.abs().max().clamp_min(1e-30))


def _prelu(v, a):
    return torch.where(v > 0, v, a.view(1, -1, 1, 1, 1) * v if a.numel() > 1 else a * v)


# ---- one row --------------------------------------------------------------------------------------------------------
def _data(r):
    gen = torch.Generator().manual_seed(sum(map(ord, LG.row_id(r))) % 100003)
    B, cin, cout, k = r["B"], r["cin"], r["cout"], r["k"]
    D = {}
    if r["op"].startswith("wrw"):
        D["g"] = torch.randn(B, cout, *r["out"], generator=gen)
        D["src"] = torch.randn(B, cin, *r["inp"], generator=gen)
        return D
    D["x"] = torch.randn(B, cin, *r["inp"], generator=gen)
    if r["op"].startswith("tr"):
        D["w"] = torch.randn(cin, cout, 4, 4, 4, generator=gen) / math.sqrt(cin * 8)
    elif r["wmode"] == 1:
        D["w"] = torch.randn(cin, cout, k, k, k, generator=gen) / math.sqrt(cin * k ** 3)
    else:
        D["w"] = torch.randn(cout, cin, k, k, k, generator=gen) / math.sqrt(cin * k ** 3)
    D["bias"] = torch.randn(cout, generator=gen)
    D["addend"] = torch.randn(B, cout, *r["out"], generator=gen)
    D["slope"] = torch.rand(cout if r["op"] != "fwd_dprelu" else 1, generator=gen) * 0.5
    D["act_y"] = torch.randn(B, cout, *r["out"], generator=gen)
    return D


def _reference(r, D):
    """fp64 CPU reference: {output name: tensor}."""
    op, k, s, p = r["op"], r["k"], r["stride"], r["pad"]
    if op.startswith("wrw"):
        src = F.pad(D["src"].double(), (p, p, p, p, p, p))
        need = [(o - 1) * s + k for o in r["out"]]
        src = src[:, :, :need[0], :need[1], :need[2]]
        dw = torch.nn.grad.conv3d_weight(src, (r["cout"], r["cin"], k, k, k), D["g"].double(), stride=s, padding=0)
        return {"dw": dw}
    x, w = D["x"].double(), D["w"].double()
    if op.startswith("tr"):
        odd = tuple(o - 2 * i for o, i in zip(r["out"], r["inp"]))
        conv = F.conv_transpose3d(x, w, stride=2, padding=1, output_padding=odd)
    else:
        weff = w if r["wmode"] == 0 else w.transpose(0, 1).flip(2, 3, 4)
        conv = F.conv3d(x, weff, stride=s, padding=p)
    b = D["bias"].double().view(1, -1, 1, 1, 1)
    a = D["slope"].double()
    if op in ("fwd", "tr"):
        return {"y": conv + b}
    if op in ("fwd_add", "tr_add"):
        return {"y": conv + b + D["addend"].double()}
    if op == "fwd_prelu":
        return {"y": conv + b, "z": _prelu(conv + b, a) + D["addend"].double()}
    if op in ("fwd_ms", "tr_prelu"):
        return {"y": conv + b, "z": _prelu(conv + b, a)}
    assert op == "fwd_dprelu"
    act = D["act_y"].double()
    gay = torch.where(act > 0, conv, a * conv)
    ga_terms = torch.where(act > 0, torch.zeros_like(conv), act * conv)
    return {"y": gay, "ga": ga_terms.sum().view(1), "gb": gay.sum(dim=(0, 2, 3, 4)),
            "_ga_abs": ga_terms.abs().sum().view(1), "_gb_abs": gay.abs().sum(dim=(0, 2, 3, 4))}


def _call(lib, r, D, bufs):
    """Launch the row's entry point on `bufs` (outputs / workspaces, Guarded); returns the status."""
    op, B, cin, cout, k, s, p = r["op"], r["B"], r["cin"], r["cout"], r["k"], r["stride"], r["pad"]
    inp, out = r["inp"], r["out"]
    if op.startswith("wrw"):
        g, src = D["g_dev"], D["src_dev"]
        geo = (B, cout, cin, *out, *inp, k, s, p)
        if op == "wrw":
            return lib.fs_conv3d_wrw(g.data_ptr(), src.data_ptr(), bufs["dw"].ptr(), *geo, _stream())
        if op == "wrw_det":
            return lib.fs_conv3d_wrw_det(g.data_ptr(), src.data_ptr(), None, None, bufs["dw"].ptr(), bufs["ws"].ptr(),
                                         bufs["ws"].n, *geo, _stream())
        planes = D["planes"]
        ptrs = (ctypes.c_void_p * cin)(*[pl.data_ptr() for pl in planes])
        strides = (ctypes.c_longlong * cin)(*[pl.stride(0) for pl in planes])
        return lib.fs_conv3d_wrw_ms(g.data_ptr(), ptrs, strides, bufs["dw"].ptr(), *geo, _stream())
    x, w = D["x_dev"], D["w_dev"]
    bias, add, a, act = D["bias_dev"], D["addend_dev"], D["slope_dev"], D["act_y_dev"]
    if op.startswith("tr"):
        geo = (B, cin, cout, *inp, *out)
        if op == "tr":
            return lib.fs_conv3d_tr(x.data_ptr(), w.data_ptr(), bias.data_ptr(), bufs["y"].ptr(), bufs["ws"].ptr(), *geo,
                                    _stream())
        if op == "tr_add":
            return lib.fs_conv3d_tr_add(x.data_ptr(), w.data_ptr(), bias.data_ptr(), add.data_ptr(), bufs["y"].ptr(),
                                        bufs["ws"].ptr(), *geo, _stream())
        return lib.fs_conv3d_tr_prelu(x.data_ptr(), w.data_ptr(), bias.data_ptr(), a.data_ptr(), bufs["y"].ptr(),
                                      bufs["z"].ptr(), bufs["ws"].ptr(), *geo, a.numel(), _stream())
    geo = (B, cin, cout, *inp, *out, k, s, p)
    if op == "fwd":
        return lib.fs_conv3d_fwd(x.data_ptr(), w.data_ptr(), bias.data_ptr(), bufs["y"].ptr(), bufs["ws"].ptr(), *geo,
                                 r["wmode"], _stream())
    if op == "fwd_add":
        return lib.fs_conv3d_fwd_add(x.data_ptr(), w.data_ptr(), bias.data_ptr(), add.data_ptr(), bufs["y"].ptr(),
                                     bufs["ws"].ptr(), *geo, r["wmode"], _stream())
    if op == "fwd_prelu":
        return lib.fs_conv3d_fwd_prelu(x.data_ptr(), w.data_ptr(), bias.data_ptr(), a.data_ptr(), add.data_ptr(),
                                       bufs["y"].ptr(), bufs["z"].ptr(), bufs["ws"].ptr(), *geo, a.numel(), _stream())
    if op == "fwd_ms":
        planes = D["planes"]
        ptrs = (ctypes.c_void_p * cin)(*[pl.data_ptr() for pl in planes])
        strides = (ctypes.c_longlong * cin)(*[pl.stride(0) for pl in planes])
        return lib.fs_conv3d_fwd_prelu_ms(ptrs, strides, w.data_ptr(), bias.data_ptr(), a.data_ptr(), bufs["y"].ptr(),
                                          bufs["z"].ptr(), bufs["ws"].ptr(), *geo, a.numel(), _stream())
    assert op == "fwd_dprelu"
    return lib.fs_conv3d_fwd_dprelu(x.data_ptr(), w.data_ptr(), act.data_ptr(), a.data_ptr(), a.numel(), bufs["y"].ptr(),
                                    bufs["ga"].ptr(), bufs["gb"].ptr(), bufs["part"].ptr(), bufs["ws"].ptr(), *geo,
                                    _stream())


def _planes(t):
    """Channel c of `t` as a plane of its own tensor (one spare channel: batch stride != the plane's volume)."""
    out = []
    for c in range(t.shape[1]):
        host = torch.cat([t[:, c:c + 1], torch.zeros_like(t[:, :1])], dim=1)
        out.append(host.to(DEV)[:, 0])
    return out


def _buffers(lib, r, D):
    op, B, cin, cout, k = r["op"], r["B"], r["cin"], r["cout"], r["k"]
    ny = B * cout * math.prod(r["out"])
    bufs = {}
    if op.startswith("wrw"):
        bufs["dw"] = Guarded(cout * cin * k ** 3, zero=op != "wrw_det")
        if op == "wrw_det":
            n = lib.fs_conv3d_wrw_det_ws_floats(D["g_dev"].data_ptr(), D["src_dev"].data_ptr(), None, None, B, cout, cin,
                                                *r["out"], *r["inp"], k, r["stride"], r["pad"])
            assert n > 0, n
            bufs["ws"] = Guarded(n)
        return bufs
    bufs["y"] = Guarded(ny)
    if op in ("fwd_prelu", "fwd_ms", "tr_prelu"):
        bufs["z"] = Guarded(ny)
    if op.startswith("tr"):
        n = lib.fs_conv3d_tr_ws_floats(cin, cout)
    else:
        n = lib.fs_conv3d_fwd_ws_floats(cin, cout, k)
    assert n >= 0, n
    bufs["ws"] = Guarded(n)
    if op == "fwd_dprelu":
        part = lib.fs_conv3d_fwd_dprelu_part_floats if k == 4 else lib.fs_conv3d_fwd_dprelu_part_floats_k3
        n = part(B, cout, *r["out"])
        assert n > 0, n
        bufs["part"] = Guarded(n)
        bufs["ga"] = Guarded(1)
        bufs["gb"] = Guarded(cout)
    return bufs


def _to_device(r, D):
    for name in list(D):
        mis = r["mis"] if name in ("x", "g") else (r["mis2"] if name == "src" else 0)
        D[name + "_dev"] = on_device(D[name], mis)
    if r["op"] in ("fwd_ms", "wrw_ms"):
        D["planes"] = _planes(D["x" if r["op"] == "fwd_ms" else "src"])


def _results(r, bufs, ref):
    op, B, cout = r["op"], r["B"], r["cout"]
    got = {}
    if op.startswith("wrw"):
        got["dw"] = bufs["dw"].view(ref["dw"].shape)
        return got
    got["y"] = bufs["y"].view(ref["y"].shape)
    if "z" in ref:
        got["z"] = bufs["z"].view(ref["z"].shape)
    if op == "fwd_dprelu":
        got["ga"], got["gb"] = bufs["ga"].t, bufs["gb"].t
    return got


def _errors(ref, got):
    errs = {}
    for name, g in got.items():
        rf = ref[name]
        diff = float((g.detach().cpu().double() - rf).abs().max())
        if name in ("ga", "gb"):  # sums over every position: the band also scales with the sum of |terms|
            scale = float(rf.abs().max()) + 0.05 * float(ref["_" + name + "_abs"].max())
        else:
            scale = float(rf.abs().max())
        errs[name] = diff / max(scale, 1e-30)
    return errs


@pytest.mark.parametrize("r", LG.ROWS, ids=[LG.row_id(r) for r in LG.ROWS])
def test_ledger_row(lib, r):
    t0 = time.perf_counter()
    D = _data(r)
    _to_device(r, D)
    bufs = _buffers(lib, r, D)
    rc, launched = _conv_kernels_launched(lambda: _call(lib, r, D, bufs))
    assert rc == 0, "status %d" % rc
    compute = [n for n in launched if n not in LG.HELPERS]
    assert r["kernel"] in compute, "expected %s, launched %s" % (r["kernel"], launched)
    assert set(compute) == {r["kernel"]}, "other convolution kernels ran: %s" % launched
    ref = _reference(r, D)
    got = _results(r, bufs, ref)
    errs = _errors(ref, got)
    snap = {name: g.detach().clone() for name, g in got.items()}
    rep_ok = True
    if r["op"] == "wrw_det":  # same bits again, and the atomic form within the band
        bufs2 = _buffers(lib, r, D)
        assert _call(lib, r, D, bufs2) == 0
        torch.cuda.synchronize()
        rep_ok = torch.equal(bufs2["dw"].t.view(torch.int32), bufs["dw"].t.view(torch.int32))
        atomic = dict(bufs2, dw=Guarded(bufs["dw"].n, zero=True))
        assert _call(lib, dict(r, op="wrw"), D, atomic) == 0
        torch.cuda.synchronize()
        errs["atomic"] = _rel(snap["dw"].view(-1), atomic["dw"].t.cpu().double())
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    print("LEDGER %-48s %-10s err %s  %.2fs" % (r["kernel"], r["op"],
                                                " ".join("%s=%.2e" % kv for kv in sorted(errs.items())), dt))
    bad_guard = [name for name, b in bufs.items() if not b.intact()]
    assert not bad_guard, "writes outside %s" % bad_guard
    assert rep_ok, "deterministic weight gradient differs between two runs"
    assert all(e <= TOL for e in errs.values()), errs


# ---- misaligned outputs are refused -----------------------------------------------------------------------------------
def _refusal_cases():
    # (name, row of the ledger, pointer to misalign)
    pick = {}
    for r in LG.ROWS:
        if r["op"] in ("fwd", "fwd_add", "fwd_prelu", "fwd_dprelu", "tr", "tr_add", "tr_prelu") and r["mis"] == 0:
            key = (r["op"], r["k"])
            if key not in pick or math.prod(r["out"]) * r["B"] * r["cout"] < math.prod(pick[key]["out"]) * pick[key]["B"] * pick[key]["cout"]:
                pick[key] = r
    cases = []
    for (op, k), r in sorted(pick.items()):
        for which in ("y", "z", "addend", "act_y"):
            if which == "z" and op not in ("fwd_prelu", "tr_prelu"):
                continue
            if which == "addend" and op not in ("fwd_add", "fwd_prelu", "tr_add"):
                continue
            if which == "act_y" and op != "fwd_dprelu":
                continue
            cases.append((op, k, which, r))
    return cases


@pytest.mark.parametrize("case", _refusal_cases(), ids=lambda c: "%s-k%d-%s" % c[:3])
def test_misaligned_output_is_refused(lib, case):
    op, k, which, r = case
    D = _data(r)
    _to_device(r, D)
    bufs = _buffers(lib, r, D)
    shift = {}
    if which in ("y", "z"):
        # the same number of floats, starting 4 bytes past the 16-byte boundary (room: the guard band)
        shift[which] = 1
    else:
        D[which + "_dev"] = on_device(D[which], 1)

    class Shifted:
        def __init__(self, g, off):
            self.g, self.off = g, off

        def ptr(self, offset=0):
            return self.g.ptr(self.off + offset)

    call_bufs = {name: (Shifted(b, shift[name]) if name in shift else b) for name, b in bufs.items()}
    rc, launched = _conv_kernels_launched(lambda: _call(lib, r, D, call_bufs))
    assert rc == FS_ERR_ARG, rc
    assert launched == [], launched
    for name, b in bufs.items():
        assert b.untouched(), "%s was written" % name
