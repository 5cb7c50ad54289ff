"""Inputs, fp64 references, fp32 oracles, exact expectations and bands of the rows of tests/corr_ledger.py (CPU tensors only;
shared by tests/test_corr_ledger.py and tests/test_gpu_corr_ledger.py).

References: the header's formulas restated in float64 on the fp32 input values.
  correlation   out[b, d, p] = (1 / C) sum_c n1[b, c, p] n2[b, c, p + d], n2 read as 0 outside the image / volume (the zero
                padding applies AFTER the normalisation n = (f - mean) * rstd); means are sum / C; gradients w.r.t. n1, n2
                by float64 autograd through that restatement.  The (mean, rstd) tables of the normalised forms are INPUTS
                of those rows -- the float64 moments rounded to fp32 -- so a defect of the moment kernels fails their rows,
                not these.
  moments       mean = sum f / S, rstd = (sum (f - mean)^2 / (S - 1) + 1e-16)^-1/2
  adjoint       grad_f = r (g - mean(g) - n sum(g n) / (S - 1)), n = (f - m) r, (m, r) the given table
  chain rows    float64 autograd through oracle.corr.corr2d_normalized_ref, the four tensors as independent leaves.
The fp32 oracle is the same code in float32 (correlation, chain) or the kernels' own arithmetic restated (moments and
adjoint: float64 accumulation of fp32 terms, fp32 elsewhere; integer rows: the exact sum, then one fp32 division).

Bands, at every element, are rounding bounds of the fp32 arithmetic with u = 2^-24, not numbers fitted to a device run:
  correlation   (n + 4) u A: n = number of terms (C forward; (2 md + 1)^2 backward, times the number of displacement planes
                inside the volume in 3-D), A = the same sum on absolute values in float64, divided by C; n + 8 with the
                normalisation folded in (two more roundings per operand); never wider than the project's older absolute
                bands (1e-5 forward, 5e-5 2-D backward, 1e-4 3-D backward).  A == 0 (every term has a factor that is exactly
                0: displacement planes outside the volume, constant planes, pixels whose whole window is padding): the
                output must be exactly 0.  Rows of kind "int" hold small integers in every operand: every partial sum is an
                integer below 2^24 in any order, so the band is 0 everywhere and the output must be fl(sum / C) bitwise
                (which a product with fl(1 / C) is not when C is no power of two).
  moments       mean 2 u |ref| (exactly the constant on a constant plane), rstd 8 u |ref|
  adjoint       8 u r (|g| + |mean g| + |n| |s2|), s2 = sum(g n) / (S - 1).  (s2 is a cancelling sum of fp32 products, so
                this is no worst-case bound; the kernel's own arithmetic restated in fp32 stays below 0.8 of it on every
                row, tests/test_corr_ledger.py.)
  chain rows    the bands of test_corr2d_normalized_golden_and_oracle: 2e-5 max|ref| forward, 1e-4 max|ref| gradients.

Poison rows (one NaN, or a whole NaN sample next to a finite one): the output's non-finite set must equal the reference's,
everything else is held to the band.  Whether NaN times a padding zero is NaN is not part of the ABI -- the direct kernels
skip the terms whose displacement leaves the image, the tiled kernels multiply by the zero -- so no row asks: NaNs in f2
are unambiguous (every term that reads one is inside the image), a single NaN of grad_out sits on the centre displacement
(inside the image at every pixel), whole NaN samples of f1 or grad_out go to the tiled kernels, whose arithmetic is the
reference's, and the one NaN of grad_out
whose target lies outside the image ("edge") is judged through grad_f2 alone, which must not see it.

Worst error over band per entry point on an MI355X (tests/test_gpu_corr_ledger.py, the LEDGER lines):
  fs_corr2d_fwd          0.413 (out; 83 rows)
  fs_corr2d_bwd          0.202 (g2; 42 rows)
  fs_corr2d_norm_fwd     0.404 (out; 24 rows)
  fs_corr2d_norm_bwd     0.134 (g1; 12 rows)
  fs_corr2d_pair_fwd     0.300 (outa; 17 rows)
  fs_corr2d_pair_bwd     0.082 (g2b; 21 rows)
  fs_plane_moments       0.449 (mean; 22 rows)
  fs_plane_moments4      0.439 (mean; 5 rows)
  fs_plane_norm_bwd      0.619 (gf; 22 rows)
  fs_plane_norm_bwd4     0.796 (gfb; 10 rows)
  fs_corr3d_fwd          0.403 (out; 21 rows)
  fs_corr3d_bwd          0.330 (g2; 22 rows)
  chain rows             0.291 (rstd; 4 rows)
"""
import torch
import torch.nn.functional as F

import corr_ledger as L
from oracle import corr as ocorr

U = 2.0 ** -24
ABS_FWD, ABS_BWD2, ABS_BWD3 = 1e-5, 5e-5, 1e-4
CHAIN_FWD, CHAIN_BWD = 2e-5, 1e-4
CONST = 0.75
ALIAS = {"f1b": "f2a", "f2b": "f1a", "fb": "fa", "fc": "fa", "fd": "fa"}
PAIR = (("f1a", "f2a", "outa", "gouta", "g1a", "g2a", 0), ("f1b", "f2b", "outb", "goutb", "g1b", "g2b", 2))
MOMENT_OPS = ("mom", "mom4", "nb", "nb4")


def gen_of(r):
    return torch.Generator().manual_seed(sum((i + 1) * ord(c) for i, c in enumerate(L.row_id(r))) % 1000003)


def shape5(r):
    return (r["B"], r["C"], r["D"], r["H"], r["W"])


def nz_of(r):
    return 2 * r["md"] + 1 if r["op"].startswith("c3_") else 1


def nd_of(r):
    return 2 * r["md"] + 1


def out_shape(r):
    return (r["B"], nz_of(r) * nd_of(r) ** 2, r["D"], r["H"], r["W"])


def operand(T, name, r):
    """The tensor behind an argument name: aliased arguments share their target's."""
    if r["alias"] and name in ALIAS:
        return T[ALIAS[name]]
    return T[name]


def moments(f, dt=torch.float64):
    """[planes, 2] (mean, rstd) of f [planes, S]."""
    f = f.to(dt)
    S = f.shape[1]
    mean = f.sum(1) / S
    var = ((f - mean[:, None]) ** 2).sum(1) / (S - 1)
    return torch.stack([mean, 1.0 / torch.sqrt(var + 1e-16)], 1)


def table(f):
    """The (mean, rstd) table of a feature tensor as an input: the float64 moments rounded to fp32."""
    return moments(f.reshape(f.shape[0] * f.shape[1], -1)).float()


def _features(r, g, shape):
    if r["kind"] == "int":
        return torch.randint(-3, 4, shape, generator=g).float()
    f = 0.3 + torch.randn(shape, generator=g)
    if r["kind"] == "const":
        f[:, -1] = CONST
    return f


def data(r):
    """{operand name: fp32 CPU tensor} -- every input of the row's call (aliased operands once, under their target's name)."""
    g, op = gen_of(r), r["op"]
    T = {}
    if op in MOMENT_OPS:
        names = ("f",) if op in ("mom", "nb") else (("fa",) if op == "mom4" and r["alias"] else ("fa", "fb", "fc", "fd"))
        for k, name in enumerate(names):
            f = torch.randn(r["planes"], r["S"], generator=g) * (1.0 + 0.5 * k) + 0.3 * (k + 1)
            if r["kind"] == "offset":
                f = f - f.mean(1, keepdim=True) + 100.0 * f.std(1, keepdim=True)
            if r["kind"] == "const":
                f = CONST * (1 + torch.arange(r["planes"], dtype=torch.float32))[:, None].expand(-1, r["S"]).contiguous()
            T[name] = f
        if op in ("nb", "nb4"):
            T["stats"] = torch.stack([moments(T[n]).float() for n in names]).reshape(-1, 2)
            for name in names:
                T["gn" + name[1:]] = torch.randn(r["planes"], r["S"], generator=g)
        return T
    sh = shape5(r)
    if op in ("p_fwd", "p_bwd", "chain"):
        for name in (("f1a", "f2a") if r["alias"] else ("f1a", "f2a", "f1b", "f2b")):
            T[name] = _features(r, g, sh)
        if r["stats"] and op != "chain":
            T["stats"] = torch.stack([table(operand(T, n, r)) for n in ("f1a", "f2a", "f1b", "f2b")])
        if op != "p_fwd":
            T["gouta"], T["goutb"] = torch.randn(out_shape(r), generator=g), torch.randn(out_shape(r), generator=g)
        return T
    T["f1"], T["f2"] = _features(r, g, sh), _features(r, g, sh)
    if op.startswith("n_"):
        T["st1"], T["st2"] = table(T["f1"]), table(T["f2"])
    if op.endswith("_bwd"):
        T["gout"] = _features(r, g, out_shape(r)) if r["kind"] == "int" else torch.randn(out_shape(r), generator=g)
    if r["poison"]:
        name, how = r["poison"]
        if how == "sample":
            T[name][-1] = float("nan")
        elif how == "edge":
            T[name][0, T[name].shape[1] // 2 + r["md"], r["D"] // 2, r["H"] // 2, r["W"] - 1] = float("nan")
        elif name == "gout":
            T[name][0, T[name].shape[1] // 2, r["D"] // 2, r["H"] // 2, r["W"] // 2] = float("nan")
        else:
            T[name][0, -1, r["D"] // 2, r["H"] // 2, r["W"] // 2] = float("nan")
    return T


def out_sizes(r):
    """{output name: floats} of every output the entry point has (the test passes NULL for those not in r['grads'])."""
    op = r["op"]
    n = r["B"] * r["C"] * r["D"] * r["H"] * r["W"]
    no = 1
    for k in out_shape(r):
        no *= k
    ps = r["planes"] * r["S"]
    if op in ("c2_fwd", "n_fwd", "c3_fwd"):
        return dict(out=no)
    if op in ("c2_bwd", "n_bwd", "c3_bwd"):
        return dict(g1=n, g2=n)
    if op == "p_fwd":
        return dict(outa=no, outb=no)
    if op == "p_bwd":
        return dict(g1a=n, g2a=n, g1b=n, g2b=n)
    if op == "mom":
        return dict(stats=2 * r["planes"])
    if op == "mom4":
        return dict(stats=8 * r["planes"])
    if op == "nb":
        return dict(gf=ps)
    if op == "nb4":
        return dict(gfa=ps, gfb=ps, gfc=ps, gfd=ps)
    assert op == "chain"
    return dict(stats=8 * r["B"] * r["C"], outa=no, outb=no, g1a=n, g2a=n, g1b=n, g2b=n, gfa=n, gfb=n, gfc=n, gfd=n)


def requested(r):
    """The outputs the row's call is given (the others are NULL)."""
    return tuple(r["grads"]) if r["op"] in L.GRADS_OF else tuple(out_sizes(r))


# ---- the operations, dtype-generic ----------------------------------------------------------------------------------------
def normalised(f, st, dt):
    f = f.to(dt)
    if st is None:
        return f
    B, C = f.shape[:2]
    st = st.to(dt).view(B, C, 2, 1, 1, 1)
    return (f - st[:, :, 0]) * st[:, :, 1]


def corr(n1, n2, md, nz):
    """[B, nz (2md+1)^2, D, H, W]: the cost volume of n1, n2 [B, C, D, H, W], dz-major then dy, dx; sum / C."""
    B, C, D, H, W = n1.shape
    nd, pz = 2 * md + 1, (md if nz > 1 else 0)
    p = F.pad(n2, (md, md, md, md, pz, pz))
    outs = []
    for dz in range(nz):
        for dy in range(nd):
            for dx in range(nd):
                outs.append((n1 * p[:, :, dz:dz + D, dy:dy + H, dx:dx + W]).sum(1) / C)
    return torch.stack(outs, 1)


def corr_all(r, f1, f2, st1, st2, gout, dt, absolute=False):
    """(out,) forward or (g1, g2) backward of one set, in `dt`; `absolute`: the same sums on absolute values."""
    n1, n2 = normalised(f1, st1, dt), normalised(f2, st2, dt)
    if absolute:
        n1, n2 = n1.abs(), n2.abs()
    if gout is None:
        return (corr(n1, n2, r["md"], nz_of(r)),)
    G = gout.to(dt).abs() if absolute else gout.to(dt)
    n1, n2 = n1.detach().requires_grad_(), n2.detach().requires_grad_()
    return torch.autograd.grad((corr(n1, n2, r["md"], nz_of(r)) * G).sum(), [n1, n2])


def terms(r, bwd):
    """Number of terms of each output element's sum, broadcastable over [B, ., D, H, W]."""
    if not bwd:
        return torch.full((1, 1, 1, 1, 1), float(r["C"]), dtype=torch.float64)
    md, D = r["md"], r["D"]
    planes = [sum(1 for dz in range(-md, md + 1) if 0 <= z + dz < D) if nz_of(r) > 1 else 1 for z in range(D)]
    return (nd_of(r) ** 2 * torch.tensor(planes, dtype=torch.float64)).view(1, 1, D, 1, 1)


def corr_band(r, A, bwd, normed):
    if r["kind"] == "int":  # exact sums: the output is the correctly rounded quotient
        return torch.zeros_like(A)
    cap = ABS_FWD if not bwd else (ABS_BWD3 if nz_of(r) > 1 else ABS_BWD2)
    return torch.clamp((terms(r, bwd) + (8 if normed else 4)) * U * A, max=cap)


def _sets(r, T):
    """(f1, f2, st1, st2, gout, output names) of each correlation set of the row."""
    op = r["op"]
    if op in ("p_fwd", "p_bwd"):
        out = []
        for f1, f2, o, go, g1, g2, k in PAIR:
            st = T.get("stats")
            out.append((operand(T, f1, r), operand(T, f2, r), None if st is None else st[k], None if st is None else st[k + 1],
                        T.get(go), (o,) if op == "p_fwd" else (g1, g2)))
        return out
    return [(T["f1"], T["f2"], T.get("st1"), T.get("st2"), T.get("gout"), ("out",) if op.endswith("fwd") else ("g1", "g2"))]


def _adjoint(f, st, gn, dt):
    """(grad_f, band) of the moment adjoint on [planes, S]; the band in float64 only."""
    f, gn, m, rs = f.to(dt), gn.to(dt), st[:, 0:1].to(dt), st[:, 1:2].to(dt)
    S = f.shape[1]
    n = (f - m) * rs
    s1, s2 = gn.sum(1, keepdim=True) / S, (gn * n).sum(1, keepdim=True) / (S - 1)
    band = 8 * U * rs * (gn.abs() + s1.abs() + n.abs() * s2.abs())
    return rs * (gn - s1 - n * s2), band


def _adjoint_as_the_kernel(f, st, gn):
    """plane_norm_bwd_kernel's arithmetic: float64 accumulation of fp32 terms, fp32 elsewhere."""
    m, rs = st[:, 0:1], st[:, 1:2]
    S = f.shape[1]
    n = (f - m) * rs
    s1 = (gn.double().sum(1, keepdim=True) / S).float()
    s2 = ((gn * n).double().sum(1, keepdim=True) / (S - 1)).float()
    return rs * (gn - s1 - n * s2)


def _moments_as_the_kernel(f):
    """plane_moments_kernel's arithmetic: float64 sums of fp32 terms, the deviations from the fp32-rounded mean."""
    S = f.shape[1]
    mean = (f.double().sum(1) / S).float()
    d = f - mean[:, None]
    var = ((d * d).double().sum(1) / (S - 1)).float()
    return torch.stack([mean, 1.0 / torch.sqrt(var + torch.tensor(1e-16, dtype=torch.float32))], 1)


def _chain(r, T, dt):
    leaves = [operand(T, n, r).to(dt).clone().requires_grad_() for n in ("f1a", "f2a", "f1b", "f2b")]
    sq = [t.squeeze(2) for t in leaves]
    ra, rb = ocorr.corr2d_normalized_ref(sq[0], sq[1], r["md"]), ocorr.corr2d_normalized_ref(sq[2], sq[3], r["md"])
    Ga, Gb = T["gouta"].to(dt).squeeze(2), T["goutb"].to(dt).squeeze(2)
    gs = torch.autograd.grad((ra * Ga).sum() + (rb * Gb).sum(), leaves)
    res = dict(outa=ra.detach().unsqueeze(2), outb=rb.detach().unsqueeze(2))
    res.update(zip(("gfa", "gfb", "gfc", "gfd"), gs))
    return res


def results(r, T):
    """{name: (float64 reference, float64 band per element)}; band == 0: the value must be exactly the reference's."""
    op = r["op"]
    if op in ("mom", "mom4"):
        names = ("f",) if op == "mom" else ("fa", "fb", "fc", "fd")
        st = torch.stack([moments(operand(T, n, r)) for n in names])  # [k, planes, 2]
        mean, rstd = st[..., 0], st[..., 1]
        return dict(mean=(mean, torch.zeros_like(mean) if r["kind"] == "const" else 2 * U * mean.abs()),
                    rstd=(rstd, 8 * U * rstd.abs()))
    if op in ("nb", "nb4"):
        names = ("",) if op == "nb" else ("a", "b", "c", "d")
        st = T["stats"].view(len(names), r["planes"], 2)
        return {"gf" + s: _adjoint(T["f" + s], st[k], T["gn" + s], torch.float64) for k, s in enumerate(names)}
    if op == "chain":
        ref = _chain(r, T, torch.float64)
        out = {k: (v, torch.full_like(v, (CHAIN_FWD if k.startswith("out") else CHAIN_BWD) * float(v.abs().max())))
               for k, v in ref.items()}
        st = torch.stack([table(operand(T, n, r)).double() for n in ("f1a", "f2a", "f1b", "f2b")])
        out["mean"], out["rstd"] = (st[..., 0], 2 * U * st[..., 0].abs()), (st[..., 1], 8 * U * st[..., 1].abs())
        return out
    res = {}
    for f1, f2, st1, st2, gout, names in _sets(r, T):
        ref = corr_all(r, f1, f2, st1, st2, gout, torch.float64)
        A = corr_all(r, f1, f2, st1, st2, gout, torch.float64, absolute=True)
        for name, v, a in zip(names, ref, A):
            if r["kind"] == "int":  # the integer sum over C, free of the reference's own float64 roundings
                v = (v * r["C"]).round() / r["C"]
            res[name] = (v, corr_band(r, a, gout is not None, st1 is not None))
    return res


def oracle(r, T):
    """{name: fp32 result} of the fp32 oracle."""
    op = r["op"]
    if op in ("mom", "mom4"):
        names = ("f",) if op == "mom" else ("fa", "fb", "fc", "fd")
        st = torch.stack([_moments_as_the_kernel(operand(T, n, r)) for n in names])
        return dict(mean=st[..., 0], rstd=st[..., 1])
    if op in ("nb", "nb4"):
        names = ("",) if op == "nb" else ("a", "b", "c", "d")
        st = T["stats"].view(len(names), r["planes"], 2)
        return {"gf" + s: _adjoint_as_the_kernel(T["f" + s], st[k], T["gn" + s]) for k, s in enumerate(names)}
    if op == "chain":
        res = _chain(r, T, torch.float32)
        st = torch.stack([_moments_as_the_kernel(operand(T, n, r).reshape(r["B"] * r["C"], -1)) for n in ("f1a", "f2a", "f1b", "f2b")])
        res["mean"], res["rstd"] = st[..., 0], st[..., 1]
        return res
    res = {}
    for f1, f2, st1, st2, gout, names in _sets(r, T):
        if r["kind"] == "int":  # the kernels' arithmetic: the exact integer sum, then one fp32 division
            sums = [(v * r["C"]).round().float() + 0.0 for v in corr_all(r, f1, f2, st1, st2, gout, torch.float64)]
            res.update(zip(names, [v / torch.tensor(float(r["C"])) for v in sums]))
        else:
            res.update(zip(names, corr_all(r, f1, f2, st1, st2, gout, torch.float32)))
    return res


def compare(got, ref, band, poison=False):
    """(worst |got - ref| / band over the elements with a band, number of elements that miss an exact expectation, whether
    the non-finite sets agree) of one fp32 output against its float64 reference.  Without `poison` a non-finite element of
    either is an infinite error."""
    got, ref, band = got.reshape(-1), ref.reshape(-1), band.expand_as(ref).reshape(-1)
    bad_g, bad_r = ~torch.isfinite(got), ~torch.isfinite(ref)
    same_set = bool(torch.equal(bad_g, bad_r))
    if not poison and bool((bad_g | bad_r).any()):
        return float("inf"), 0, same_set
    ok = ~(bad_g | bad_r)
    got, ref, band = got[ok], ref[ok], band[ok]
    ex = band == 0
    inexact = int((got[ex].view(torch.int32) != (ref[ex] + 0.0).float().view(torch.int32)).sum())  # (+ 0.0: no -0.0)
    d = (got[~ex].double() - ref[~ex]).abs() / band[~ex]
    return (float(d.max()) if d.numel() else 0.0), inexact, same_set
