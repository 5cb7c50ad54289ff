"""GPU (-m gpu): the split-bf16 body of convtr_p8_kernel (<= 32 input channels, <= 3 row tiles; csrc/convtr.hip) through
the C-ABI, as the ledger test calls it (fs_conv3d_tr, fs_conv3d_tr_add).

Per shape: seeded normal inputs, and the same with input channel c scaled by 2^e(c) and its weights by 2^-e(c), e spread
over -20 .. 20 (exact scalings: the piece split sees the whole exponent range, the reference stays the same); with and
without addend, with and without bias.  Every launch works on FRESH buffers and is the first work that touches them, and
is repeated: the two outputs must agree bit for bit (no atomics) and both must match the fp64 CPU reference within the
ledger's band, error = max |y - ref| / max |ref|.  Outputs and workspace sit inside NaN guard bands that must stay intact.
Where the ablation build is available the same cases run in a fresh process on its fp32 body (FLOWSCI_TR_P8_NO_S3=1):
the split body's error is at most 1.5 x that (the round-5 gate).

As a script (`python tests/test_gpu_tr_p8_s3.py`): prints one `CASE <shape> <kind> <variant> err=<e>` line per launch
pair for whatever library FLOWSCI_HIP_LIBRARY selects."""
import math
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(1, ROOT)
from ledger_harness import Guarded, load_lib, on_device, stream as _stream  # noqa: E402

pytestmark = pytest.mark.gpu

TOL = 2e-5  # tests/test_gpu_conv_ledger.py
# (B, Cin, Cout, input extent): instantiation / what it covers
SHAPES = [
    (1, 32, 6, (6, 6, 64)),    # <3, 5, 32>
    (1, 8, 5, (6, 6, 128)),    # <3, 9, 32>
    (1, 8, 1, (6, 6, 64)),     # <1, 5, 32>
    (1, 8, 2, (6, 6, 128)),    # <1, 9, 32>
    (1, 5, 6, (6, 6, 128)),    # Cin % 4 != 0: channels past Cin read as zero
    (1, 32, 6, (6, 6, 132)),   # two x bricks, the second partial, and the q = Wi column
    (1, 8, 1, (34, 34, 64)),   # 324 bricks > 256 workgroups: the loader stream crosses a brick boundary
]
KINDS = ("normal", "scaled")
VARIANTS = ((False, False), (False, True), (True, False), (True, True))  # (addend, bias)


def _sid(s):
    return "b%d_ci%d_co%d_%dx%dx%d" % (s[0], s[1], s[2], *s[3])


_cache = {}


def _case(shape):
    """Host data and the fp64 reference of a shape, computed once."""
    if shape not in _cache:
        B, cin, cout, inp = shape
        gen = torch.Generator().manual_seed(1300 + sum(map(ord, _sid(shape))))
        x = torch.randn(B, cin, *inp, generator=gen)
        w = torch.randn(cin, cout, 4, 4, 4, generator=gen) / math.sqrt(cin * 8)
        bias = torch.randn(cout, generator=gen)
        addend = torch.randn(B, cout, *(2 * i for i in inp), generator=gen)
        e = torch.tensor([-20 + (40 * c) // max(cin - 1, 1) for c in range(cin)], dtype=torch.float32)
        sc = torch.pow(2.0, e)
        xs, ws = x * sc.view(1, -1, 1, 1, 1), w / sc.view(-1, 1, 1, 1, 1)  # exact
        conv = F.conv_transpose3d(x.double(), w.double(), stride=2, padding=1)
        _cache[shape] = {"normal": (x, w), "scaled": (xs, ws), "bias": bias, "addend": addend, "conv": conv}
    return _cache[shape]


def _launch_pair(lib, shape, kind, with_add, with_bias):
    """Two launches, each on fresh buffers it is the first to touch: (error of each against fp64, bit-equal, guards)."""
    B, cin, cout, inp = shape
    out = tuple(2 * i for i in inp)
    C = _case(shape)
    ref = C["conv"].clone()
    if with_bias:
        ref += C["bias"].double().view(1, -1, 1, 1, 1)
    if with_add:
        ref += C["addend"].double()
    scale = float(ref.abs().max())
    got, errs, guards = [], [], True
    for _ in range(2):
        x, w = (on_device(t) for t in C[kind])
        bias = on_device(C["bias"]) if with_bias else None
        add = on_device(C["addend"]) if with_add else None
        y = Guarded(B * cout * math.prod(out))
        n = lib.fs_conv3d_tr_ws_floats(cin, cout)
        assert n > 0, n
        ws = Guarded(n)
        geo = (B, cin, cout, *inp, *out)
        bp = bias.data_ptr() if with_bias else None
        if with_add:
            rc = lib.fs_conv3d_tr_add(x.data_ptr(), w.data_ptr(), bp, add.data_ptr(), y.ptr(), ws.ptr(), *geo, _stream())
        else:
            rc = lib.fs_conv3d_tr(x.data_ptr(), w.data_ptr(), bp, y.ptr(), ws.ptr(), *geo, _stream())
        assert rc == 0, "status %d" % rc
        torch.cuda.synchronize()
        g = y.view(ref.shape).detach().cpu()
        got.append(g)
        errs.append(float((g.double() - ref).abs().max()) / scale)  # (a NaN left in the output gives NaN: fails the band)
        guards = guards and y.intact() and ws.intact()
    same = torch.equal(got[0].view(torch.int32), got[1].view(torch.int32))
    return errs, same, guards


def _vid(with_add, with_bias):
    return ("add" if with_add else "noadd") + "_" + ("bias" if with_bias else "nobias")


def _all_cases(lib, shape):
    for kind in KINDS:
        for with_add, with_bias in VARIANTS:
            yield kind, _vid(with_add, with_bias), _launch_pair(lib, shape, kind, with_add, with_bias)


@pytest.fixture(scope="module")
def lib():
    return load_lib()


@pytest.fixture(scope="module")
def product_errors():
    return {}


@pytest.mark.parametrize("shape", SHAPES, ids=_sid)
def test_split_body_against_fp64(lib, shape, product_errors):
    bad = []
    for kind, vid, (errs, same, guards) in _all_cases(lib, shape):
        print("P8S3 %-24s %-6s %-12s err %.3e %.3e" % (_sid(shape), kind, vid, errs[0], errs[1]))
        product_errors[(_sid(shape), kind, vid)] = max(errs)
        if not guards:
            bad.append((kind, vid, "writes outside the output or the workspace"))
        if not same:
            bad.append((kind, vid, "two launches on fresh buffers differ", errs))
        if not all(e <= TOL for e in errs):  # (NaN fails)
            bad.append((kind, vid, "outside the band", errs))
    assert not bad, bad


@pytest.fixture(scope="module")
def fp32_errors(ablation_lib):
    """The same cases on the fp32 body of the ablation build, in a fresh process (the switch is read once per process)."""
    env = {k: v for k, v in os.environ.items() if not k.startswith("FLOWSCI_")}
    env.update(FLOWSCI_HIP_LIBRARY=ablation_lib, FLOWSCI_TR_P8_NO_S3="1")
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "DONE" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    out = {}
    for line in r.stdout.splitlines():
        f = line.split()
        if f and f[0] == "CASE":
            out[(f[1], f[2], f[3])] = float(f[4].split("=", 1)[1])
    return out


@pytest.mark.parametrize("shape", SHAPES, ids=_sid)
def test_error_at_most_1p5_of_the_fp32_body(lib, shape, product_errors, fp32_errors):
    bad = []
    for kind in KINDS:
        for with_add, with_bias in VARIANTS:
            key = (_sid(shape), kind, _vid(with_add, with_bias))
            if key not in product_errors:
                product_errors[key] = max(_launch_pair(lib, shape, kind, with_add, with_bias)[0])
            s3, fp = product_errors[key], fp32_errors[key]
            print("P8S3 %-24s %-6s %-12s split %.3e fp32 %.3e" % (*key, s3, fp))
            if not s3 <= 1.5 * fp:
                bad.append((key, s3, fp))
    assert not bad, bad


if __name__ == "__main__":
    from opticalflowscivis_amd import _lib
    L = _lib.lib()
    for shape_ in SHAPES:
        for kind_, vid_, (errs_, same_, guards_) in _all_cases(L, shape_):
            print("CASE %s %s %s err=%.6e same=%d guards=%d" % (_sid(shape_), kind_, vid_, max(errs_), same_, guards_), flush=True)
    print("DONE")
