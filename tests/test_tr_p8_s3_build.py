"""CPU (needs hipcc): what the split-bf16 body of convtr_p8_kernel (csrc/convtr.hip, round 13) needs from the build.

* every convtr_p8_kernel instantiation of the product build compiles without scratch and inside the 256 registers of
  launch_bounds(512, 2), with its LDS inside a CU's 160 KB;
* fs_conv3d_tr_ws_floats covers the pre-split weight table of the heads;
* the FS_WPREP_P8 word layout of the split table, computed on the host by the library's own element function
  (tests/tools/p8s_words.hip includes csrc/wprep.hpp), against entries worked out by hand from the transposed convolution:
  output o = 2 i - 1 + k, so position q's output 2 q - p reads input q - d through kernel index k = 2 d - p + 1."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_build_resources import CSRC, HIPCC, ROOT, _resource_usage  # noqa: E402

INSTANTIATIONS = [(1, 9, 32), (1, 5, 32), (3, 9, 32), (3, 5, 32), (1, 9, 64), (1, 5, 64), (3, 9, 64), (3, 5, 64), (6, 5, 32)]


def test_every_p8_instantiation_fits_registers_and_lds():
    usage = {k: v for k, v in _resource_usage("convtr.hip").items() if "convtr_p8_kernel" in k}
    for rt, nt, cinp in INSTANTIATIONS:
        hits = [v for k, v in usage.items() if "convtr_p8_kernelILi%dELi%dELi%dEE" % (rt, nt, cinp) in k]
        assert len(hits) == 1, (rt, nt, cinp, sorted(usage))
        u = hits[0]
        assert u["ScratchSize [bytes/lane]"] == 0 and u["VGPRs Spill"] == 0 and u["SGPRs Spill"] == 0, (rt, nt, cinp, u)
        assert u["VGPRs"] <= 256, (rt, nt, cinp, u)                       # two waves per SIMD: launch_bounds(512, 2)
        assert u["LDS Size [bytes/block]"] <= 160 * 1024, (rt, nt, cinp, u)
    assert len(usage) == len(INSTANTIATIONS), sorted(usage)


def test_workspace_covers_the_split_table():
    from opticalflowscivis_amd import _lib
    try:
        L = _lib.lib()
    except _lib.FlowsciLibraryError as e:
        pytest.skip("library not built: %s" % e)
    # words [chunk of 4 channels][row tile][piece 3] x 1 KB
    assert L.fs_conv3d_tr_ws_floats(32, 6) >= 8 * 3 * 3 * 256
    assert L.fs_conv3d_tr_ws_floats(32, 1) >= 8 * 1 * 3 * 256
    buf = (_lib.FsWprepJob * 4)()
    for cin, cout, rt in ((32, 6, 3), (32, 1, 1), (5, 6, 3), (8, 2, 1)):
        n = L.fs_conv3d_tr_wprep_jobs(buf, 4, 0x4000, 0x1000, 0x2000, 2, cin, cout, 128, 128, 128, 256, 256, 256, 0)
        assert n == 1 and buf[0].kind == 3, (cin, cout, n)
        assert buf[0].total == (cin + 3) // 4 * rt * 768 <= L.fs_conv3d_tr_ws_floats(cin, cout), (cin, cout, buf[0].total)
        assert [buf[0].p[i] for i in range(5)] == [cin, cout, (cin + 3) // 4 * 4, rt, 1], (cin, cout)
    # 64 input channels keep the fp32 table
    n = L.fs_conv3d_tr_wprep_jobs(buf, 4, 0x4000, 0x1000, 0x2000, 2, 64, 6, 32, 32, 64, 64, 64, 128, 0)
    assert n == 1 and buf[0].kind == 3 and buf[0].total == 64 * (128 * 3 + 16) and buf[0].p[4] == 0


# ---- the word layout ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def table(tmp_path_factory):
    """table(cin, cout, rt) -> the words of that layer's split table, from the host program (compiled once)"""
    if not (os.path.exists(HIPCC) or shutil.which("hipcc")):
        pytest.skip("needs hipcc")
    exe = str(tmp_path_factory.mktemp("p8s") / "p8s_words")
    r = subprocess.run([HIPCC, "-O2", "-std=c++17", "--cuda-host-only", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
                        os.path.join(ROOT, "tests", "tools", "p8s_words.hip"), "-o", exe], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    cache = {}

    def run(cin, cout, rt):
        if (cin, cout, rt) not in cache:
            r = subprocess.run([exe, str(cin), str(cout), str(rt)], capture_output=True, text=True, timeout=60)
            assert r.returncode == 0, r.stderr[-3000:]
            out = [int(line.split()[1], 16) for line in r.stdout.splitlines()]
            assert len(out) == (cin + 3) // 4 * rt * 768
            cache[(cin, cout, rt)] = out
        return cache[(cin, cout, rt)]

    return run


def _weight(cout, ci, co, kz, ky, kx):
    """element i of w[ci][co][tap] as tests/tools/p8s_words.hip fills it (exact in fp32)"""
    i = (ci * cout + co) * 64 + (kz * 4 + ky) * 4 + kx
    return np.float32(1.0 + i / 4096.0 + (i % 7) / 1048576.0 + 1.0 / 8388608.0)


def _bf16(a):
    """float32 -> (bf16 bits, its value as float32), round to nearest even"""
    u = int(np.float32(a).view(np.uint32))
    h = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) & 0xFFFF
    return h, np.uint32(h << 16).view(np.float32)


def _piece(a, piece):
    a = np.float32(a)
    for _ in range(piece):
        a = np.float32(a - _bf16(a)[1])
    return _bf16(a)[0]


def _index(rts, chunk, rt, piece, kq, row, xs, cp):
    return (((((chunk * rts + rt) * 3 + piece) * 4 + kq) * 16 + row) * 4) + xs * 2 + cp


# (pz, py, px), (dz, dy, dx) -> (kz, ky, kx), by hand from k = 2 d - p + 1 per axis
HAND = [
    ((0, 0, 0), (0, 0, 0), (1, 1, 1)),
    ((0, 0, 1), (0, 1, 1), (1, 3, 2)),
    ((0, 1, 0), (1, 0, 1), (3, 0, 3)),
    ((0, 1, 1), (1, 1, 0), (3, 2, 0)),
    ((1, 0, 0), (0, 0, 1), (0, 1, 3)),
    ((1, 0, 1), (1, 0, 0), (2, 1, 0)),
    ((1, 1, 0), (0, 1, 0), (0, 2, 1)),
    ((1, 1, 1), (1, 1, 1), (2, 2, 2)),
]


@pytest.mark.parametrize("cls,d,k", HAND, ids=["p%d%d%d" % c for c, _, _ in HAND])
def test_a_tap_of_each_parity_class(table, cls, d, k):
    cin, cout, rts = 5, 6, 3
    words = table(cin, cout, rts)
    (pz, py, px), (dz, dy, dx) = cls, d
    co = 4
    item = (pz * 2 + py) * cout + co          # 0 .. 23: row tile item / 8, row px 8 + item % 8
    rt, row = item // 8, px * 8 + item % 8
    kq, xs = dz * 2 + dy, 1 - dx              # the lower input position (dx = 1) is stored first
    for piece in range(3):
        # chunk 0, channel pair 1: channels 2 (low half) and 3 (high half)
        want = _piece(_weight(cout, 2, co, *k), piece) | (_piece(_weight(cout, 3, co, *k), piece) << 16)
        got = words[_index(rts, 0, rt, piece, kq, row, xs, 1)]
        assert got == want, (piece, hex(got), hex(want))
    assert _piece(_weight(cout, 2, co, *k), 1) != 0  # (the 2^-23 bit: the split is not trivial)


def test_padded_rows_are_zero(table):
    # one output channel: items 0 .. 3 = the four (pz, py) classes; rows 4 .. 7 and 12 .. 15 of the only tile are padding
    words = table(8, 1, 1)
    for chunk in range(2):
        for piece in range(3):
            for kq in range(4):
                for row in range(16):
                    for w4 in range(4):
                        w = words[_index(1, chunk, 0, piece, kq, row, w4 >> 1, w4 & 1)]
                        if row % 8 >= 4:
                            assert w == 0, (chunk, piece, kq, row, w4, hex(w))
                        elif piece < 2:  # (a third piece may be zero: the first two can hold the value exactly)
                            assert w & 0xFFFF != 0 and w >> 16 != 0, (chunk, piece, kq, row, w4, hex(w))
    # the mask head's row 9 = (px 1, item 1 = (pz 0, py 1)): neighbour (dz 1, dy 0, dx 0) -> taps (3, 0, 2), channels 4 and 5
    want = _piece(_weight(1, 4, 0, 3, 0, 2), 0) | (_piece(_weight(1, 5, 0, 3, 0, 2), 0) << 16)
    assert words[_index(1, 1, 0, 0, 2, 9, 1, 0)] == want


def test_channels_past_cin_are_zero(table):
    # chunk 1 holds channels 4 .. 7, Cin = 5: channel pair 0 = (4, 5) -> upper half zero; pair 1 = (6, 7) -> zero
    words = table(5, 6, 3)
    for piece in range(3):
        for kq in range(4):
            for row in (0, 5, 9, 15):
                for xs in range(2):
                    w0 = words[_index(3, 1, 1, piece, kq, row, xs, 0)]
                    assert w0 >> 16 == 0 and (piece > 0 or w0 & 0xFFFF != 0), (piece, kq, row, xs, hex(w0))
                    assert words[_index(3, 1, 1, piece, kq, row, xs, 1)] == 0
