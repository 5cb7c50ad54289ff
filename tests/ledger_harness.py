"""What the dispatch ledgers share (a plain module, not collected): the names kernels go by, the enumeration of the
kernels a source compiles and the completeness assertions over it (CPU), and the guarded device buffers and the profiler
witness of the GPU tests.  A ledger itself -- rows, inputs, references, bands, entry-point calls -- stays in its own files
(tests/conv_ledger.py, tests/mem_ledger.py and their test_*.py)."""
import os
import re
import shutil
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "opticalflowscivis_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

DEV = torch.device("cuda:0")
GUARD = 4096
NAN_BITS = 0x7FC0DEAD  # a quiet NaN no kernel produces


def normalize(name):
    """A demangled kernel name as ops._KERNELS writes symbols: no `void `, no anonymous namespace, no argument list."""
    name = name.strip()
    if name.startswith("void "):
        name = name[5:]
    name = name.replace("(anonymous namespace)::", "")
    if name.endswith(".kd"):
        name = name[:-3]
    depth = 0
    for i, ch in enumerate(name):  # cut at the first '(' outside template brackets
        if ch == "<":
            depth += 1
        elif ch == ">":
            depth -= 1
        elif ch == "(" and depth == 0:
            return name[:i].strip()
    return name


def _demangle(raw):
    """`raw` with its mangled names demangled by c++filt (one process for all of them)."""
    mangled = sorted({n for n in raw if n.startswith("_Z")})
    if not mangled:
        return list(raw)
    out = subprocess.run(["c++filt"], input="\n".join(mangled), capture_output=True, text=True, check=True).stdout
    plain = dict(zip(mangled, out.splitlines()))
    return [plain.get(n, n) for n in raw]


# ---- CPU: the kernels a source compiles -----------------------------------------------------------------------------
def _extra_flags(src):
    """The flags csrc/Makefile adds for this source's object (`name.o ...: CXXFLAGS += ...`)."""
    with open(os.path.join(CSRC, "Makefile")) as f:
        m = re.search(r"^%s\.o\b[^\n:]*:\s*CXXFLAGS\s*\+=(.*)$" % re.escape(src[:-len(".hip")]), f.read(), flags=re.M)
    return m.group(1).split() if m else []


def _kernels_of(src):
    cmd = [HIPCC, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
           *_extra_flags(src), "-S", "--cuda-device-only", os.path.join(CSRC, src), "-o", "-"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    return re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", r.stdout, flags=re.M)


def compiled_kernels(sources, normalize):
    """The normalized names of every kernel hipcc compiles from `sources` (files of csrc/) for gfx950."""
    if not (os.path.exists(HIPCC) or shutil.which("hipcc")):
        pytest.skip("needs hipcc")
    if not shutil.which("c++filt"):
        pytest.skip("needs c++filt")
    with ThreadPoolExecutor(len(sources)) as ex:
        mangled = [n for names in ex.map(_kernels_of, sources) for n in names]
    return {normalize(n) for n in _demangle(mangled) if n.strip()}


def assert_complete(compiled, expected, unreachable, helpers):
    """`compiled` is exactly the rows' kernels (`expected`) plus `unreachable` plus `helpers`, and no kernel is two of them."""
    both = expected & set(unreachable)
    assert not both, "kernels both reached by a row and listed as unreachable: %s" % sorted(both)
    compute = compiled - helpers
    missing = sorted(compute - expected - set(unreachable))
    stale = sorted((expected | set(unreachable)) - compute)
    assert not missing, "compiled compute kernels without a ledger row: %s" % missing
    assert not stale, "ledger kernels the build no longer compiles: %s" % stale
    assert helpers <= compiled, "helpers no longer compiled: %s" % sorted(helpers - compiled)


# ---- GPU: guarded buffers and the launch witness --------------------------------------------------------------------
def load_lib():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from opticalflowscivis_amd import _lib
    return _lib.lib()


class Guarded:
    """n floats starting `mis` floats past a 16-byte boundary, between two guard bands of NAN_BITS; the interior starts as
    NAN_BITS too (an output element the kernel never writes then fails the comparison), or zero."""

    def __init__(self, n, zero=False, mis=0):
        self.n = int(n)
        self.buf = torch.empty(self.n + 2 * GUARD + 4, dtype=torch.float32, device=DEV)
        self.buf.view(torch.int32).fill_(NAN_BITS)
        self.lo = GUARD + mis
        self.t = self.buf[self.lo:self.lo + self.n]
        assert self.t.data_ptr() % 16 == 4 * mis
        if zero:
            self.t.zero_()

    def ptr(self, offset=0):
        return self.t.data_ptr() + 4 * offset

    def view(self, shape):
        return self.t.view(shape)

    def intact(self):
        b = self.buf.view(torch.int32)
        return bool((b[:self.lo] == NAN_BITS).all()) and bool((b[self.lo + self.n:] == NAN_BITS).all())

    def untouched(self):
        return bool((self.buf.view(torch.int32) == NAN_BITS).all())


def on_device(t, mis=0):
    """`t` on the GPU as a contiguous view starting `mis` floats past a 16-byte boundary."""
    buf = torch.empty(t.numel() + 4, dtype=torch.float32, device=DEV)
    v = buf[mis:mis + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 * mis
    return v


def stream():
    return torch.cuda.current_stream(DEV).cuda_stream


def kernels_launched(fn, normalize, is_ours, known=None):
    """(fn's return value, normalized names of the kernels it launched for which is_ours(name) holds) -- torch.profiler's
    device activity, which records launches from the ctypes-loaded library as well.  With `known` (a set of names), one
    of our kernels outside it is an error."""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        rc = fn()
        torch.cuda.synchronize()
    names = [normalize(n) for n in _demangle([e.name for e in prof.events()])]  # (a tracer may report mangled names)
    ours = [n for n in names if is_ours(n)]
    if known is not None:
        strangers = sorted(set(ours) - known)
        assert not strangers, "kernels of the ledger's sources that the ledger does not know: %s" % strangers
    return rc, ours
