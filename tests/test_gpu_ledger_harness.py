"""GPU (-m gpu): the ledgers' shared harness (tests/ledger_harness.py) held to what the ledger tests rely on.

Guarded: the pointer sits where `mis` says, and intact() / untouched() see a single float stored just below, just above
and inside the interior -- every store here is a torch store into the buffer's own allocation.  kernels_launched: around
one call of the mem ledger's smallest up_add row it reports status 0 and that row's kernel, and with an empty `known` set
it fails naming that kernel."""
import math
import os
import re
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ledger_harness as H  # noqa: E402
import mem_ledger as LG  # noqa: E402
import mem_ledger_inputs as I  # noqa: E402
import test_gpu_mem_ledger as M  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    return H.load_lib()


@pytest.mark.parametrize("mis", range(4))
def test_guarded_sees_a_store_on_either_side(lib, mis):
    n = 37
    g = H.Guarded(n, mis=mis)
    assert g.ptr() % 16 == 4 * mis and g.ptr(3) == g.ptr() + 12
    assert g.ptr() == g.buf.data_ptr() + 4 * g.lo and g.view((1, n)).data_ptr() == g.ptr()
    assert g.lo >= H.GUARD and g.buf.numel() - (g.lo + n) >= H.GUARD
    assert g.intact() and g.untouched()
    for at in (g.lo - 1, g.lo + n):  # the last float of the band below, the first of the band above
        g.buf[at] = 1.0
        assert not g.intact() and not g.untouched(), at
        g.buf.view(torch.int32)[at] = H.NAN_BITS
        assert g.intact() and g.untouched(), at
    for at in (0, n // 2, n - 1):
        g.t[at] = 1.0
        assert g.intact() and not g.untouched(), at
    z = H.Guarded(n, zero=True, mis=mis)
    assert z.intact() and not z.untouched() and bool((z.t == 0).all())


def test_kernels_launched_witnesses_one_call(lib):
    r = min((r for r in LG.ROWS if r["op"] == "up_add"),
            key=lambda r: r["B"] * r["C"] * math.prod(r["ext"]) * r["factor"] ** 3)
    (kernel,) = LG.kernels_of(r)
    call = M.Call(lib, r, I.data(r))

    def ours(name):
        return name in M.KNOWN or name.startswith(M.PREFIXES)

    rc, launched = H.kernels_launched(call.launch, LG.normalize, ours, M.KNOWN)
    assert rc == 0 and kernel in launched and set(launched) - LG.HELPERS == {kernel}, (rc, launched)
    assert H.kernels_launched(call.launch, LG.normalize, ours) == (rc, launched)
    with pytest.raises(AssertionError, match="does not know.*" + re.escape(kernel)):
        H.kernels_launched(call.launch, LG.normalize, ours, known=set())
    assert all(b.intact() for b in call.bufs.values())
