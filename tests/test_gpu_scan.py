"""GPU: the exclusive scan the exhaustive exploration and the outcome distribution share
(dsm_reach.hip scan_sums_kernel / scan_top_kernel / scan_final_kernel behind dsm_exscan_launch,
through the test-only dsm_debug_exscan_device) against numpy.cumsum in uint64, out[n] the total.

A tile is 2 048 items and the top kernel scans 256 tile sums per pass, so the sizes are one tile and
its edges, 256 tiles and one item past them (the first carry of the top kernel's loop, which no
search of the suite comes near) and a ragged third batch.  The values are seeded and below 16; the
2 049 case also holds 0xFFFFFFFF at four places, so a 32-bit accumulation anywhere would show.  The
output lies between two canaries that must survive."""
import numpy as np
import pytest

import helper_cases as hc

pytestmark = pytest.mark.gpu

SIZES = (1, 2047, 2048, 2049, 524288, 524289, 1050000)
BIG_AT = (0, 1023, 2047, 2048)       # both tiles of the 2 049 case, the last item of the first included


@pytest.fixture(scope="module")
def eng():
    import pydsm
    if pydsm.device_count() < 1:
        pytest.fail("gpu tests need a GPU (no fallback exists)")
    with pydsm.Engine(4, 8) as e:
        yield e


def values(n):
    v = np.random.default_rng(0x5CA9 + n).integers(0, 16, size=n, dtype=np.uint32)
    if n == 2049:
        v[list(BIG_AT)] = 0xFFFFFFFF
    return v


@pytest.mark.parametrize("n", SIZES)
def test_exscan(eng, n):
    import torch
    v = values(n)
    ref = np.zeros(n + 1, dtype=np.uint64)
    np.cumsum(v, dtype=np.uint64, out=ref[1:])
    if n == 2049:
        assert int(ref[n]) > 4 * 0xFFFFFFFF > 1 << 33
    d_in = torch.from_numpy(v.view(np.int32)).cuda()
    nbytes = 8 * (n + 1)
    raw = torch.full((hc.PAD + nbytes + hc.PAD,), hc.CANARY, dtype=torch.uint8, device="cuda")
    ptr = raw.data_ptr() + hc.PAD
    assert ptr % 8 == 0
    eng.debug_exscan_device(d_in, n, ptr, torch.cuda.current_stream().cuda_stream)
    got = raw.cpu().numpy()
    out = got[hc.PAD:hc.PAD + nbytes].view(np.uint64)
    bad = np.nonzero(out != ref)[0]
    assert bad.size == 0, (f"{bad.size} of {n + 1} entries differ, the first at {int(bad[0])}: "
                           f"{int(out[bad[0]])} for {int(ref[bad[0]])}")
    assert (got[:hc.PAD] == hc.CANARY).all() and (got[hc.PAD + nbytes:] == hc.CANARY).all()
