"""Crafted ensembles for the serial pass's run phase (a helper module, imported like
adversarial.py): one node with a trace of a chosen length beside nodes of 0-7 instructions that
finish first, so the long node becomes the lone one early and enters the runs
(dsm_serial.h ser_solo) at whatever instruction index it has then.

Address families, a third of the systems each way: adversarial.contention()'s few-address
systems (1-8 distinct blocks, half of them on one cache index: every miss evicts) and all
np * 16 blocks uniformly.  LENS are the lone traces' lengths around the 8-instruction chunk
boundaries of the packed trace."""
import numpy as np

import adversarial

LENS = (1, 7, 8, 9, 15, 16, 17, 63, 64, 65)


def up8(x):
    return -(-x // 8) * 8


def crafted(np_, seed, n, stride, lens=LENS, multi=None):
    """-> (traces u16 [n, np, stride], counts u32 [n, np], who [n]): system i's node who[i] has
    lens[i % len(lens)] instructions (at most the stride), the others 0-7.  multi: a bool [n];
    where set, every node has the long length, so the system is still multi-node when the
    budget pass suspends it."""
    base = max(72, up8(stride))
    tr, _, _ = adversarial.contention(np_, seed, n, stride=base)
    rng = np.random.default_rng(seed + 1000)
    wide = np.arange(n) % 3 == 2
    addr = rng.integers(0, np_ * 16, (n, np_, base))
    wr = (rng.random((n, np_, base)) < 0.5).astype(np.int64)
    val = rng.integers(0, 256, (n, np_, base)) * wr
    wtr = ((wr << 15) | (addr << 8) | val).astype(np.uint16)
    tr = np.where(wide[:, None, None], wtr, tr)[:, :, :stride]
    who = rng.integers(0, np_, n)
    length = np.minimum(np.array(lens)[np.arange(n) % len(lens)], stride)
    cn = np.minimum(rng.integers(0, 8, (n, np_)), stride)
    cn[np.arange(n), who] = length
    if multi is not None:
        cn = np.where(multi[:, None], length[:, None], cn)
    return np.ascontiguousarray(tr, dtype=np.uint16), cn.astype(np.uint32), who


def beyond_np(orc, seed, n, n_instr=512):
    """4-node uniform traces with one instruction homed at nodes 4-7 in every node's trace, at
    index 40-399: whichever node is the lone one meets it (ASSERT_FAILED, include/dsm.h)."""
    tr, cn = orc.generate(4, "uniform", seed, n_instr, 0, n)
    rng = np.random.default_rng(seed)
    i = rng.integers(40, 400, (n, 4))
    a = 0x40 + rng.integers(0, 64, (n, 4))
    s, nd = np.meshgrid(np.arange(n), np.arange(4), indexing="ij")
    tr[s, nd, i] = (tr[s, nd, i] & 0x80FF) | (a << 8).astype(np.uint16)
    return tr, cn
