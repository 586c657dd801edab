"""Cases and plain references for the helper kernels around the engine: the text generator
(textlen_kernel / scan_kernel / textgen_kernel, dsm_text.hip), gen_kernel, ffscan_kernel and
agg_kernel (dsm_kernels.hip).  Shared by tests/test_helpers_model.py (the CPU certificate of the
references and of what the case lists cover) and tests/test_gpu_helpers.py (the kernels)."""
from collections import namedtuple

import numpy as np

DISTS = ("uniform", "hot", "evict")
SEED = 11                       # the generator seed of every case below
FAR = (1 << 40) + 3             # a system id whose key does not fit 32 bits
PAD = 256                       # canary bytes on either side of a device output buffer
CANARY = 0xA5

# ---- grid caps: what one launch covers before its grid-stride loop takes a second iteration,
# per CU (cus: dsm_launch_info.cus).  Each constant copies the line named beside it.
TEXT_WRITE_FILES_PER_CU = 16 * 4    # dsm_text.hip dsm_generate_text_device: `wblocks > cus * 16`,
                                    # textgen_kernel: one file per wave, 4 waves per workgroup
TEXT_LEN_FILES_PER_CU = 8 * 256     # dsm_text.hip dsm_generate_text_device: `blocks > cus * 8`,
                                    # textlen_kernel: one file per thread, 256 threads
GEN_SLOTS_PER_CU = 512              # dsm_kernels.hip dsm_generate_device: `cap = cus * 512`,
                                    # gen_kernel: one (system, node) slot per workgroup iteration
AGG_SYSTEMS_PER_CU = 8 * 256        # dsm_kernels.hip dsm_aggregate_device: `cap = cus * 8`,
                                    # agg_kernel: one system per thread, 256 threads
SCAN_BLOCK = 1024                   # dsm_text.hip scan_kernel: one workgroup of 1024 threads,
                                    # ceil(n_files / 1024) offsets per thread
SCAN_SYS = 4096                     # dsm_plan.h SCAN_SYS: systems ffscan_kernel samples
SCAN_INSTR = 256                    # dsm_kernels.hip SCAN_INSTR: instructions per sampled trace
SCAN_RUN = 8                        # dsm_kernels.hip ffscan_kernel: `run >= 8u`


def beyond(cap_per_cu, cus, np_=1):
    """Systems of np_ units each that take a kernel past its grid cap: twice the cap plus an
    odd remainder, so a part with fewer CUs than the one the test ran on is past it too."""
    return 2 * cap_per_cu * cus // np_ + 1


# ---- text generator ----------------------------------------------------------------------
TextCase = namedtuple("TextCase", "np dist n_sys n_instr first_sys")

TEXT_CASES = (
    # every distribution at both widths: three systems of 67 lines hold all four line lengths
    [TextCase(n, d, 3, 67, 5000) for n in (4, 8) for d in DISTS] +
    # the writer's wave step (64 lines): empty, one line, one below / at / past a step, two
    # steps and a remainder, the longest trace and one below it
    [TextCase(n, d, 3, k, 5000) for k in (0, 1, 63, 64, 65, 130, 4095, 4096)
     for n, d in ((8, "uniform"), (4, "evict"))] +
    # the offset scan (1024 threads): one file per thread or fewer, exactly 1024 files, one
    # system below and above, and three files per thread with a remainder
    [TextCase(4, "uniform", s, 5, 5000) for s in (1, 255, 256, 257, 769)] +
    [TextCase(8, "uniform", s, 5, 5000) for s in (127, 128, 129, 385)] +
    [TextCase(8, "uniform", 2, 9, FAR), TextCase(8, "uniform", 0, 9, 5000)])


def text_large_cases(cus):
    """Second grid-stride iteration of textgen_kernel and of textlen_kernel (np 8, 3 lines)."""
    return [TextCase(8, "uniform", beyond(TEXT_WRITE_FILES_PER_CU, cus, 8), 3, 5000),
            TextCase(8, "uniform", beyond(TEXT_LEN_FILES_PER_CU, cus, 8), 3, 5000)]


def slot_stride(n_instr):
    """The smallest trace slot (a multiple of 8, at least 8) that holds n_instr instructions."""
    return max(8, (n_instr + 7) // 8 * 8)


def oracle_traces(orc, np_, dist, n_instr, first_sys, n_sys):
    """orc.generate, with the empty shapes answered here."""
    if n_sys == 0 or n_instr == 0:
        return np.zeros((n_sys, np_, n_instr), dtype=np.uint16)
    return orc.generate(np_, dist, SEED, n_instr, first_sys, n_sys)[0]


_HEX = np.frombuffer(b"0123456789abcdef", dtype=np.uint8)


def ref_text(tr):
    """The core files of a [n, np, k] u16 trace array in the shipped tests' format, one file per
    (system, node): "RD 0x%02x\\n" of the address, "WR 0x%02x %u\\n" of the address and the value
    (bit 15 WR, bits 8-14 address, bits 0-7 value).  Returns (bytes as a u8 array, n*np + 1
    u64 offsets)."""
    tr = np.asarray(tr, dtype=np.uint16)
    n, npn, k = tr.shape
    ins = tr.reshape(-1).astype(np.int64)
    wr = (ins >> 15) != 0
    a, v = (ins >> 8) & 0x7F, ins & 0xFF
    nd = 1 + (v >= 10) + (v >= 100)                     # decimal digits of the value
    ln = np.where(wr, 9 + nd, 8)
    pos = np.cumsum(ln) - ln
    out = np.zeros(int(ln.sum()), dtype=np.uint8)
    out[pos] = np.where(wr, ord("W"), ord("R"))
    out[pos + 1] = np.where(wr, ord("R"), ord("D"))
    out[pos + 2] = ord(" ")
    out[pos + 3] = ord("0")
    out[pos + 4] = ord("x")
    out[pos + 5] = _HEX[a >> 4]
    out[pos + 6] = _HEX[a & 15]
    out[pos + 7] = np.where(wr, ord(" "), ord("\n"))
    pw, vw, dw = pos[wr], v[wr], nd[wr]
    out[pw[dw == 3] + 8] = ord("0") + vw[dw == 3] // 100
    out[pw[dw >= 2] + 6 + dw[dw >= 2]] = ord("0") + (vw[dw >= 2] // 10) % 10
    out[pw + 7 + dw] = ord("0") + vw % 10
    out[pw + 8 + dw] = ord("\n")
    off = np.zeros(n * npn + 1, dtype=np.uint64)
    off[1:] = np.cumsum(ln.reshape(n * npn, k).sum(axis=1))
    return out, off


def line_lengths(tr):
    """The set of text line lengths of a trace array."""
    ins = np.asarray(tr, dtype=np.uint16).reshape(-1).astype(np.int64)
    v = ins & 0xFF
    return set(np.unique(np.where(ins >> 15, 10 + (v >= 10) + (v >= 100), 8)).tolist())


# ---- gen_kernel ---------------------------------------------------------------------------
GenCase = namedtuple("GenCase", "np dist stride n_instr n_sys first_sys")
GEN_STRIDES = (8, 16, 72, 520, 4096)        # 1, 2, 9, 65 and 512 16-byte chunks per slot


def _gen_counts(stride):
    return sorted({min(k, stride) for k in (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, stride - 1, stride)})


GEN_CASES = (
    [GenCase(8, "uniform", s, k, 5, 77) for s in GEN_STRIDES for k in _gen_counts(s)] +
    # each of the 12 instantiations (np x dist x FULL) at a ragged and at a full slot
    [GenCase(n, d, 72, k, 5, 77) for n in (4, 8) for d in DISTS for k in (37, 72)] +
    [GenCase(8, "uniform", 72, 37, 5, FAR)])


def gen_large_case(cus):
    """More slots than workgroups: the slot loop's second iteration."""
    return GenCase(8, "uniform", 8, 7, beyond(GEN_SLOTS_PER_CU, cus, 8), 77)


# ---- ffscan_kernel --------------------------------------------------------------------------
def ref_scan(tr, cn, stride, n_sys, np_):
    """ffscan_kernel's definition (dsm_plan.h "fast-forward verdict", dsm_kernels.hip): of
    S = min(n_sys, 4096) systems j * n_sys // S, every node's first min(count, stride, 256)
    instructions go through a private table of four entries, indexed by address & 3, that
    holds the last address seen there (nothing at the start); `run` counts consecutive hits,
    and an instruction at which run >= 8 ends a run.  Returns (instructions read, run ends)."""
    tr = np.asarray(tr, dtype=np.uint16).reshape(n_sys, np_, stride)
    cn = np.asarray(cn, dtype=np.int64).reshape(n_sys, np_)
    S = min(n_sys, SCAN_SYS)
    if S == 0:
        return 0, 0
    pick = np.arange(S, dtype=np.int64) * n_sys // S
    t = tr[pick].reshape(S * np_, stride).astype(np.int64)
    n = np.minimum(np.minimum(cn[pick].reshape(-1), stride), SCAN_INSTR)
    rows = np.arange(S * np_)
    table = np.full((S * np_, 4), -1, dtype=np.int64)
    run = np.zeros(S * np_, dtype=np.int64)
    ends = 0
    for i in range(int(n.max())):
        live = i < n
        a = (t[:, i] >> 8) & 0x7F
        hit = table[rows, a & 3] == a
        run = np.where(live, np.where(hit, run + 1, 0), run)
        table[rows[live], (a & 3)[live]] = a[live]
        ends += int((live & (run >= SCAN_RUN)).sum())
    return int(n.sum()), ends


def scan_verdict(instrs, runs):
    """dsm_plan.h ff_verdict."""
    return runs != 0 and runs * 16 >= instrs


CRAFT_REPEATS = (7, 8, 9)       # node j repeats its address CRAFT_REPEATS[j % 3] times ...
CRAFT_ENDS = (0, 1, 2)          # ... which ends this many runs per repetition
CRAFT_REPS = 20


def crafted_runs(np_, n_sys, stride=256):
    """Traces for the run threshold: node j issues, CRAFT_REPS times over, an address B and
    then an address A (A & 3 == B & 3, so B evicts A from the sampled table and A misses once)
    followed by r = CRAFT_REPEATS[j % 3] repeats of A: r hits in a row, run = r at the last,
    so r = 7, 8, 9 end 0, 1, 2 runs.  A final B closes the trace.  Returns (traces, counts)."""
    tr = np.zeros((n_sys, np_, stride), dtype=np.uint16)
    cn = np.zeros((n_sys, np_), dtype=np.uint32)
    for s in range(n_sys):
        for j in range(np_):
            a = (((j + s) % np_) << 4) | (1 + j % 3)
            b = a ^ 4
            ia = (a << 8) | ((1 << 15) | (s & 0xFF) if s & 1 else 0)       # RD, or WR of s
            ib = (b << 8) | ((1 << 15) | 200 if j & 1 else 0)
            seq = ([ib] + [ia] * (1 + CRAFT_REPEATS[j % 3])) * CRAFT_REPS + [ib]
            assert len(seq) <= min(stride, SCAN_INSTR)
            tr[s, j, :len(seq)] = seq
            cn[s, j] = len(seq)
    return tr, cn


def crafted_ends(np_, n_sys):
    return n_sys * CRAFT_REPS * sum(CRAFT_ENDS[j % 3] for j in range(np_))


# ---- agg_kernel -----------------------------------------------------------------------------
AGG_SIZES = (1, 63, 64, 65, 255, 256, 257, 1000)
AGG_FIRST = (0, 999_000, FAR)


def agg_large_size(cus):
    return 2 * AGG_SYSTEMS_PER_CU * cus + 5


def random_results(dtype, n, seed):
    """n result records: status 0..4 with a random dumped-node mask in bits 8-15, rounds, msgs
    and instrs over the whole u32 range, the two hashes over u64."""
    rng = np.random.default_rng(seed)
    res = np.zeros(n, dtype=dtype)
    res["status"] = rng.integers(0, 5, n, dtype=np.uint32) | (rng.integers(0, 256, n, dtype=np.uint32) << 8)
    for f in ("rounds", "msgs", "instrs"):
        res[f] = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    for f in ("dump_hash", "final_hash"):
        res[f] = rng.integers(0, 1 << 64, n, dtype=np.uint64)
    return res
