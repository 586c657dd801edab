"""Cases for the dump reader (dsm_parse_dump on the host, unfmt_kernel on the GPU) and a plain
model of printProcessorState's text in Python that does not call the library: the reader splits
a line on `|` and takes int(...) of the pieces, the formatter is the reference's format strings
(assignment.c:839-873) with `%`, and a text is accepted exactly when formatting what was read
gives the text back.  Shared by tests/test_dump_reader_host.py (which also certifies the model
against fixtures the reference produced) and tests/test_gpu_dump_reader.py."""
import ctypes
import functools
import glob
import json
import os

import numpy as np

BASE, MAX, SLOT = 1954, 1958, 1968            # DSM_DUMP_BASE / _MAX / _SLOT
ABSENT, E_FORMAT = 1, -5                      # DSM_DUMP_ABSENT, DSM_E_FORMAT
NPS = (4, 8)
# unfmt_kernel's launch (dsm_text.hip): records per workgroup iteration, and the grid cap per CU
UNFMT_FR = 16                                 # UNFMT_FR
UNFMT_GRID_PER_CU = 3                         # UNFMT_GRID_PER_CU

CACHE_NAMES = ("MODIFIED", "EXCLUSIVE", "SHARED", "INVALID")
DIR_NAMES = ("EM", "S", "U")
VALUES = (0, 9, 10, 99, 100, 255)
BITVECTORS = (0x00, 0x0A, 0xFF)
CACHE_ADDRS = (0x00, 0x7F, 0xFF)
SUBST = (b" ", b"0", b"9", b"A", b"a", b"|", b"\n", b"\x00", b"\x80")

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


# ---- the model ------------------------------------------------------------------------------
def model_format(node, rec):
    """printProcessorState's text of a 64-byte record (bytes 0..59 are printed)."""
    r = [int(x) for x in np.asarray(rec, dtype=np.uint8).reshape(64)]
    mem, bv, ds = r[0:16], r[16:32], r[32:48]
    ca, cv, cs = r[48:52], r[52:56], r[56:60]
    t = ["=======================================\n", " Processor Node: %d\n" % node,
         "=======================================\n\n", "-------- Memory State --------\n",
         "| Index | Address |   Value  |\n", "|----------------------------|\n"]
    t += ["|  %3d  |  0x%02X   |  %5d   |\n" % (i, (node << 4) + i, mem[i]) for i in range(16)]
    t += ["------------------------------\n\n", "------------ Directory State ---------------\n",
          "| Index | Address | State |    BitVector   |\n", "|------------------------------------------|\n"]
    t += ["|  %3d  |  0x%02X   |  %2s   |   0x%08X   |\n" % (i, (node << 4) + i, DIR_NAMES[ds[i]], bv[i])
          for i in range(16)]
    t += ["--------------------------------------------\n\n", "------------ Cache State ----------------\n",
          "| Index | Address | Value |    State    |\n", "|---------------------------------------|\n"]
    t += ["|  %3d  |  0x%02X   |  %3d  |  %8s \t|\n" % (i, ca[i], cv[i], CACHE_NAMES[cs[i]]) for i in range(4)]
    t += ["----------------------------------------\n\n"]
    return "".join(t)


def model_parse(raw):
    """bytes -> (node, record uint8 [64] with bytes 60..63 = 0, 2, 0, 0), or None when no node
    in 0..7 and record with states in range format to exactly these bytes."""
    try:
        lines = bytes(raw).decode("ascii").split("\n")
        node = int(lines[1].split(":")[1])
        mem = [int(lines[7 + i].split("|")[3]) for i in range(16)]
        d = [lines[28 + i].split("|") for i in range(16)]
        ds = [DIR_NAMES.index(x[3].strip()) for x in d]
        bv = [int(x[4], 16) for x in d]
        c = [lines[49 + i].split("|") for i in range(4)]
        ca = [int(x[2], 16) for x in c]
        cv = [int(x[3]) for x in c]
        cs = [CACHE_NAMES.index(x[4].strip()) for x in c]
    except (ValueError, IndexError):
        return None
    vals = mem + bv + ds + ca + cv + cs
    if not 0 <= node < 8 or min(vals) < 0 or max(vals) > 255:
        return None
    rec = np.array(vals + [0, 2, 0, 0], dtype=np.uint8)
    return (node, rec) if model_format(node, rec).encode("ascii") == bytes(raw) else None


# ---- fixtures the reference produced --------------------------------------------------------
def observed_texts():
    """The dump texts the unmodified OpenMP binary wrote: [(test, core, text)]."""
    out = []
    for p in sorted(glob.glob(os.path.join(GOLD, "observed", "*.json"))):
        with open(p) as f:
            cores = json.load(f)["cores"]
        for c in sorted(cores):
            out += [(os.path.basename(p)[:-5], int(c), o["text"]) for o in cores[c]["outcomes"].values()]
    return out


# ---- crafted records ----------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def crafted(np_):
    """[(node, record)]: all 16 EXCLUSIVE layouts, each of VALUES in every value column (the 16
    memory values, the 4 cache values), each of BITVECTORS and every directory state in every
    directory line, each of CACHE_ADDRS in every cache line, every non-EXCLUSIVE state in every
    cache line, every node id.  The records are shared and read-only."""
    out = []
    for em in range(16):
        for vi in range(len(VALUES)):
            r = np.zeros(64, dtype=np.uint8)
            for j in range(16):
                r[j] = VALUES[(j + vi) % 6]
                r[16 + j] = BITVECTORS[(j + vi + em) % 3]
                r[32 + j] = (j + vi) % 3
            for s in range(4):
                r[48 + s] = CACHE_ADDRS[(s + vi) % 3]
                r[52 + s] = VALUES[(s + vi + em) % 6]
                r[56 + s] = 1 if (em >> s) & 1 else (0, 2, 3)[(s + vi + em // 2) % 3]
            r[61] = 2
            r.setflags(write=False)
            out.append(((em * 6 + vi) % np_, r))
    return tuple(out)


def record_of_length(length):
    """A crafted record whose text has `length` bytes: EXCLUSIVE in the first length - BASE lines."""
    em = (1 << (length - BASE)) - 1
    return crafted(8)[em * 6 + 3][1]


def substitutions(np_):
    """Every single-byte substitution, by each of SUBST, of one text of each length BASE..MAX:
    a list of bytes.  Item k is made from the text of node k % np_, the node a device slot k
    must print."""
    out = []
    for length in range(BASE, MAX + 1):
        rec = record_of_length(length)
        texts = [bytearray(model_format(n, rec).encode("ascii")) for n in range(np_)]
        assert len(texts[0]) == length
        for pos in range(length):
            for ch in SUBST:
                t = bytearray(texts[len(out) % np_])
                t[pos] = ch[0]
                out.append(bytes(t))
    return out


def lowercase_hex(text):
    """`text` (str) with the first upper-case hex letter of its directory section in lower case."""
    i = text.index("BitVector")
    j = next(k for k in range(i + 60, len(text)) if text[k] in "ABCDEF" and text[k - 1] in "0123456789ABCDEFx")
    return text[:j] + text[j].lower() + text[j + 1:]


# ---- slot buffers ---------------------------------------------------------------------------
def pack_slots(texts, fill=0):
    """A list of bytes (None or b"": an absent slot) -> (uint8 [n, SLOT] with `fill` behind each
    text, uint32 [n] lengths)."""
    buf = np.full((len(texts), SLOT), fill, dtype=np.uint8)
    lens = np.zeros(len(texts), dtype=np.uint32)
    for k, t in enumerate(texts):
        if t:
            buf[k, :len(t)] = np.frombuffer(t, dtype=np.uint8)
            lens[k] = len(t)
    return buf, lens


def host_expect(dsm, buf, lens, np_):
    """What dsm_parse_dumps_device must give for a slot buffer, from dsm_parse_dump slot by slot:
    (int32 [n] statuses, uint8 [n, 64] records).  Only lens[k] bytes of slot k are handed over."""
    n = len(lens)
    status = np.zeros(n, dtype=np.int32)
    recs = np.zeros((n, 64), dtype=np.uint8)
    fn, node = dsm.lib().dsm_parse_dump, ctypes.c_int(0)
    rec = np.zeros(64, dtype=np.uint8)
    prec, pnode = ctypes.c_void_p(rec.ctypes.data), ctypes.byref(node)
    for k in range(n):
        ln = int(lens[k])
        if ln == 0:
            status[k] = ABSENT
            continue
        rc = E_FORMAT                                           # a length no slot can hold
        if ln <= SLOT:
            tmp = buf[k, :ln].copy()                            # its own allocation: no tail behind it
            rc = fn(ctypes.c_void_p(tmp.ctypes.data), ln, pnode, prec)
        if rc == 0 and node.value == k % np_:
            recs[k] = rec
        else:
            status[k] = E_FORMAT
    return status, recs


def cycle_texts(np_, n, start=0):
    """n slot texts that cycle through the crafted records (each printed for node k % np_), with
    every 7th slot absent and every 11th refused (a lower-case hex digit)."""
    cr = crafted(np_)
    out = []
    for k in range(n):
        rec = cr[(start + k) % len(cr)][1]
        t = model_format(k % np_, rec)
        if k % 7 == 3:
            out.append(None)
        elif k % 11 == 5:
            out.append(lowercase_hex(t).encode("ascii"))
        else:
            out.append(t.encode("ascii"))
    return out


def past_cap_slots(cus):
    """One slot more than the grid at its cap covers in one iteration."""
    return cus * UNFMT_GRID_PER_CU * UNFMT_FR + 1
