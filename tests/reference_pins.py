"""The adversarial inputs pinned to the reference's own handler text (a helper module, imported
like adversarial.py): the table of stored variants, their inputs, and the loaders of
tests/golden/adversarial.

oracle/gen_fixtures.py `adversarial` runs every variant through oracle/_ref/ref_lockstep_np{4,8}
`packed` (the reference's handler and issue text under the lock-step schedule, seeded stalls, an
inbox limit and a round limit; the crafted hit runs of tests/hitrun_cases.py among them) and stores, per variant, one .npy of per-system result digests
(dsm_common.h dsm_result_digest, idx = the system's index), where the issue order is compared a
second .npy of per-system issue digests (the first 8 bytes of the md5 of the system's DEBUG_INSTR
lines), and an index.json entry with the input's sha256, status counts, sums and the 13 per-type
totals.  tests/test_reference_pins.py compares the oracle with them, tests/test_gpu_reference_pins.py
the engine, and the module fixtures of tests/test_gpu_routes.py, test_gpu_observers.py and
test_gpu_instances.py assert through pinned() that the oracle run they compare with is the stored
one where a variant exists."""
import hashlib
import json
import os
import subprocess

import numpy as np

import adversarial as adv
import hitrun_cases
import solo_inputs

DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "adversarial")
RES_DT = np.dtype([("status", "<u4"), ("rounds", "<u4"), ("msgs", "<u4"), ("instrs", "<u4"),
                   ("dump_hash", "<u8"), ("final_hash", "<u8")])
LOCKSTEP = 0x10000
NPS = (4, 8)
CRAFTED = dict(seed=5, n=4096, stride=72)
# one generated fixture beyond 32-bit system ids (ref_lockstep `gen`, not `packed`)
FAR = dict(name="np8_uniform_2p40", np=8, dist="uniform", seed=1, n_instr=64,
           first_sys=(1 << 40) + 12345, n_sys=1024)
STATUS = ("COMPLETED", "DEADLOCKED", "RING_OVERFLOW", "ASSERT_FAILED", "ROUND_LIMIT")


def _variant(kind, np_, stalls=False, cap=256, limit=0, issue=False):
    name = f"{kind}_np{np_}_" + ("stalls" if stalls else "lockstep")
    if cap != 256:
        name += f"_inbox{cap}"
    if limit:
        name += f"_limit{limit}"
    return dict(name=name, kind=kind, np=np_, stalls=stalls, cap=cap, limit=limit, issue=issue)


def variants():
    """Every stored variant: on the contention ensemble exactly the (schedule, inbox limit, round
    limit) combinations adversarial.ROUTES and OBSERVER_ROUTES compare with; the tiled scenarios,
    the crafted lone-node inputs, the generated ensemble and the crafted hit runs
    (tests/hitrun_cases.py, stride 2048) beside them."""
    lock, stall = (1 << adv.OBS_ROUND_LOG2[k] for k in ("lockstep", "stalls"))
    out = []
    for np_ in NPS:
        out += [_variant("contention", np_, issue=True),
                _variant("contention", np_, cap=64),
                _variant("contention", np_, stalls=True, issue=True),
                _variant("contention", np_, limit=lock, issue=True),
                _variant("contention", np_, stalls=True, limit=stall, issue=True),
                _variant("contention", np_, stalls=True, cap=adv.OBS_INBOX),
                _variant("tiled", np_, issue=True),
                _variant("tiled", np_, stalls=True, issue=True),
                _variant("crafted", np_),
                _variant("generated", np_),
                _variant("generated", np_, stalls=True),
                _variant("hitruns", np_)]
    return out


VARIANTS = {v["name"]: v for v in variants()}
_KINDS = {"tiled_scenarios": "tiled", "packed": "contention"}


def find(kind, np_, stalls=False, cap=256, limit=0):
    """The stored variant's name for a run of a test module's ensemble, or None."""
    name = _variant(_KINDS.get(kind, kind), np_, bool(stalls), cap, limit)["name"]
    return name if name in VARIANTS else None


def sched(v):
    """(seed, threshold) of a variant's schedule; the system's index is its schedule id."""
    return (adv.STALL_SEED, adv.STALL_THRESH) if v["stalls"] else (0, LOCKSTEP)


_inputs = {}


def inputs(kind, np_, orc=None):
    """-> (traces, counts) of a variant's ensemble, built once, read-only.  The generated one is
    the generator's systems of adversarial.GEN_ENSEMBLE in a GEN_STRIDE slot (orc: pyoracle)."""
    if (kind, np_) not in _inputs:
        if kind == "contention":
            tr, cn, _ = adv.contention(np_, adv.SEED, adv.N_CONTENTION)
            assert adv.digest(tr, cn) == adv.CONTENTION_SHA256[np_]
        elif kind == "tiled":
            tr, cn, _, _ = adv.tiled_scenarios(np_)
        elif kind == "crafted":
            tr, cn, _ = solo_inputs.crafted(np_, CRAFTED["seed"], CRAFTED["n"], CRAFTED["stride"])
        elif kind == "hitruns":
            tr, cn, _ = hitrun_cases.hitruns(np_, hitrun_cases.STRIDE)
        elif kind == "generated":
            g = adv.GEN_ENSEMBLE
            t, cn = orc.generate(np_, g["dist"], g["seed"], g["n_instr"], g["first"], g["n"])
            tr = np.zeros((g["n"], np_, adv.GEN_STRIDE), dtype=np.uint16)
            tr[:, :, :g["n_instr"]] = t
        else:
            raise KeyError(kind)
        tr = np.ascontiguousarray(tr, dtype=np.uint16)
        cn = np.ascontiguousarray(cn, dtype=np.uint32)
        tr.setflags(write=False)
        cn.setflags(write=False)
        _inputs[(kind, np_)] = (tr, cn)
    return _inputs[(kind, np_)]


# ---- digests -----------------------------------------------------------------------------------
def _fmix64(z):
    z = z ^ (z >> np.uint64(33))
    z = z * np.uint64(0xff51afd7ed558ccd)
    z = z ^ (z >> np.uint64(33))
    z = z * np.uint64(0xc4ceb9fe1a85ec53)
    return z ^ (z >> np.uint64(33))


def digests(res, first_idx=0):
    """dsm_result_digest (oracle/dsm_common.h) of every system: u64 [n]."""
    res = np.ascontiguousarray(res).view(RES_DT).reshape(-1)
    with np.errstate(over="ignore"):
        idx = np.arange(len(res), dtype=np.uint64) + np.uint64(first_idx)
        h = _fmix64(idx * np.uint64(0x9E3779B97F4A7C15) + np.uint64(1))
        h = _fmix64(h ^ (res["status"].astype(np.uint64) | (res["rounds"].astype(np.uint64) << np.uint64(32))))
        h = _fmix64(h ^ (res["msgs"].astype(np.uint64) | (res["instrs"].astype(np.uint64) << np.uint64(32))))
        h = _fmix64(h ^ res["dump_hash"])
        return _fmix64(h ^ res["final_hash"])


def text_digest(text):
    """The first 8 bytes of the md5 of a system's DEBUG_INSTR lines, as a little-endian u64."""
    return int.from_bytes(hashlib.md5(text).digest()[:8], "little")


class _Lines(dict):
    """event (node << 16 | packed instruction) -> its DEBUG_INSTR line (assignment.c:596-597)."""

    def __missing__(self, e):
        node, ins = e >> 16, e & 0xFFFF
        s = self[e] = b"Processor %d: instr type=%c, address=0x%02X, value=%d\n" % (
            node, b"W" if ins >> 15 else b"R", (ins >> 8) & 0x7F, ins & 0xFF)
        return s


_lines = _Lines()


def issue_digests(events):
    """events: per system a sequence of issue events -> u64 [n] of text_digest of their lines."""
    return np.array([text_digest(b"".join(map(_lines.__getitem__, np.asarray(ev).tolist())))
                     for ev in events], dtype=np.uint64)


def summary(res, types):
    """The index.json fields of a run: status counts, sums, maximum, hash sums, type totals."""
    res = np.ascontiguousarray(res).view(RES_DT).reshape(-1)
    st = np.bincount((res["status"] & 0xFF).astype(np.int64), minlength=5)
    return dict(systems=len(res), status=[int(x) for x in st[:5]],
                msgs=int(res["msgs"].sum(dtype=np.uint64)), instrs=int(res["instrs"].sum(dtype=np.uint64)),
                rounds=int(res["rounds"].sum(dtype=np.uint64)), max_rounds=int(res["rounds"].max()),
                sum_dump_hash="0x%016x" % int(res["dump_hash"].sum(dtype=np.uint64)),
                sum_final_hash="0x%016x" % int(res["final_hash"].sum(dtype=np.uint64)),
                types=[int(x) for x in np.asarray(types, dtype=np.uint64).reshape(-1, 13).sum(axis=0)])


SUMMARY_KEYS = ("systems", "status", "msgs", "instrs", "rounds", "max_rounds", "sum_dump_hash",
                "sum_final_hash", "types")


# ---- the stored fixtures -----------------------------------------------------------------------
_index = None


def index():
    global _index
    if _index is None:
        with open(os.path.join(DIR, "index.json")) as f:
            _index = json.load(f)
    return _index


def load(name):
    """-> (index entry, digests u64 [n], issue digests u64 [n] or None) of a stored variant."""
    e = index()["variants"][name]
    d = np.load(os.path.join(DIR, name + ".npy"))
    i = np.load(os.path.join(DIR, name + "_issue.npy")) if VARIANTS[name]["issue"] else None
    return e, d, i


def differing(name, res):
    """Indices of the systems whose result digest differs from the stored variant's."""
    _, d, _ = load(name)
    mine = digests(res)
    assert mine.shape == d.shape, (name, mine.shape, d.shape)
    return np.nonzero(mine != d)[0]


def pinned(kind, np_, stalls, cap, limit, res):
    """Where a variant is stored for this run of a test module's ensemble: the run's per-system
    digests are the reference's.  -> the variant's name, or None when none is stored."""
    name = find(kind, np_, stalls, cap, limit)
    if name is not None:
        bad = differing(name, res)
        assert bad.size == 0, (f"{name}: {bad.size} systems differ from the reference's handler text "
                               f"(tests/golden/adversarial); first {bad[:4].tolist()}: {res[bad[:2]]}")
    return name


STORM_KEYS = ("status", "rounds", "msgs", "instrs", "dump_hash", "final_hash")


def storm_fields(r):
    """One system's result as the index's storm entries hold it."""
    return dict(status=int(r["status"]), rounds=int(r["rounds"]), msgs=int(r["msgs"]), instrs=int(r["instrs"]),
                dump_hash="0x%016x" % int(r["dump_hash"]), final_hash="0x%016x" % int(r["final_hash"]))


def far_results():
    """The far fixture ([n, 6] u64, as tests/golden/ensemble holds results) as a result array."""
    g = np.load(os.path.join(DIR, FAR["name"] + ".npy"))
    res = np.zeros(len(g), dtype=RES_DT)
    for i, k in enumerate(RES_DT.names):
        res[k] = g[:, i]
    return res


# ---- the reference's handler text (oracle/_ref, where built) --------------------------------------
def ref_exe(np_, dbg=False):
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    return os.path.join(here, "oracle", "_ref", f"ref_lockstep_np{np_}" + ("_dbg" if dbg else ""))


_usable = {}


def ref_packed(np_, dbg=False):
    """-> (path of the reference-text runner that has the `packed` sub-command, None), or
    (None, the reason there is none): oracle/_ref is built only where the reference is present,
    and one built by an earlier recipe (oracle/build_ref.sh) has no `packed`."""
    exe = ref_exe(np_, dbg)
    if exe not in _usable:
        if not os.path.exists(exe):
            _usable[exe] = "oracle/_ref not built"
        else:
            r = subprocess.run([exe, "packed"], capture_output=True)      # no arguments: the usage line
            _usable[exe] = None if b"packed" in r.stderr else \
                "oracle/_ref was built by an earlier recipe (no `packed`): make -C oracle ref"
    return (exe, None) if _usable[exe] is None else (None, _usable[exe])


class RefError(RuntimeError):
    """ref_lockstep ended with an error: its exit status and what it wrote to stderr."""


ISSUE_PREFIX = b": instr type="


def run_ref_packed(exe, np_, traces, counts, tmp, seed=0, thresh=LOCKSTEP, cap=256, limit=0, lines=False):
    """ref_lockstep `packed` on an ensemble -> (res, dump [n, np, 64], fin, types u64 [n, 13],
    and with lines=True (a DEBUG_INSTR build) every system's issue lines as bytes)."""
    tp, cp, op = (os.path.join(str(tmp), f) for f in ("t.bin", "c.bin", "o.bin"))
    np.ascontiguousarray(traces, dtype="<u2").tofile(tp)
    np.ascontiguousarray(counts, dtype="<u4").tofile(cp)
    n, _, stride = traces.shape
    env = {k: v for k, v in os.environ.items() if not k.startswith("DSM_REF_")}
    if cap != 256:
        env["DSM_REF_INBOX_LIMIT"] = str(cap)
    if limit:
        env["DSM_REF_ROUND_LIMIT"] = str(limit)
    r = subprocess.run([exe, "packed", str(stride), str(n), tp, cp, op, str(seed), hex(thresh)],
                       env=env, stdout=subprocess.PIPE if lines else subprocess.DEVNULL, stderr=subprocess.PIPE)
    if r.returncode:
        raise RefError(f"{os.path.basename(exe)} packed: exit status {r.returncode}: "
                       f"{r.stderr.decode(errors='replace').strip()[-500:]}")
    rec = 32 + 2 * np_ * 64 + 13 * 8
    b = np.fromfile(op, dtype=np.uint8).reshape(n, rec)
    res = b[:, :32].copy().view(RES_DT).reshape(-1)
    recs = b[:, 32:32 + 2 * np_ * 64].reshape(n, 2, np_, 64)
    types = b[:, 32 + 2 * np_ * 64:].copy().view("<u8").reshape(n, 13)
    out = [res, recs[:, 0].copy(), recs[:, 1].copy(), types]
    if lines:
        ls = [l for l in r.stdout.splitlines(keepends=True) if ISSUE_PREFIX in l]
        assert len(ls) == int(res["instrs"].sum(dtype=np.uint64))
        ends = np.cumsum(res["instrs"].astype(np.int64))
        out.append([b"".join(ls[e - int(k):e]) for e, k in zip(ends.tolist(), res["instrs"].tolist())])
    return out
