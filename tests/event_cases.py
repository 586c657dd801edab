"""The event trace's cases (a helper module, imported like reference_pins.py): the variants whose
DEBUG_INSTR text is pinned to the reference's own (tests/golden/events, written by
tools/gen_event_fixtures.py where oracle/_ref is built), their inputs and schedules, the runner
that splits the `_dbg` binary's stdout into systems, and small helpers over event arrays.

Per variant the fixture holds one u64 per system: reference_pins.text_digest of the system's
stdout (every DEBUG_INSTR line, :596 to :751), systems separated by the np `Processor n
initialized` lines.  For the five tests/golden/inputs directories the full text is stored too."""
import hashlib
import json
import os
import subprocess

import numpy as np

import adversarial as adv
import reference_pins as rp

DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "events")
INPUT_DIRS = ("sample", "test_1", "test_2", "test_3", "test_4")
INIT = b" initialized\n"


def variants():
    """contention: lock-step, stalls, stalls + inbox OBS_INBOX, stalls + the stalls round limit;
    tiled: lock-step, stalls; crafted lock-step; the three storms -- each at np 4 and 8."""
    stall_limit = 1 << adv.OBS_ROUND_LOG2["stalls"]
    out = []
    for np_ in rp.NPS:
        out += [rp._variant("contention", np_),
                rp._variant("contention", np_, stalls=True),
                rp._variant("contention", np_, stalls=True, cap=adv.OBS_INBOX),
                rp._variant("contention", np_, stalls=True, limit=stall_limit),
                rp._variant("tiled", np_),
                rp._variant("tiled", np_, stalls=True),
                rp._variant("crafted", np_)]
        out += [dict(rp._variant("storm_" + s, np_), storm=s) for s in adv.STORMS]
    return out


VARIANTS = {v["name"]: v for v in variants()}


def inputs(v):
    """-> (traces [n, np, stride], counts [n, np]) of a variant, read-only."""
    if "storm" in v:
        return adv.storm(v["storm"], v["np"])
    return rp.inputs(v["kind"], v["np"])


def settings(v):
    """-> (sched (seed, thresh), round_limit_log2 or 0, inbox limit or 0) as the entry points take them."""
    return rp.sched(v), (v["limit"].bit_length() - 1 if v["limit"] else 0), (v["cap"] if v["cap"] != 256 else 0)


def load(name):
    return np.load(os.path.join(DIR, name + ".npy"))


def stored_text(test):
    with open(os.path.join(DIR, test + "_instr.txt"), "rb") as f:
        return f.read()


def ref_systems(exe, np_, traces, counts, tmp, seed=0, thresh=rp.LOCKSTEP, cap=256, limit=0, keep_text=False):
    """The `_dbg` binary's `packed` run of an ensemble -> per system the digest (u64 [n]) of its
    stdout, or with keep_text the text itself (a list of bytes).  The stdout is read as a stream:
    np `Processor n initialized` lines open a system."""
    tp, cp, op = (os.path.join(str(tmp), f) for f in ("et.bin", "ec.bin", "eo.bin"))
    np.ascontiguousarray(traces, dtype="<u2").tofile(tp)
    np.ascontiguousarray(counts, dtype="<u4").tofile(cp)
    n, _, stride = traces.shape
    env = {k: v for k, v in os.environ.items() if not k.startswith("DSM_REF_")}
    if cap != 256:
        env["DSM_REF_INBOX_LIMIT"] = str(cap)
    if limit:
        env["DSM_REF_ROUND_LIMIT"] = str(limit)
    p = subprocess.Popen([exe, "packed", str(stride), str(n), tp, cp, op, str(seed), hex(thresh)], env=env,
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    out, cur, inits = [], None, 0
    for line in p.stdout:
        if line.endswith(INIT) and line.startswith(b"Processor "):
            if inits == 0:
                if cur is not None:
                    out.append(cur if keep_text else cur.digest())
                cur = [] if keep_text else hashlib.md5()
            inits = (inits + 1) % np_
            continue
        assert inits == 0, line
        if keep_text:
            cur.append(line)
        else:
            cur.update(line)
    if cur is not None:
        out.append(cur if keep_text else cur.digest())
    err = p.stderr.read()
    if p.wait():
        raise rp.RefError(f"{os.path.basename(exe)} packed: exit status {p.returncode}: "
                          f"{err.decode(errors='replace').strip()[-500:]}")
    assert len(out) == n, (len(out), n)
    if keep_text:
        return [b"".join(t) for t in out]
    return np.array([int.from_bytes(d[:8], "little") for d in out], dtype=np.uint64)


def flat(ev, cnt):
    """events [n, cap] and counts [n] (all <= cap) -> the events of all systems back to back."""
    ev = np.asarray(ev)
    return ev[np.arange(ev.shape[1])[None, :] < np.asarray(cnt)[:, None]]


def index():
    with open(os.path.join(DIR, "index.json")) as f:
        return json.load(f)
