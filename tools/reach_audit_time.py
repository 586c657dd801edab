#!/usr/bin/env python3
"""Time of the reach audit (dsm_reach_audit_device; DESIGN.md, "Reach audit") on the four-node
contention system (tests/reach_cases.py C4, 663,027 states) and the shipped test_4, np 4, by
tools/fate_time.py's method: max_states 2^24, the default chunk, warm-up calls, then `reps` timed
ones, every call synchronous with the caller's buffers already allocated.

Per input: dsm_reach_audit_device with every output, and in the same session the yardstick,
dsm_reach_device alone on the same input.  `reps` more calls run with DSM_RAUDIT_TIMING=1 for the
milliseconds per phase on the stream -- search, rebuild, class, audit (reach_audit_kernel alone) --
of which the medians are reported; beside them the bytes the audit kernel reads and writes per
state (its 16 np record words, np fills, the status word and the class byte read, the word and the
set byte written), those bytes over the audit phase's time, and that rate as a fraction of the HBM
peak (8 TB/s on the MI355X).

Prints one JSON line per input.

    python tools/reach_audit_time.py [--inputs contention,test_4] [--max-states 16777216] [--reps 5] [--warmup 2]
                                     [--out FILE]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "hp-assignment-2_amd"), os.path.join(REPO, "oracle"), os.path.join(REPO, "tests")]

NP, STRIDE = 4, 32
PHASES = ("search", "rebuild", "class", "audit")
HBM_PEAK = 8.0e12                  # bytes per second, MI355X


def stats(ms):
    return {"min": round(min(ms), 3), "max": round(max(ms), 3), "median": round(statistics.median(ms), 3),
            "calls": [round(x, 3) for x in ms]}


def load(name):
    import pyoracle as orc
    if name == "contention":
        import reach_cases
        tr, cn = reach_cases.CASES["C4"][1:3]
    else:
        tr, cn = orc.load_test(os.path.join(REPO, "tests", "golden", "inputs", name))
    return np.array(tr, dtype=np.uint16).reshape(NP, STRIDE), np.array(cn, dtype=np.uint32).reshape(NP)


def time_input(a, name):
    import torch
    import pydsm
    dev = torch.device("cuda", 0)
    n, term_cap = a.max_states, min(a.max_states, 1 << 20)
    tr, cn = load(name)
    out = {"input": name, "max_states": n, "device": torch.cuda.get_device_name(0)}
    with pydsm.Engine(NP, STRIDE) as eng:
        d_tr = torch.from_numpy(tr.view(np.int16).reshape(-1)).to(dev)
        d_cn = torch.from_numpy(cn.view(np.int32)).to(dev)
        d_par = torch.zeros(n, dtype=torch.int32, device=dev)
        d_msk = torch.zeros(n, dtype=torch.uint8, device=dev)
        d_words = torch.zeros(n, dtype=torch.int32, device=dev)
        d_sets = torch.zeros(n, dtype=torch.uint8, device=dev)
        d_term = torch.zeros(5 * term_cap, dtype=torch.int64, device=dev)
        d_tw = torch.zeros(term_cap, dtype=torch.int32, device=dev)
        info = np.zeros(len(pydsm.REACH_INFO_FIELDS), dtype=np.uint64)
        ainfo = np.zeros(1, dtype=pydsm.RAUDIT_INFO_DTYPE)
        level_off = np.zeros(pydsm.REACH_MAX_LEVELS + 1, dtype=np.uint64)
        opts = pydsm.ReachOpts(16, pydsm.CENSUS_DUMPS, n, 0, 0)
        st = torch.cuda.current_stream(dev).cuda_stream

        def audit():
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            rc = eng.reach_audit_device(d_tr, d_cn, opts, info, ainfo, d_par, d_msk, level_off, d_term, term_cap, d_words,
                                        d_sets, d_tw, st)
            t1 = time.perf_counter()
            assert rc == 0, rc
            return 1e3 * (t1 - t0)

        def reach():
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            rc = eng.reach_device(d_tr, d_cn, opts, info, d_par, d_msk, None, level_off, d_term, term_cap, st)
            t1 = time.perf_counter()
            assert rc == 0, rc
            return 1e3 * (t1 - t0)

        for what, fn in (("reach_ms", reach), ("audit_call_ms", audit)):
            for _ in range(a.warmup):
                fn()
            out[what] = stats([fn() for _ in range(a.reps)])
        os.environ["DSM_RAUDIT_TIMING"] = "1"
        try:
            rows, nbytes = [], ctypes.c_uint64(0)
            for _ in range(a.reps):
                audit()
                ms = np.zeros(len(PHASES), dtype=np.float64)
                assert pydsm.lib().dsm_debug_raudit_times(pydsm._ptr(ms), ctypes.byref(nbytes)) == 0
                rows.append(ms)
        finally:
            del os.environ["DSM_RAUDIT_TIMING"]
        med = np.median(np.stack(rows), axis=0)
        out["phases_ms"] = {k: round(float(v), 4) for k, v in zip(PHASES, med)}
        out["audit_phase_calls_ms"] = [round(float(r[3]), 4) for r in rows]
        ri = pydsm.reach_info_to_dict(info)
        a_ms = float(med[3])
        out.update(states=ri["states"], transitions=ri["transitions"], terminals=ri["terminals"], levels=ri["levels"],
                   reach_flags=ri["flags"], audit={k: pydsm.audit_to_dict(ainfo[0]["set"][i])
                                                   for i, k in enumerate(pydsm.RAUDIT_SET_NAMES)},
                   audit_bytes=int(nbytes.value), bytes_per_state=round(nbytes.value / max(ri["states"], 1), 1),
                   audit_bytes_per_s=round(nbytes.value / (a_ms * 1e-3)) if a_ms else None,
                   audit_fraction_of_hbm_peak=round(nbytes.value / (a_ms * 1e-3) / HBM_PEAK, 4) if a_ms else None,
                   audit_over_search=round(a_ms / float(med[0]), 5) if med[0] else None,
                   call_over_reach=round(out["audit_call_ms"]["median"] / out["reach_ms"]["median"], 4))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inputs", default="contention,test_4")
    ap.add_argument("--max-states", type=int, default=1 << 24)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out")
    a = ap.parse_args()
    import pydsm
    if pydsm.device_count() < 1:
        raise SystemExit("reach_audit_time: no GPU")
    lines = []
    for name in a.inputs.split(","):
        lines.append(json.dumps(time_input(a, name)))
        print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
