#!/usr/bin/env python3
"""Time of the exhaustive exploration (dsm_reach_device; DESIGN.md, "Exhaustive exploration") on
one input: the four-node contention system (tests/reach_cases.py C4) or a shipped test directory.

Warm-up searches, then `reps` timed ones: the call is synchronous, so each is wall time around
dsm_reach_device with every buffer already allocated by the caller (the call's own scratch --
state store, visited table, chunk buffers -- is allocated and freed inside it, and counts).  One
more search runs with DSM_REACH_TIMING=1 for the share of device time in each kernel class.
Beside it, the yardstick that predates the search: Engine.explore of `explore` seeded variants
of the same system (default 1 Mi), its time and how many outcomes it found; and, with --host, the
host reference's single-thread time on the same input, as a plain fact.

Prints one JSON line: min / max / median milliseconds per search and every call's in order, states
and transitions per second (at the median), levels, chunks, the kernel shares, the outcomes of both.

    python tools/reach_time.py [--input contention|sample|test_4|..] [--max-states 16777216] [--chunk 0]
                               [--reps 5] [--warmup 2] [--explore 1048576] [--host] [--out FILE]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "hp-assignment-2_amd"), os.path.join(REPO, "oracle"), os.path.join(REPO, "tests")]

NP, STRIDE = 4, 32
CLASSES = ("count", "expand", "insert", "resolve", "settle")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--input", default="contention")
    ap.add_argument("--max-states", type=int, default=1 << 24)
    ap.add_argument("--chunk", type=int, default=0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--explore", type=int, default=1 << 20)
    ap.add_argument("--host", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    import pydsm
    import pyoracle as orc
    if pydsm.device_count() < 1:
        raise SystemExit("reach_time: no GPU")
    if a.input == "contention":
        import reach_cases
        tr, cn = reach_cases.CASES["C4"][1:3]
    else:
        tr, cn = orc.load_test(os.path.join(REPO, "tests", "golden", "inputs", a.input))
    tr = np.array(tr, dtype=np.uint16).reshape(NP, STRIDE)
    cn = np.array(cn, dtype=np.uint32).reshape(NP)
    dev = torch.device("cuda", 0)
    n, term_cap = a.max_states, min(a.max_states, 1 << 20)
    out = {"input": a.input, "max_states": n, "chunk": a.chunk, "device": torch.cuda.get_device_name(0)}
    with pydsm.Engine(NP, STRIDE) as eng:
        d_tr = torch.from_numpy(tr.view(np.int16).reshape(-1)).to(dev)
        d_cn = torch.from_numpy(cn.view(np.int32)).to(dev)
        d_par = torch.zeros(n, dtype=torch.int32, device=dev)
        d_msk = torch.zeros(n, dtype=torch.uint8, device=dev)
        d_fps = torch.zeros(n, dtype=torch.int64, device=dev)
        d_term = torch.zeros(5 * term_cap, dtype=torch.int64, device=dev)
        info = np.zeros(len(pydsm.REACH_INFO_FIELDS), dtype=np.uint64)
        level_off = np.zeros(pydsm.REACH_MAX_LEVELS + 1, dtype=np.uint64)
        opts = pydsm.ReachOpts(16, pydsm.CENSUS_DUMPS, n, 0, a.chunk)
        st = torch.cuda.current_stream(dev).cuda_stream

        def search():
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            rc = eng.reach_device(d_tr, d_cn, opts, info, d_par, d_msk, d_fps, level_off, d_term, term_cap, st)
            t1 = time.perf_counter()
            assert rc == 0, rc
            return 1e3 * (t1 - t0)

        ms = [search() for _ in range(a.warmup + a.reps)][a.warmup:]
        i = pydsm.reach_info_to_dict(info)
        os.environ["DSM_REACH_TIMING"] = "1"
        timed_ms = search()
        del os.environ["DSM_REACH_TIMING"]
        kms = (ctypes.c_double * len(CLASSES))()
        chunks = ctypes.c_uint64(0)
        assert pydsm.lib().dsm_debug_reach_times(kms, ctypes.byref(chunks)) == 0
        terms = d_term.cpu().numpy().view(pydsm.REACH_TERMINAL_DTYPE)[:min(i["terminals"], term_cap)]
        table, cap = pydsm.reach_census(terms, pydsm.CENSUS_DUMPS)
        med = float(np.median(ms))
        out.update({"info": i, "ms": {"min": min(ms), "max": max(ms), "median": med, "reps": len(ms),
                           "calls": [round(x, 3) for x in ms]},
                    "states_per_s": i["states"] / (med * 1e-3), "transitions_per_s": i["transitions"] / (med * 1e-3),
                    "levels": i["levels"], "chunks": int(chunks.value), "timed_run_ms": timed_ms,
                    "kernel_ms": dict(zip(CLASSES, (float(x) for x in kms))),
                    "kernel_share": dict(zip(CLASSES, (float(x) / max(sum(kms), 1e-9) for x in kms))),
                    "outcomes": int(pydsm.census_header(table)["distinct"]),
                    "exhaustive": i["flags"] & 3 == 0})
        del d_par, d_msk, d_fps, d_term
        if a.explore:
            ex = []
            for _ in range(3):
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                oc = eng.explore(tr, cn, a.explore, 7, 0x8000)
                torch.cuda.synchronize(dev)
                ex.append(1e3 * (time.perf_counter() - t0))
            out["explore"] = {"variants": a.explore, "outcomes": len(oc), "ms_min": min(ex[1:]), "ms_max": max(ex[1:])}
    if a.host:
        t0 = time.perf_counter()
        h = pydsm.reach(NP, tr, cn, max_states=n)
        out["host_ms"] = 1e3 * (time.perf_counter() - t0)
        assert h["info"]["states"] == out["info"]["states"]
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
