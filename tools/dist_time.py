#!/usr/bin/env python3
"""Time of the outcome distribution (dsm_reach_dist_device; DESIGN.md, "Outcome distribution") on
the four-node contention system (tests/reach_cases.py C4) and the shipped test_4, np 4.

Per input: warm-up calls, then `reps` timed ones of dsm_reach_device alone (the search, the
yardstick that predates the distribution), of dsm_reach_dist_device with one threshold (0x8000)
and with four (0x2000, 0x4000, 0x8000, 0xC000), all in one session.  Every call is synchronous,
so each figure is wall time around it with the caller's buffers already allocated; what the call
allocates and frees inside counts.  One more call of each distribution runs with
DSM_DIST_TIMING=1 for the milliseconds per phase: search, rebuild (with classes and offsets),
table, edges, push (all rounds of all thresholds).  Beside the times, the figures users quote:
the deadlock probability at 0x8000, the rarest outcome's probability, and the number of outcomes
below 2^-20, which a 1 Mi sample is likely to miss.

Prints one JSON line per input.

    python tools/dist_time.py [--inputs contention,test_4] [--max-states 16777216] [--reps 5] [--warmup 2] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "hp-assignment-2_amd"), os.path.join(REPO, "oracle"), os.path.join(REPO, "tests")]

NP, STRIDE = 4, 32
PHASES = ("search", "rebuild", "table", "edges", "push")
ONE, FOUR = (0x8000,), (0x2000, 0x4000, 0x8000, 0xC000)


def stats(ms):
    return {"min": round(min(ms), 3), "max": round(max(ms), 3), "median": round(statistics.median(ms), 3),
            "calls": [round(x, 3) for x in ms]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inputs", default="contention,test_4")
    ap.add_argument("--max-states", type=int, default=1 << 24)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    import pydsm
    import pyoracle as orc
    if pydsm.device_count() < 1:
        raise SystemExit("dist_time: no GPU")
    dev = torch.device("cuda", 0)
    n, term_cap = a.max_states, min(a.max_states, 1 << 20)
    lines = []
    for name in a.inputs.split(","):
        if name == "contention":
            import reach_cases
            tr, cn = reach_cases.CASES["C4"][1:3]
        else:
            tr, cn = orc.load_test(os.path.join(REPO, "tests", "golden", "inputs", name))
        tr = np.array(tr, dtype=np.uint16).reshape(NP, STRIDE)
        cn = np.array(cn, dtype=np.uint32).reshape(NP)
        out = {"input": name, "max_states": n, "device": torch.cuda.get_device_name(0)}
        with pydsm.Engine(NP, STRIDE) as eng:
            d_tr = torch.from_numpy(tr.view(np.int16).reshape(-1)).to(dev)
            d_cn = torch.from_numpy(cn.view(np.int32)).to(dev)
            d_par = torch.zeros(n, dtype=torch.int32, device=dev)
            d_msk = torch.zeros(n, dtype=torch.uint8, device=dev)
            d_fps = torch.zeros(n, dtype=torch.int64, device=dev)
            d_term = torch.zeros(5 * term_cap, dtype=torch.int64, device=dev)
            d_tm = torch.zeros(len(FOUR) * term_cap, dtype=torch.int64, device=dev)
            info = np.zeros(len(pydsm.REACH_INFO_FIELDS), dtype=np.uint64)
            dinfo = np.zeros((len(FOUR), len(pydsm.DIST_INFO_FIELDS)), dtype=np.uint64)
            level_off = np.zeros(pydsm.REACH_MAX_LEVELS + 1, dtype=np.uint64)
            opts = pydsm.ReachOpts(16, pydsm.CENSUS_DUMPS, n, 0, 0)
            st = torch.cuda.current_stream(dev).cuda_stream

            def search():
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                rc = eng.reach_device(d_tr, d_cn, opts, info, d_par, d_msk, d_fps, level_off, d_term, term_cap, st)
                t1 = time.perf_counter()
                assert rc == 0, rc
                return 1e3 * (t1 - t0)

            def dist(thresh):
                th = np.array(thresh, dtype=np.uint32)
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                rc = eng.reach_dist_device(d_tr, d_cn, opts, th, 0, info, dinfo, d_term, d_tm, term_cap, None, st)
                t1 = time.perf_counter()
                assert rc == 0, rc
                return 1e3 * (t1 - t0)

            for what, fn in (("search_ms", search), ("dist1_ms", lambda: dist(ONE)), ("dist4_ms", lambda: dist(FOUR))):
                for _ in range(a.warmup):
                    fn()
                out[what] = stats([fn() for _ in range(a.reps)])
            out["dist1_over_search"] = round(out["dist1_ms"]["median"] / out["search_ms"]["median"], 2)
            out["dist4_over_search"] = round(out["dist4_ms"]["median"] / out["search_ms"]["median"], 2)
            os.environ["DSM_DIST_TIMING"] = "1"
            try:
                for what, thresh in (("phases1_ms", ONE), ("phases4_ms", FOUR)):
                    dist(thresh)
                    ms = np.zeros(len(PHASES), dtype=np.float64)
                    assert pydsm.lib().dsm_debug_dist_times(pydsm._ptr(ms)) == 0
                    out[what] = {k: round(float(v), 3) for k, v in zip(PHASES, ms)}
            finally:
                del os.environ["DSM_DIST_TIMING"]
            ri = pydsm.reach_info_to_dict(info)
            out.update(states=ri["states"], transitions=ri["transitions"], terminals=ri["terminals"],
                       reach_flags=ri["flags"])
            r = eng.reach_dist(tr, cn, thresh=ONE, max_states=n)
            d = r["dist"][0]
            ps = sorted(o["mass"] for o in d["outcomes"])
            out.update(outcomes=len(ps), rounds=d["rounds"], edges=d["edges"], lost=d["lost"], dist_flags=d["flags"],
                       p_deadlock=d["by_status"][1] / pydsm.DIST_ONE, p_completed=d["by_status"][0] / pydsm.DIST_ONE,
                       p_rarest=ps[0] / pydsm.DIST_ONE, p_commonest=ps[-1] / pydsm.DIST_ONE,
                       outcomes_below_2_20=sum(1 for m in ps if m < pydsm.DIST_ONE >> 20),
                       outcomes_with_zero_mass=sum(1 for m in ps if m == 0))
        lines.append(json.dumps(out))
        print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
