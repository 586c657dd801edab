#!/usr/bin/env python3
"""Time of the outcome fate (dsm_reach_fate_device; DESIGN.md, "Outcome fate") on the four-node
contention system (tests/reach_cases.py C4) and the shipped test_4, np 4, by tools/dist_time.py's
method: max_states 2^24, the default chunk, warm-up calls, then `reps` timed ones, every call
synchronous with the caller's buffers already allocated.

Per input: dsm_reach_fate_device for target deadlocked with 0, 1 (0x8000) and 4 thresholds, and in
the same session the yardstick, dsm_reach_dist_device with one threshold -- of this build, and with
--dist-lib FILE also of another build of the library (the parent commit's), timed in a child
process that loads it.  One more call of each runs with DSM_FATE_TIMING=1 / DSM_DIST_TIMING=1 for
the milliseconds per phase; the fate's sweeps of the values are to be compared with the
distribution's push.  Beside the times: the sweep counts, and the bytes one value sweep reads and
writes as computed from the edge and state counts (per edge 4 of dst, 1 of pk and two 8-byte
values; per state two 8-byte offsets, a class byte and two 8-byte values compared or stored).

Prints one JSON line per input.

    python tools/fate_time.py [--inputs contention,test_4] [--max-states 16777216] [--reps 5] [--warmup 2]
                              [--dist-lib FILE] [--out FILE]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "hp-assignment-2_amd"), os.path.join(REPO, "oracle"), os.path.join(REPO, "tests")]

NP, STRIDE = 4, 32
FATE_PHASES = ("search", "rebuild", "table", "edges", "class", "value", "rest")
DIST_PHASES = ("search", "rebuild", "table", "edges", "push")
ONE, FOUR = (0x8000,), (0x2000, 0x4000, 0x8000, 0xC000)


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


def time_dist(a, name):
    """dsm_reach_dist_device with one threshold -> {"dist1_ms", "dist_phases1_ms", "rounds"}"""
    import torch
    import pydsm
    dev = torch.device("cuda", 0)
    n, term_cap = a.max_states, min(a.max_states, 1 << 20)
    tr, cn = load(name)
    out = {}
    with pydsm.Engine(NP, STRIDE) as eng:
        d_tr = torch.from_numpy(tr.view(np.int16).reshape(-1)).to(dev)
        d_cn = torch.from_numpy(cn.view(np.int32)).to(dev)
        d_term = torch.zeros(5 * term_cap, dtype=torch.int64, device=dev)
        d_tm = torch.zeros(term_cap, dtype=torch.int64, device=dev)
        info = np.zeros(len(pydsm.REACH_INFO_FIELDS), dtype=np.uint64)
        dinfo = np.zeros((1, len(pydsm.DIST_INFO_FIELDS)), dtype=np.uint64)
        opts = pydsm.ReachOpts(16, pydsm.CENSUS_DUMPS, n, 0, 0)
        st = torch.cuda.current_stream(dev).cuda_stream
        th = np.array(ONE, dtype=np.uint32)

        def dist():
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            rc = eng.reach_dist_device(d_tr, d_cn, opts, th, 0, info, dinfo, d_term, d_tm, term_cap, None, st)
            t1 = time.perf_counter()
            assert rc == 0, rc
            return 1e3 * (t1 - t0)

        for _ in range(a.warmup):
            dist()
        out["dist1_ms"] = stats([dist() for _ in range(a.reps)])
        os.environ["DSM_DIST_TIMING"] = "1"
        try:
            dist()
            ms = np.zeros(len(DIST_PHASES), dtype=np.float64)
            assert pydsm.lib().dsm_debug_dist_times(pydsm._ptr(ms)) == 0
            out["dist_phases1_ms"] = {k: round(float(v), 3) for k, v in zip(DIST_PHASES, ms)}
        finally:
            del os.environ["DSM_DIST_TIMING"]
        out["rounds"] = pydsm.dist_info_to_dict(dinfo[0])["rounds"]
    return out


def time_fate(a, name):
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
        d_cls = torch.zeros(n, dtype=torch.uint8, device=dev)
        d_lo = torch.zeros(len(FOUR) * n, dtype=torch.int64, device=dev)
        d_hi = torch.zeros(len(FOUR) * n, dtype=torch.int64, device=dev)
        d_term = torch.zeros(5 * term_cap, dtype=torch.int64, device=dev)
        info = np.zeros(len(pydsm.REACH_INFO_FIELDS), dtype=np.uint64)
        finfo = np.zeros(len(pydsm.FATE_INFO_FIELDS), dtype=np.uint64)
        values = np.zeros((len(FOUR), len(pydsm.FATE_VALUE_FIELDS)), dtype=np.uint64)
        level_off = np.zeros(pydsm.REACH_MAX_LEVELS + 1, dtype=np.uint64)
        opts = pydsm.ReachOpts(16, pydsm.CENSUS_DUMPS, n, 0, 0)
        fopts = pydsm.FateOpts(1 << 1, 0, 0)            # deadlocked
        st = torch.cuda.current_stream(dev).cuda_stream

        def fate(thresh):
            th = np.array(thresh, dtype=np.uint32)
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            rc = eng.reach_fate_device(d_tr, d_cn, opts, fopts, th, info, finfo, values, d_par, d_msk, level_off, d_term,
                                       term_cap, d_cls, d_lo, d_hi, st)
            t1 = time.perf_counter()
            assert rc == 0, rc
            return 1e3 * (t1 - t0)

        sets = (("fate0", ()), ("fate1", ONE), ("fate4", FOUR))
        for what, thresh in sets:
            for _ in range(a.warmup):
                fate(thresh)
            out[what + "_ms"] = stats([fate(thresh) for _ in range(a.reps)])
        os.environ["DSM_FATE_TIMING"] = "1"
        try:
            for what, thresh in sets:
                fate(thresh)
                ms, sw = np.zeros(len(FATE_PHASES), dtype=np.float64), np.zeros(2, dtype=np.uint64)
                assert pydsm.lib().dsm_debug_fate_times(pydsm._ptr(ms), pydsm._ptr(sw)) == 0
                out[what + "_phases_ms"] = {k: round(float(v), 3) for k, v in zip(FATE_PHASES, ms)}
                out[what + "_sweeps"] = {"class": int(sw[0]), "value": int(sw[1])}
        finally:
            del os.environ["DSM_FATE_TIMING"]
        ri, fi = pydsm.reach_info_to_dict(info), pydsm.fate_info_to_dict(finfo)
        out.update(states=ri["states"], transitions=ri["transitions"], terminals=ri["terminals"], levels=ri["levels"],
                   reach_flags=ri["flags"], fate=fi, values=[pydsm.fate_value_to_dict(values[j]) for j in range(len(FOUR))],
                   pull_form="one lane per source (np 4)",
                   value_sweep_bytes=fi["edges"] * (4 + 1 + 16) + ri["states"] * (16 + 1 + 16))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inputs", default="contention,test_4")
    ap.add_argument("--max-states", type=int, default=1 << 24)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--dist-lib", help="another build of libdsm.so whose dsm_reach_dist_device is timed too")
    ap.add_argument("--only-dist", help=argparse.SUPPRESS)
    ap.add_argument("--out")
    a = ap.parse_args()
    import pydsm
    if pydsm.device_count() < 1:
        raise SystemExit("fate_time: no GPU")
    if a.only_dist:                                     # the child of --dist-lib
        print(json.dumps(time_dist(a, a.only_dist)), flush=True)
        return
    lines = []
    for name in a.inputs.split(","):
        out = time_fate(a, name)
        out.update(time_dist(a, name))
        if a.dist_lib:
            env = dict(os.environ, DSM_LIB=os.path.abspath(a.dist_lib))
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--only-dist", name, "--max-states",
                                str(a.max_states), "--reps", str(a.reps), "--warmup", str(a.warmup)], env=env,
                               capture_output=True, text=True, timeout=900, check=True)
            out["other_lib"] = json.loads(r.stdout.strip().splitlines()[-1])
        v, p = out["fate1_phases_ms"]["value"], out["dist_phases1_ms"]["push"]
        out["value_over_push"] = round(v / p, 3) if p else None
        lines.append(json.dumps(out))
        print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
