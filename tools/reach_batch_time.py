#!/usr/bin/env python3
"""Time of the reach batch (dsm_reach_batch_device; DESIGN.md, "Reach batch") against a loop of
dsm_reach_device over the same systems, in one process: the generator's 512 one-instruction
four-node systems generate(4, dist, seed 11, n_instr 1, first 0, 512) for dist uniform and hot.

Per input: `warmup` calls, then `reps` timed ones.  The batch call is asynchronous, so a timed
call is wall time from a synchronised stream to the stream synchronised again, every buffer and
the ctx's scratch already there.  The loop calls the synchronous dsm_reach_device once per system
with the same per-system max_states; both sides write the info alone (terminals, parents and masks
NULL), and their states, flags and terminal counts are compared before anything is reported.

Prints one JSON line: per input the min / max / median milliseconds of both, every call's in
order, their ratio (loop median over batch median), states per second at the batch's median, the
systems the batch kept in flight and the bytes of its scratch.

    python tools/reach_batch_time.py [--dist uniform,hot] [--systems 512] [--max-states 65536] [--chunk 0]
                                     [--scratch-bytes 0] [--reps 5] [--warmup 2] [--no-loop] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "hp-assignment-2_amd"), os.path.join(REPO, "oracle")]

NP, STRIDE = 4, 8


def stats(ms):
    return {"min": min(ms), "max": max(ms), "median": float(np.median(ms)), "reps": len(ms),
            "calls": [round(x, 3) for x in ms]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dist", default="uniform,hot")
    ap.add_argument("--systems", type=int, default=512)
    ap.add_argument("--max-states", type=int, default=1 << 16)
    ap.add_argument("--chunk", type=int, default=0)
    ap.add_argument("--scratch-bytes", type=int, default=0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-loop", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    import pydsm
    import pyoracle as orc
    if pydsm.device_count() < 1:
        raise SystemExit("reach_batch_time: no GPU")
    dev = torch.device("cuda", 0)
    n, cap = a.systems, a.max_states
    out = {"systems": n, "max_states": cap, "chunk": a.chunk, "scratch_bytes": a.scratch_bytes,
           "slab_bytes": pydsm.reach_batch_slab_bytes(NP, max_states=cap, chunk=a.chunk),
           "device": torch.cuda.get_device_name(0), "inputs": {}}
    nw = len(pydsm.REACH_INFO_FIELDS)
    with pydsm.Engine(NP, STRIDE) as eng:
        st = torch.cuda.current_stream(dev).cuda_stream
        d_info = torch.zeros(n * nw, dtype=torch.int64, device=dev)
        for dist in a.dist.split(","):
            g_tr, cn = orc.generate(NP, dist, 11, 1, 0, n)
            tr = np.zeros((n, NP, STRIDE), dtype=np.uint16)
            tr[:, :, :1] = g_tr
            d_tr = torch.from_numpy(tr.view(np.int16).reshape(-1)).to(dev)
            d_cn = torch.from_numpy(np.ascontiguousarray(cn, dtype=np.uint32).view(np.int32).reshape(-1)).to(dev)
            opts = pydsm.ReachOpts(16, pydsm.CENSUS_DUMPS, cap, 0, a.chunk)

            def batch():
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                rc = eng.reach_batch_device(d_tr, d_cn, n, opts, d_info, None, 0, None, None, a.scratch_bytes, st)
                t1 = time.perf_counter()
                torch.cuda.synchronize(dev)
                t2 = time.perf_counter()
                assert rc == 0, rc
                return 1e3 * (t2 - t0), 1e3 * (t1 - t0)

            runs = [batch() for _ in range(a.warmup + a.reps)][a.warmup:]
            info = d_info.cpu().numpy().view(pydsm.REACH_INFO_DTYPE)[:n].copy()
            in_flight, scratch = eng.reach_batch_state()
            b = stats([r[0] for r in runs])
            res = {"batch_ms": b, "batch_enqueue_ms": stats([r[1] for r in runs]),
                   "states": int(info["states"].sum()), "max_states_seen": int(info["states"].max()),
                   "transitions": int(info["transitions"].sum()),
                   "can_deadlock": int(np.count_nonzero(info["by_status"][:, 1])),
                   "truncated": int(np.count_nonzero(info["flags"] & 3)),
                   "states_per_s": int(info["states"].sum()) / (b["median"] * 1e-3),
                   "in_flight": in_flight, "scratch_allocated": scratch}
            if not a.no_loop:
                one = np.zeros(nw, dtype=np.uint64)
                linfo = np.zeros((n, nw), dtype=np.uint64)
                o1 = pydsm.ReachOpts(16, pydsm.CENSUS_DUMPS, cap, 0, 0)

                def loop():
                    torch.cuda.synchronize(dev)
                    t0 = time.perf_counter()
                    for s in range(n):
                        rc = eng.reach_device(d_tr[s * NP * STRIDE:], d_cn[s * NP:], o1, one, None, None, None, None,
                                              None, 0, st)
                        assert rc == 0, rc
                        linfo[s] = one
                    torch.cuda.synchronize(dev)
                    return 1e3 * (time.perf_counter() - t0)

                lms = [loop() for _ in range(a.warmup + a.reps)][a.warmup:]
                li = linfo.view(pydsm.REACH_INFO_DTYPE).reshape(n)
                assert np.array_equal(li["states"], info["states"]) and np.array_equal(li["flags"], info["flags"])
                assert np.array_equal(li["by_status"], info["by_status"])
                res["loop_ms"] = stats(lms)
                res["loop_over_batch"] = res["loop_ms"]["median"] / b["median"]
            out["inputs"][dist] = res
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
