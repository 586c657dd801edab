#!/usr/bin/env python3
"""Time of the reach batch audit (dsm_reach_batch_audit_device; DESIGN.md, "Reach batch audit") in
one process, by tools/reach_batch_time.py's method and on its inputs: the generator's 512
one-instruction four-node systems generate(4, dist, seed 11, n_instr 1, first 0, 512) for dist
uniform and hot.  Three calls are compared:

  (a) the audit call, writing info and ainfo alone (every row output NULL);
  (b) the plain dsm_reach_batch_device, writing the info alone;
  (c) a loop of the synchronous dsm_reach_audit_device, once per system, writing rinfo and ainfo.

Per input and call: `warmup` calls, then `reps` timed ones.  (a) and (b) are asynchronous, so a
timed call is wall time from a synchronised stream to the stream synchronised again, every buffer
and the ctx's scratch already there.  Before anything is reported (a)'s info equals (b)'s, and
(a)'s summaries, first depths and flags equal (c)'s, system by system.

Prints one JSON line: per input the min / max / median milliseconds of each call, every call's in
order, the ratios (a)/(b) and (c)/(a) of the medians, states per second at (a)'s median, the systems
that can end incoherent, the systems (a) kept in flight and the bytes of its scratch.

    python tools/reach_batch_audit_time.py [--dist uniform,hot] [--systems 512] [--max-states 65536] [--chunk 0]
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
        raise SystemExit("reach_batch_audit_time: no GPU")
    dev = torch.device("cuda", 0)
    n, cap = a.systems, a.max_states
    out = {"systems": n, "max_states": cap, "chunk": a.chunk, "scratch_bytes": a.scratch_bytes,
           "slab_bytes": pydsm.reach_batch_slab_bytes(NP, max_states=cap, chunk=a.chunk),
           "device": torch.cuda.get_device_name(0), "inputs": {}}
    nw, aw = len(pydsm.REACH_INFO_FIELDS), pydsm.RAUDIT_INFO_DTYPE.itemsize // 8
    with pydsm.Engine(NP, STRIDE) as eng:
        st = torch.cuda.current_stream(dev).cuda_stream
        d_info = torch.zeros(n * nw, dtype=torch.int64, device=dev)
        d_pinfo = torch.zeros(n * nw, dtype=torch.int64, device=dev)
        d_ainfo = torch.zeros(n * aw, dtype=torch.int64, device=dev)
        for dist in a.dist.split(","):
            g_tr, cn = orc.generate(NP, dist, 11, 1, 0, n)
            tr = np.zeros((n, NP, STRIDE), dtype=np.uint16)
            tr[:, :, :1] = g_tr
            d_tr = torch.from_numpy(tr.view(np.int16).reshape(-1)).to(dev)
            d_cn = torch.from_numpy(np.ascontiguousarray(cn, dtype=np.uint32).view(np.int32).reshape(-1)).to(dev)
            opts = pydsm.ReachOpts(16, pydsm.CENSUS_DUMPS, cap, 0, a.chunk)

            def timed(call):
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                rc = call()
                t1 = time.perf_counter()
                torch.cuda.synchronize(dev)
                t2 = time.perf_counter()
                assert rc == 0, rc
                return 1e3 * (t2 - t0), 1e3 * (t1 - t0)

            def audit():
                return eng.reach_batch_audit_device(d_tr, d_cn, n, opts, d_info, d_ainfo, None, 0, None, None, None, None,
                                                    None, a.scratch_bytes, st)

            def plain():
                return eng.reach_batch_device(d_tr, d_cn, n, opts, d_pinfo, None, 0, None, None, a.scratch_bytes, st)

            a_runs = [timed(audit) for _ in range(a.warmup + a.reps)][a.warmup:]
            in_flight, scratch = eng.reach_batch_state()
            b_runs = [timed(plain) for _ in range(a.warmup + a.reps)][a.warmup:]
            info = d_info.cpu().numpy().view(pydsm.REACH_INFO_DTYPE)[:n].copy()
            pinfo = d_pinfo.cpu().numpy().view(pydsm.REACH_INFO_DTYPE)[:n]
            ainfo = d_ainfo.cpu().numpy().view(pydsm.RAUDIT_INFO_DTYPE)[:n].copy()
            assert info.tobytes() == pinfo.tobytes(), "the audit call's search differs from the plain call's"
            am, bm = stats([r[0] for r in a_runs]), stats([r[0] for r in b_runs])
            viol = ainfo["set"]["violating"]
            res = {"audit_ms": am, "audit_enqueue_ms": stats([r[1] for r in a_runs]), "plain_ms": bm,
                   "audit_over_plain": am["median"] / bm["median"],
                   "states": int(info["states"].sum()), "max_states_seen": int(info["states"].max()),
                   "can_deadlock": int(np.count_nonzero(info["by_status"][:, 1])),
                   "can_end_incoherent": int(np.count_nonzero(viol[:, pydsm.RAUDIT_COMPLETED])),
                   "incoherent_quiescent": int(np.count_nonzero(viol[:, pydsm.RAUDIT_QUIESCENT])),
                   "truncated": int(np.count_nonzero(info["flags"] & 3)),
                   "states_per_s": int(info["states"].sum()) / (am["median"] * 1e-3),
                   "in_flight": in_flight, "scratch_allocated": scratch}
            if not a.no_loop:
                one = np.zeros(nw, dtype=np.uint64)
                aone = np.zeros(1, dtype=pydsm.RAUDIT_INFO_DTYPE)
                linfo = np.zeros((n, nw), dtype=np.uint64)
                lainfo = np.zeros(n, dtype=pydsm.RAUDIT_INFO_DTYPE)
                o1 = pydsm.ReachOpts(16, pydsm.CENSUS_DUMPS, cap, 0, 0)

                def loop():
                    torch.cuda.synchronize(dev)
                    t0 = time.perf_counter()
                    for s in range(n):
                        rc = eng.reach_audit_device(d_tr[s * NP * STRIDE:], d_cn[s * NP:], o1, one, aone, None, None, None,
                                                    None, 0, None, None, None, st)
                        assert rc == 0, rc
                        linfo[s] = one
                        lainfo[s] = aone[0]
                    torch.cuda.synchronize(dev)
                    return 1e3 * (time.perf_counter() - t0)

                lms = [loop() for _ in range(a.warmup + a.reps)][a.warmup:]
                li = linfo.view(pydsm.REACH_INFO_DTYPE).reshape(n)
                assert np.array_equal(li["states"], info["states"]) and np.array_equal(li["flags"], info["flags"])
                assert lainfo.tobytes() == ainfo.tobytes(), "the batch audit differs from the loop of dsm_reach_audit_device"
                res["loop_ms"] = stats(lms)
                res["loop_over_audit"] = res["loop_ms"]["median"] / am["median"]
            out["inputs"][dist] = res
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
