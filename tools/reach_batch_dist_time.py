#!/usr/bin/env python3
"""Time of the reach batch distribution (dsm_reach_batch_dist_device; DESIGN.md, "Reach batch
distribution") in one process, by tools/reach_batch_time.py's method and on its inputs: the
generator's 512 one-instruction four-node systems generate(4, dist, seed 11, n_instr 1, first 0,
512) for dist uniform and hot.  Three calls are compared:

  (a) the dist call with 1 threshold (0x8000) and with 4 (0x8000, 0x4000, 0x2000, 0x1000), writing
      info and dinfo alone (every row output NULL);
  (b) the plain dsm_reach_batch_device, writing the info alone;
  (c) a loop of the synchronous dsm_reach_dist_device, once per system, writing rinfo and dinfo
      (1 threshold).

Per input and call: `warmup` calls, then `reps` timed ones.  (a) and (b) are asynchronous, so a
timed call is wall time from a synchronised stream to the stream synchronised again, every buffer
and the ctx's scratch already there.  Before anything is reported (a)'s info equals (b)'s, and
(a)'s dinfo equals (c)'s, system by system.

Prints one JSON line: per input the min / max / median milliseconds of each call, every call's in
order, the ratios (a)/(b) and (c)/(a) of the medians, the edges, the deadlockers, the systems (a)
kept in flight and the bytes of its scratch; the slab sizes of both forms.

    python tools/reach_batch_dist_time.py [--dist uniform,hot] [--systems 512] [--max-states 65536] [--chunk 0]
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
T1, T4 = (0x8000,), (0x8000, 0x4000, 0x2000, 0x1000)


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
        raise SystemExit("reach_batch_dist_time: no GPU")
    dev = torch.device("cuda", 0)
    n, cap = a.systems, a.max_states
    out = {"systems": n, "max_states": cap, "chunk": a.chunk, "scratch_bytes": a.scratch_bytes,
           "slab_bytes": pydsm.reach_batch_slab_bytes(NP, max_states=cap, chunk=a.chunk),
           "dist_slab_bytes": pydsm.reach_batch_dist_slab_bytes(NP, max_states=cap, chunk=a.chunk),
           "device": torch.cuda.get_device_name(0), "inputs": {}}
    nw, dw = len(pydsm.REACH_INFO_FIELDS), len(pydsm.DIST_INFO_FIELDS)
    with pydsm.Engine(NP, STRIDE) as eng:
        st = torch.cuda.current_stream(dev).cuda_stream
        d_info = torch.zeros(n * nw, dtype=torch.int64, device=dev)
        d_pinfo = torch.zeros(n * nw, dtype=torch.int64, device=dev)
        d_dinfo = torch.zeros(n * len(T4) * dw, dtype=torch.int64, device=dev)
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

            def dist_call(th):
                dopts = pydsm.dist_batch_opts(th)
                return lambda: eng.reach_batch_dist_device(d_tr, d_cn, n, opts, dopts, d_info, d_dinfo, None, None, 0, None, None,
                                                           a.scratch_bytes, st)

            def plain():
                return eng.reach_batch_device(d_tr, d_cn, n, opts, d_pinfo, None, 0, None, None, a.scratch_bytes, st)

            a4 = [timed(dist_call(T4)) for _ in range(a.warmup + a.reps)][a.warmup:]
            dinfo4 = d_dinfo.cpu().numpy().view(pydsm.DIST_INFO_DTYPE)[:n * 4].reshape(n, 4).copy()
            a1 = [timed(dist_call(T1)) for _ in range(a.warmup + a.reps)][a.warmup:]
            in_flight, scratch = eng.reach_batch_state()
            b_runs = [timed(plain) for _ in range(a.warmup + a.reps)][a.warmup:]
            info = d_info.cpu().numpy().view(pydsm.REACH_INFO_DTYPE)[:n].copy()
            pinfo = d_pinfo.cpu().numpy().view(pydsm.REACH_INFO_DTYPE)[:n]
            dinfo = d_dinfo.cpu().numpy().view(pydsm.DIST_INFO_DTYPE)[:n].copy()
            assert info.tobytes() == pinfo.tobytes(), "the dist call's search differs from the plain call's"
            assert dinfo4[:, 0].tobytes() == dinfo.tobytes(), "the first of four thresholds differs from the one alone"
            m1, m4, bm = stats([r[0] for r in a1]), stats([r[0] for r in a4]), stats([r[0] for r in b_runs])
            res = {"dist1_ms": m1, "dist4_ms": m4, "dist1_enqueue_ms": stats([r[1] for r in a1]), "plain_ms": bm,
                   "dist1_over_plain": m1["median"] / bm["median"], "dist4_over_plain": m4["median"] / bm["median"],
                   "states": int(info["states"].sum()), "max_states_seen": int(info["states"].max()),
                   "edges": int(dinfo["edges"].sum()), "rounds_sum": int(dinfo["rounds"].sum()),
                   "edge_visits_full": int((dinfo["edges"] * dinfo["rounds"]).sum()),
                   "can_deadlock": int(np.count_nonzero(info["by_status"][:, 1])),
                   "p_deadlock_max": float(dinfo["by_status"][:, 1].max()) / float(pydsm.DIST_ONE),
                   "flagged": int(np.count_nonzero(dinfo["flags"] & pydsm.DIST_F_EDGES)),
                   "truncated": int(np.count_nonzero(info["flags"] & 3)),
                   "in_flight": in_flight, "scratch_allocated": scratch}
            if not a.no_loop:
                one = np.zeros(nw, dtype=np.uint64)
                done = np.zeros((1, dw), dtype=np.uint64)
                ldinfo = np.zeros((n, dw), dtype=np.uint64)
                th = np.array(T1, dtype=np.uint32)
                o1 = pydsm.ReachOpts(16, pydsm.CENSUS_DUMPS, cap, 0, 0)

                def loop():
                    torch.cuda.synchronize(dev)
                    t0 = time.perf_counter()
                    for s in range(n):
                        rc = eng.reach_dist_device(d_tr[s * NP * STRIDE:], d_cn[s * NP:], o1, th, 0, one, done, None, None, 0,
                                                   None, st)
                        assert rc == 0, rc
                        ldinfo[s] = done[0]
                    torch.cuda.synchronize(dev)
                    return 1e3 * (time.perf_counter() - t0)

                lms = [loop() for _ in range(a.warmup + a.reps)][a.warmup:]
                assert ldinfo.tobytes() == dinfo.tobytes(), "the batch distribution differs from the loop of dsm_reach_dist_device"
                res["loop_ms"] = stats(lms)
                res["loop_over_dist1"] = res["loop_ms"]["median"] / m1["median"]
            out["inputs"][dist] = res
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
