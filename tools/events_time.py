#!/usr/bin/env python3
"""Device time of the event trace's replay (dsm_trace_events_device, event_cap 0: counts, hashes
and results only) next to dsm_run_packed_device on the same ensemble, already in HBM (DESIGN.md,
"Event trace"): n explored variants (default 1 Mi) of tests/sample -- n copies of the system under
the seeded schedule, variant i with schedule id i, as cache_simulator --explore runs them.

Warm-up rounds, then `reps` rounds that alternate the engine's run and the replay, each between
its own pair of device events.  Prints one JSON line: median / min / max / p10 / p90 in
milliseconds per call for both, replay / engine of the medians, and the replay's events per
second.  The replay's results must equal the engine's on all n systems.

    python tools/events_time.py [--n 1048576] [--reps 10] [--warmup 2] [--seed 7] [--thresh 32768] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "hp-assignment-2_amd"), os.path.join(REPO, "oracle")]

NP, STRIDE = 4, 32


def stats(ms):
    ms = np.sort(np.asarray(ms, dtype=np.float64))
    q = lambda p: float(ms[min(len(ms) - 1, int(p * len(ms)))])
    return {"median_ms": float(np.median(ms)), "min_ms": float(ms[0]), "max_ms": float(ms[-1]),
            "p10_ms": q(0.1), "p90_ms": q(0.9), "reps": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--thresh", type=int, default=0x8000)
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    import pydsm
    import pyoracle as orc
    if pydsm.device_count() < 1:
        raise SystemExit("events_time: no GPU")
    n, dev = a.n, torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev).cuda_stream
    tr, cn = orc.load_test(os.path.join(REPO, "tests", "golden", "inputs", "sample"))
    tr = np.ascontiguousarray(tr, dtype=np.uint16).reshape(NP * STRIDE)
    cn = np.ascontiguousarray(cn, dtype=np.uint32).reshape(NP)
    out = {"n": n, "np": NP, "seed": a.seed, "thresh": a.thresh, "device": torch.cuda.get_device_name(0)}
    with pydsm.Engine(NP, STRIDE) as eng:
        eng.set_schedule(a.seed, a.thresh)
        # n copies of the system (slack behind both buffers as Engine.explore keeps)
        d_tr = torch.zeros(n * NP * STRIDE + 8, dtype=torch.int16, device=dev)
        d_tr[:n * NP * STRIDE].view(n, NP * STRIDE)[:] = torch.from_numpy(tr.view(np.int16).copy()).to(dev)
        d_cn = torch.zeros(n * NP + 1, dtype=torch.int32, device=dev)
        d_cn[:n * NP].view(n, NP)[:] = torch.from_numpy(cn.view(np.int32).copy()).to(dev)
        d_res = torch.zeros(4 * n, dtype=torch.int64, device=dev)
        d_cnt = torch.zeros(pydsm.NCOUNTERS, dtype=torch.int64, device=dev)
        d_res2 = torch.zeros(4 * n, dtype=torch.int64, device=dev)
        d_n = torch.zeros(n, dtype=torch.int32, device=dev)
        d_h = torch.zeros(n, dtype=torch.int64, device=dev)

        def timed(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            return e0, e1

        engine = lambda: eng.run_packed_device(d_tr, d_cn, n, d_res, d_cnt, st)
        replay = lambda: eng.trace_events_device(d_tr, d_cn, n, None, n, None, 0, d_n, d_h, d_res2, st)
        ev = {"engine": [], "replay": []}
        for i in range(a.warmup + a.reps):
            pair = (timed(engine), timed(replay))
            if i >= a.warmup:
                ev["engine"].append(pair[0])
                ev["replay"].append(pair[1])
        torch.cuda.synchronize()
        assert torch.equal(d_res, d_res2), "the replay's results differ from the engine's"
        events = int(d_n.sum(dtype=torch.int64).item())
        for k, v in ev.items():
            out[k] = stats([e0.elapsed_time(e1) for e0, e1 in v])
        out["events"] = events
        out["ratio"] = out["replay"]["median_ms"] / out["engine"]["median_ms"]
        out["events_per_s"] = events / (out["replay"]["median_ms"] * 1e-3)
        out["lanes"] = min(-(-n // 64) * 64, pydsm.EVENTS_MAX_LANES)
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
