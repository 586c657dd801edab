#!/usr/bin/env python3
"""Device time of the access profile (dsm_profile_runs_device: node profiles, summary and results)
next to the event trace's replay (dsm_trace_events_device, event_cap 0) and dsm_run_packed_device
on the same ensemble, already in HBM ("profile_kernel"): n explored variants (default
1 Mi) of tests/sample -- n copies of the system under the seeded schedule, variant i with schedule
id i, as cache_simulator --explore runs them.

Warm-up rounds, then `reps` rounds that alternate the engine's run, the replay and the profile, each
between its own pair of device events.  Prints one JSON line per invocation: median / min / max /
p10 / p90 in milliseconds per call for all three (and for the profile without per-node records), profile / replay and profile / engine of the
medians with the spread the rounds allow (min / max and max / min), and the summary's totals.  The
profile's and the replay's results must equal the engine's on all n systems, and the summary's
accesses the engine's instruction count.

The measuring runs in a child process per invocation, each under its own time limit; after a child
that fails or runs out of time nothing more is started.

    python tools/profile_time.py [--n 1048576] [--reps 10] [--warmup 2] [--seed 7] [--thresh 32768]
                                 [--invocations 2] [--limit 240] [--out FILE]
"""
import argparse
import json
import os
import subprocess
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


def ratio(a, b):
    """a / b of the medians, and the least and most the rounds allow"""
    return {"median": a["median_ms"] / b["median_ms"], "min": a["min_ms"] / b["max_ms"], "max": a["max_ms"] / b["min_ms"]}


def measure(a):
    import torch
    import pydsm
    import pyoracle as orc
    if pydsm.device_count() < 1:
        raise SystemExit("profile_time: no GPU")
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
        d_res3 = torch.zeros(4 * n, dtype=torch.int64, device=dev)
        d_np = torch.zeros(8 * NP * n, dtype=torch.int64, device=dev)
        d_pf = torch.zeros(pydsm.NPROFILE, dtype=torch.int64, device=dev)
        d_scratch_pf = torch.zeros(pydsm.NPROFILE, dtype=torch.int64, device=dev)

        def timed(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            return e0, e1

        calls = {"engine": lambda: eng.run_packed_device(d_tr, d_cn, n, d_res, d_cnt, st),
                 "replay": lambda: eng.trace_events_device(d_tr, d_cn, n, None, n, None, 0, d_n, d_h, d_res2, st),
                 "profile": lambda: eng.profile_device(d_tr, d_cn, n, None, n, d_np, d_pf, d_res3, st),
                 # the summary alone: no per-node records written
                 "profile_summary": lambda: eng.profile_device(d_tr, d_cn, n, None, n, None, d_scratch_pf, None, st)}
        ev = {k: [] for k in calls}
        for i in range(a.warmup + a.reps):
            d_pf.zero_()                    # the summary is accumulated into: one round's at the end
            trio = {k: timed(f) for k, f in calls.items()}
            if i >= a.warmup:
                for k, v in trio.items():
                    ev[k].append(v)
        torch.cuda.synchronize()
        assert torch.equal(d_res, d_res2), "the replay's results differ from the engine's"
        assert torch.equal(d_res, d_res3), "the profile's results differ from the engine's"
        for k, v in ev.items():
            out[k] = stats([e0.elapsed_time(e1) for e0, e1 in v])
        summary = pydsm.profile_to_dict(d_pf.cpu().numpy().view(np.uint64))
        res = d_res.cpu().numpy().view(pydsm.RESULT_DTYPE)
        assert summary["systems"] == n and summary["accesses"] == int(res["instrs"].astype(np.int64).sum())
        assert summary["totals"]["recv"] == int(res["msgs"].astype(np.int64).sum())
        out["profile_vs_replay"] = ratio(out["profile"], out["replay"])
        out["profile_vs_engine"] = ratio(out["profile"], out["engine"])
        out["replay_vs_engine"] = ratio(out["replay"], out["engine"])
        out["accesses"] = summary["accesses"]
        out["accesses_per_s"] = summary["accesses"] / (out["profile"]["median_ms"] * 1e-3)
        out["summary"] = {k: summary[k] for k in ("hits", "hit_ratio", "misses", "txns", "mean_latency", "max_latency", "open")}
        out["lanes"] = min(-(-n // 64) * 64, pydsm.EVENTS_MAX_LANES)
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--thresh", type=int, default=0x8000)
    ap.add_argument("--invocations", type=int, default=2)
    ap.add_argument("--limit", type=int, default=240, help="seconds each invocation may take")
    ap.add_argument("--out")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return measure(a)
    lines = []
    for _ in range(a.invocations):          # a fresh process each: its own context, allocations and clocks
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--n", str(a.n), "--reps", str(a.reps),
               "--warmup", str(a.warmup), "--seed", str(a.seed), "--thresh", str(a.thresh)]
        try:
            r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=a.limit)
        except subprocess.TimeoutExpired:
            raise SystemExit(f"profile_time: an invocation ran past {a.limit} s; nothing more is started")
        if r.returncode:
            raise SystemExit(f"profile_time: an invocation ended with status {r.returncode}; nothing more is started")
        line = r.stdout.strip().splitlines()[-1]
        print(line, flush=True)
        lines.append(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
