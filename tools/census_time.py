#!/usr/bin/env python3
"""Device time of dsm_census_device next to dsm_aggregate_device on the same result records
already in HBM (docs/PERF_LOG.md, "outcome census"): both are one pass over 32 B per system,
one lane per system.

Three inputs of n records (default 1 Mi): one outcome; the 29 outcomes of the stored test_4
exploration, drawn at random; all distinct (census table of 2^20 slots, so at n = 2^20 the
table ends full) -- and, for the table's other regime, n draws from n / 2 of those keys (about
0.43 n distinct: load 0.43).  Per input: warm-up
launches, then `reps` rounds that alternate aggregate and census, each between its own pair of
device events around `inner` back-to-back launches (10 for the few-outcome inputs, whose calls
take microseconds; 1 for all distinct, where a second call would find its keys in place); the
census table is zeroed before the start event.  Prints one JSON
line: median / min / max / p10 / p90 in microseconds per call and the census / aggregate ratio
of the medians.  The census is checked against the host census once per input.

    python tools/census_time.py [--n 1048576] [--reps 30] [--warmup 5] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "hp-assignment-2_amd"), os.path.join(REPO, "tests")]


def stats(ms):
    us = np.sort(np.asarray(ms) * 1000.0)
    q = lambda p: float(us[min(len(us) - 1, int(p * len(us)))])
    return {"median_us": float(np.median(us)), "min_us": float(us[0]), "max_us": float(us[-1]),
            "p10_us": q(0.1), "p90_us": q(0.9), "reps": len(us)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    import pydsm
    if pydsm.device_count() < 1:
        raise SystemExit("census_time: no GPU")
    rng = np.random.default_rng(1)
    f4 = np.load(os.path.join(REPO, "tests", "golden", "explore", "test_4.npy"))

    def recs(g):
        r = np.zeros(len(g), dtype=pydsm.RESULT_DTYPE)
        for i, f in enumerate(pydsm.RESULT_DTYPE.names):
            r[f] = g[:, i]
        return r

    distinct = np.zeros(a.n, dtype=pydsm.RESULT_DTYPE)
    distinct["dump_hash"] = rng.permutation(a.n).astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15)
    inputs = [("one_outcome", recs(f4[:1].repeat(a.n, 0)), 16, 10),
              ("test_4_29_outcomes", recs(f4[rng.integers(0, len(f4), a.n)]), 64, 10),
              ("all_distinct", distinct, 1 << 20, 1),
              ("half_distinct", distinct[rng.integers(0, max(a.n // 2, 1), a.n)], 1 << 20, 1)]
    out = {"n": a.n, "bytes": 32 * a.n, "kind": "dumps", "device": torch.cuda.get_device_name(0)}
    st = torch.cuda.current_stream().cuda_stream
    with pydsm.Engine(4, 32) as eng:
        for name, res, cap, inner in inputs:
            d_res = torch.from_numpy(res.view(np.uint8).reshape(-1).copy()).cuda()
            d_cen = torch.zeros(pydsm.CENSUS_WORDS(cap), dtype=torch.int64, device="cuda")
            d_agg = torch.zeros(pydsm.NAGG, dtype=torch.int64, device="cuda")

            def timed(fn):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(inner):
                    fn()
                e1.record()
                return e0, e1

            agg = lambda: eng.aggregate_device(d_res, a.n, 0, d_agg, st)
            cen = lambda: eng.census_device(d_res, a.n, 0, "dumps", d_cen, cap, st)
            ev = {"aggregate": [], "census": []}
            for i in range(a.warmup + a.reps):
                d_cen.zero_()
                pair = (timed(agg), timed(cen))
                if i >= a.warmup:
                    ev["aggregate"].append(pair[0])
                    ev["census"].append(pair[1])
            d_cen.zero_()
            cen()
            torch.cuda.synchronize()
            want = pydsm.census_results(res, "dumps", cap)
            got = d_cen.cpu().numpy().view(np.uint64)
            if a.n <= cap:      # an overfull table's survivors are free
                assert pydsm.census_header(got) == pydsm.census_header(want), name
                assert pydsm.census_sorted(got, cap).tobytes() == pydsm.census_sorted(want, cap).tobytes(), name
            r = {k: stats([e0.elapsed_time(e1) / inner for e0, e1 in v]) for k, v in ev.items()}
            r["cap"], r["inner"] = cap, inner
            r["ratio"] = r["census"]["median_us"] / r["aggregate"]["median_us"]
            r["GBps_census"] = 32 * a.n / (r["census"]["median_us"] * 1e-6) / 1e9
            out[name] = r
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
