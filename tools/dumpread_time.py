#!/usr/bin/env python3
"""Device time of dsm_parse_dumps_device (the dump reader, unfmt_kernel) next to
dsm_format_dumps_device (the formatter, fmt_kernel) on the same buffers in the same session
(docs/PERF_LOG.md, "dump reader"): the reader loads the slot bytes the formatter stores and writes
3% as much, so the formatter's time is its yardstick.

n records (default 1 Mi) at np 8: the dump records of a generated uniform run (seed 7, 32
instructions per node) tiled to n, formatted once into n slots of DSM_DUMP_SLOT bytes (2 GiB at
the default).  Warm-up rounds, then `reps` rounds that alternate formatter and reader, each
between its own pair of device events around `inner` back-to-back launches.  Prints one JSON
line: median / min / max / p10 / p90 in microseconds per call of both, reader / formatter of the
medians, and both kernels' bytes per second over the slot bytes, also as a share of the HBM peak
bench.py's roofline uses.  Before timing, the records read back are compared with the records
formatted (bytes 0..59), every status must be 0, and the first `check` slots go through
dsm_parse_dump on the host.

    python tools/dumpread_time.py [--n 1048576] [--reps 20] [--warmup 3] [--inner 3] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "hp-assignment-2_amd")]

NP, N_INSTR, SEED, N_RUN = 8, 32, 7, 1024
HBM_PEAK_GBS = 8000.0       # bench.py HBM_PEAK_GBS


def stats(ms):
    us = np.sort(np.asarray(ms) * 1000.0)
    q = lambda p: float(us[min(len(us) - 1, int(p * len(us)))])
    return {"median_us": float(np.median(us)), "min_us": float(us[0]), "max_us": float(us[-1]),
            "p10_us": q(0.1), "p90_us": q(0.9), "reps": len(us)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--check", type=int, default=256)
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    import pydsm
    if pydsm.device_count() < 1:
        raise SystemExit("dumpread_time: no GPU")
    n, dev = a.n, torch.device("cuda", 0)
    assert n % NP == 0
    st = torch.cuda.current_stream(dev).cuda_stream
    out = {"n": n, "np": NP, "slot_bytes": pydsm.DUMP_SLOT * n, "device": torch.cuda.get_device_name(0)}
    with pydsm.Engine(NP, N_INSTR, snapshots=True) as eng:
        # the dump records of a small generated run, tiled to n records (record k is node k % np)
        eng.run_generated("uniform", SEED, N_INSTR, 0, N_RUN)
        small = np.stack([eng.node_state(s, c)[0] for s in range(N_RUN) for c in range(NP)])
        small[:, 32:48] = np.minimum(small[:, 32:48], 2)
        small[:, 56:60] = np.minimum(small[:, 56:60], 3)
        d_small = torch.from_numpy(small).to(dev)
        d_recs = d_small.repeat(-(-n // len(small)), 1)[:n].contiguous()
        d_text = torch.zeros(n * pydsm.DUMP_SLOT, dtype=torch.uint8, device=dev)
        d_len = torch.zeros(n, dtype=torch.int32, device=dev)
        d_back = torch.zeros(n, 64, dtype=torch.uint8, device=dev)
        d_status = torch.full((n,), -1, dtype=torch.int32, device=dev)
        fmt = lambda: eng.format_dumps_device(d_recs.data_ptr(), n, d_text.data_ptr(), d_len.data_ptr(), 1, st)
        rd = lambda: eng.parse_dumps_device(d_text, d_len, n, d_back, d_status, 1, st)
        fmt()
        rd()
        torch.cuda.synchronize()
        assert int(d_status.abs().max()) == 0, "a formatted slot was refused"
        assert bool((d_back[:, :60] == d_recs[:, :60]).all()), "records read differ from records formatted"
        k = min(a.check, n)
        lens = d_len[:k].cpu().numpy()
        text = d_text[:k * pydsm.DUMP_SLOT].cpu().numpy().reshape(k, pydsm.DUMP_SLOT)
        back = d_back[:k].cpu().numpy()
        for i in range(k):
            node, rec = pydsm.parse_dump(bytes(text[i, :lens[i]]))
            assert node == i % NP and rec.tobytes() == back[i].tobytes(), i
        out["layouts"] = len({bytes(x) for x in (small[:, 56:60] == 1)})

        def timed(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.inner):
                fn()
            e1.record()
            return e0, e1

        ev = {"format": [], "read": []}
        for i in range(a.warmup + a.reps):
            pair = (timed(fmt), timed(rd))
            if i >= a.warmup:
                ev["format"].append(pair[0])
                ev["read"].append(pair[1])
        torch.cuda.synchronize()
        for name, v in ev.items():
            r = stats([e0.elapsed_time(e1) / a.inner for e0, e1 in v])
            r["GBps"] = pydsm.DUMP_SLOT * n / (r["median_us"] * 1e-6) / 1e9
            r["GBps_best"] = pydsm.DUMP_SLOT * n / (r["min_us"] * 1e-6) / 1e9
            r["hbm_share"] = r["GBps"] / HBM_PEAK_GBS
            out[name] = r
        out["inner"] = a.inner
        out["ratio"] = out["read"]["median_us"] / out["format"]["median_us"]
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
