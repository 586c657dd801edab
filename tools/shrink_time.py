#!/usr/bin/env python3
"""Time of the test shrinker on the GPU (dsm_shrink_many_device; DESIGN.md, "Shrink") against the
loop a user could write without it, in one process.

Ensemble: the 11 systems of generate(4, "hot", seed 11, n_instr 1, first 0, 64) that can deadlock,
tiled to `--systems` systems (default 1024), shrunk under the deadlock property.

  (a) one dsm_shrink_many_device call: every round's candidates of all systems in one launch;
  (b) the yardstick: per system and per round one Engine.reach_audit_many over that round's
      candidates, which the host builds, and the host picks -- the same rule, with what the library
      offered before the shrinker.

Per call: `warmup` runs, then `reps` timed ones, wall time from a synchronised device to the call's
return (both are synchronous).  Before anything is reported (a)'s traces, counts and rounds equal
(b)'s, system by system.  A last run of (a) under DSM_SHRINK_TIMING=1 gives the split by phase (plan
with its scan and read-back, build, search, pick); it waits after every phase, so its total is no
measurement of the call.

Prints one JSON line: min / max / median milliseconds and every run of (a) and (b), the ratio of the
medians, the rounds, candidates and states of the ensemble, and the phase split.

    python tools/shrink_time.py [--systems 1024] [--max-states 65536] [--reps 5] [--warmup 2]
                                [--yard-reps 3] [--yard-warmup 1] [--out FILE]
"""
import argparse
import ctypes
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


def yardstick(eng, tr, cn, cap):
    """The rule of include/dsm.h's "shrink" section for the deadlock property, a system and a round at
    a time over Engine.reach_audit_many -> (traces, counts, rounds)."""
    out_t, out_c = tr.copy(), cn.copy()
    rounds = np.zeros(len(tr), np.uint32)
    for s in range(len(tr)):
        cores = [[int(w) for w in tr[s, c, :cn[s, c]]] for c in range(NP)]
        r = eng.reach_audit_many(tr[s:s + 1], cn[s:s + 1], max_states=cap, term_cap=1)
        if not r["can_deadlock"][0] or not any(cores):
            continue
        g = 1
        while 2 * g <= max(len(p) for p in cores):
            g *= 2
        while True:
            cands = [(c, k * g, min(g, len(p) - k * g)) for c, p in enumerate(cores) for k in range((len(p) + g - 1) // g)]
            ct = np.zeros((len(cands), NP, STRIDE), np.uint16)
            cc = np.zeros((len(cands), NP), np.uint32)
            for i, (c, start, ln) in enumerate(cands):
                for q, p in enumerate(cores):
                    cut = p[:start] + p[start + ln:] if q == c else p
                    ct[i, q, :len(cut)] = cut
                    cc[i, q] = len(cut)
            r = eng.reach_audit_many(ct, cc, max_states=cap, term_cap=1)
            rounds[s] += 1
            found = np.flatnonzero(r["can_deadlock"])
            if len(found):
                c, start, ln = cands[int(found[0])]
                cores[c] = cores[c][:start] + cores[c][start + ln:]
                longest = max(len(p) for p in cores)
                while g > 1 and g > longest:
                    g //= 2
                if longest == 0:
                    break
            else:
                if g == 1:
                    break
                g //= 2
        out_t[s] = 0
        for c, p in enumerate(cores):
            out_t[s, c, :len(p)] = p
            out_c[s, c] = len(p)
    return out_t, out_c, rounds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--systems", type=int, default=1024)
    ap.add_argument("--max-states", type=int, default=1 << 16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--yard-reps", type=int, default=3)
    ap.add_argument("--yard-warmup", type=int, default=1)
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    import pydsm
    import pyoracle as orc
    if pydsm.device_count() < 1:
        raise SystemExit("shrink_time: no GPU")
    dev = torch.device("cuda", 0)
    n, cap = a.systems, a.max_states
    g_tr, g_cn = orc.generate(NP, "hot", 11, 1, 0, 64)
    pad = np.zeros((64, NP, STRIDE), dtype=np.uint16)
    pad[:, :, :1] = g_tr
    flagged = np.flatnonzero(pydsm.reach_many(NP, pad, g_cn, max_states=cap)["can_deadlock"])
    pick = flagged[np.arange(n) % len(flagged)]
    tr, cn = np.ascontiguousarray(pad[pick]), np.ascontiguousarray(g_cn[pick], dtype=np.uint32)
    out = {"systems": n, "distinct": len(flagged), "max_states": cap, "device": torch.cuda.get_device_name(0)}
    with pydsm.Engine(NP, STRIDE) as eng:
        st = torch.cuda.current_stream(dev).cuda_stream
        d_tr = torch.from_numpy(tr.view(np.int16).reshape(-1)).to(dev)
        d_cn = torch.from_numpy(cn.view(np.int32).reshape(-1)).to(dev)
        d_out = torch.zeros(tr.size, dtype=torch.int16, device=dev)
        d_ocn = torch.zeros(cn.size, dtype=torch.int32, device=dev)
        d_orig = torch.zeros(tr.size, dtype=torch.int16, device=dev)
        info = np.zeros(n, dtype=pydsm.SHRINK_INFO_DTYPE)
        opts = pydsm.ReachOpts(16, pydsm.CENSUS_DUMPS, cap, 0, 0)
        so = pydsm.shrink_opts("deadlock")

        def ensemble():
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            rc = eng.shrink_many_device(d_tr, d_cn, n, opts, so, d_out, d_ocn, d_orig, info, None, 0, 0, st)
            t1 = time.perf_counter()
            assert rc == 0, rc
            return 1e3 * (t1 - t0)

        a_ms = [ensemble() for _ in range(a.warmup + a.reps)][a.warmup:]
        in_flight, scratch = eng.reach_batch_state()
        got_t = d_out.cpu().numpy().view(np.uint16).reshape(tr.shape)
        got_c = d_ocn.cpu().numpy().view(np.uint32).reshape(cn.shape)

        def yard():
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            res = yardstick(eng, tr, cn, cap)
            return 1e3 * (time.perf_counter() - t0), res

        y_runs = [yard() for _ in range(a.yard_warmup + a.yard_reps)][a.yard_warmup:]
        y_t, y_c, y_rounds = y_runs[-1][1]
        assert np.array_equal(y_t, got_t) and np.array_equal(y_c, got_c), "the ensemble call differs from the yardstick loop"
        assert np.array_equal(y_rounds, info["rounds"])
        os.environ["DSM_SHRINK_TIMING"] = "1"
        ensemble()
        del os.environ["DSM_SHRINK_TIMING"]
        ms = (ctypes.c_double * 4)()
        rounds = ctypes.c_uint64(0)
        assert pydsm.lib().dsm_debug_shrink_times(ms, ctypes.byref(rounds)) == 0
        am, ym = stats(a_ms), stats([r[0] for r in y_runs])
        out.update({"ensemble_ms": am, "yardstick_ms": ym, "yardstick_over_ensemble": ym["median"] / am["median"],
                    "rounds": int(info["rounds"].max()), "device_rounds": int(rounds.value),
                    "candidates": int(info["candidates"].sum()), "states": int((info["states"] + info["root_states"]).sum()),
                    "instrs_in": int(info["instrs_in"].sum()), "instrs_out": int(info["instrs_out"].sum()),
                    "yardstick_calls": int(n + y_rounds.sum()),
                    "phase_ms": dict(zip(("plan", "build", "search", "pick"), (round(float(x), 3) for x in ms))),
                    "in_flight": in_flight, "scratch_allocated": scratch})
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
