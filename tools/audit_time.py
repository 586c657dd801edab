#!/usr/bin/env python3
"""Device time of dsm_audit_run_device (words plus summary) next to dsm_census_run_nodes_device
over the same node records of a run, already in HBM (docs/PERF_LOG.md, "coherence audit"): both
stream the run's 128-byte [dump, final] lines, one lane per node.

Two runs of n systems (default 1 Mi) at np 8, 32 instructions per node, snapshots kept:
  generated    the fused generator's uniform ensemble (seed 7): about n distinct dumps per core,
               so the node census works its table (cap 2^20) -- for information;
  one_system   n copies of the ensemble's system 0 under the lock-step schedule: one outcome
               per core, the census's cheap regime and the yardstick.
Per run: warm-up rounds, then `reps` rounds that alternate census and audit, each between its
own pair of device events around `inner` back-to-back launches; the census tables and the audit
summary are zeroed before the start event.  Prints one JSON line: median / min / max / p10 / p90
in microseconds per call, audit / census of the medians, and the audit's bytes per second
(128 B per node record) as a share of the HBM peak bench.py's roofline uses.  The audit of the
first `check` systems is compared with the host audit of their records.  A bound probe follows
the generated run: those checked records tiled to n systems, audited packed (stride 1, 64 B per
record) and at the run's stride 2 (128 B per record) -- the same instructions over half and all
of the bytes, so a ratio near 1 says issue-bound and one near 0.5 memory-bound.

    python tools/audit_time.py [--n 1048576] [--reps 20] [--warmup 3] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "hp-assignment-2_amd")]

NP, N_INSTR, SEED = 8, 32, 7
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
    ap.add_argument("--check", type=int, default=256)
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    import pydsm
    if pydsm.device_count() < 1:
        raise SystemExit("audit_time: no GPU")
    n, dev = a.n, torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev).cuda_stream
    out = {"n": n, "np": NP, "bytes": 128 * NP * n, "device": torch.cuda.get_device_name(0)}
    with pydsm.Engine(NP, N_INSTR, snapshots=True) as eng:
        d_res = torch.zeros(4 * n, dtype=torch.int64, device=dev)
        d_cnt = torch.zeros(pydsm.NCOUNTERS, dtype=torch.int64, device=dev)
        d_words = torch.zeros(n, dtype=torch.int32, device=dev)
        d_aud = torch.zeros(pydsm.NAUDIT, dtype=torch.int64, device=dev)
        # system 0 of the ensemble, n times over (slack behind both buffers as Engine.explore keeps)
        d_one = torch.zeros(NP * N_INSTR + 8, dtype=torch.int16, device=dev)
        d_onec = torch.zeros(NP + 1, dtype=torch.int32, device=dev)
        eng.generate_device("uniform", SEED, N_INSTR, 0, 1, d_one.data_ptr(), d_onec.data_ptr(), st)
        d_tr = torch.zeros(n * NP * N_INSTR + 8, dtype=torch.int16, device=dev)
        d_tr[:n * NP * N_INSTR].view(n, NP * N_INSTR)[:] = d_one[:NP * N_INSTR]
        d_cn = torch.zeros(n * NP + 1, dtype=torch.int32, device=dev)
        d_cn[:n * NP].view(n, NP)[:] = d_onec[:NP]

        def run_generated():
            eng.run_generated_device("uniform", SEED, N_INSTR, 0, n, d_res, d_cnt, st)

        def run_copies():
            eng.run_packed_device(d_tr, d_cn, n, d_res, d_cnt, st)

        # (the generated run's census fills its tables: a call takes a large part of a second,
        # so it gets a fifth of the rounds)
        for name, run, cap, inner, reps, warmup in (("generated", run_generated, 1 << 20, 1, max(a.reps // 5, 1), 1),
                                                    ("one_system", run_copies, 16, 5, a.reps, a.warmup)):
            run()
            torch.cuda.synchronize()
            d_cen = torch.zeros(NP * pydsm.CENSUS_WORDS(cap), dtype=torch.int64, device=dev)

            def timed(fn):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(inner):
                    fn()
                e1.record()
                return e0, e1

            cen = lambda: eng.census_run_nodes_device(0, n, d_cen, cap, st)
            aud = lambda: eng.audit_run_device(0, n, d_words, d_aud, st)
            ev = {"census": [], "audit": []}
            for i in range(warmup + reps):
                d_cen.zero_()
                d_aud.zero_()
                pair = (timed(cen), timed(aud))
                if i >= warmup:
                    ev["census"].append(pair[0])
                    ev["audit"].append(pair[1])
            d_aud.zero_()
            aud()
            torch.cuda.synchronize()
            # the first `check` systems against the host audit of their final records
            k = min(a.check, n)
            fin = np.stack([np.stack([eng.node_state(s, c)[1] for c in range(NP)]) for s in range(k)])
            hw, _ = pydsm.audit_states(NP, fin)
            words = d_words.cpu().numpy().view(np.uint32)
            assert words[:k].tolist() == hw.tolist(), name
            summ = pydsm.audit_to_dict(d_aud.cpu().numpy().view(np.uint64))
            assert summ["systems"] == n and summ["violating"] == int(((words & 0x7F) != 0).sum()), name
            r = {k2: stats([e0.elapsed_time(e1) / inner for e0, e1 in v]) for k2, v in ev.items()}
            r["cap"], r["inner"] = cap, inner
            r["ratio"] = r["audit"]["median_us"] / r["census"]["median_us"]
            r["GBps_audit"] = 128 * NP * n / (r["audit"]["median_us"] * 1e-6) / 1e9
            r["GBps_census"] = 128 * NP * n / (r["census"]["median_us"] * 1e-6) / 1e9
            r["hbm_share_audit"] = r["GBps_audit"] / HBM_PEAK_GBS
            r["violating"], r["classes"] = summ["violating"], {c: v[0] for c, v in summ["classes"].items()}
            out[name] = r
            del d_cen
            if name != "generated":
                continue
            # Which bound: the same records (the checked ones, tiled to n systems) through
            # dsm_audit_states_device packed (64 B per record fetched) and at stride 2 (the run's
            # layout, 128-byte lines): the same instructions over half and all of the bytes.
            d_fin = torch.from_numpy(fin.reshape(k, NP * 64)).to(dev)
            probe = {}
            for stride in (1, 2):
                d_st = torch.zeros(n, stride * NP * 64, dtype=torch.uint8, device=dev)
                d_st.view(n, NP, stride * 64)[:, :, :64] = d_fin.repeat(-(-n // k), 1)[:n].view(n, NP, 64)
                fn = lambda: eng.audit_states_device(d_st, n, 0, d_words, d_aud, stride, st)
                evs = [timed(fn) for _ in range(a.warmup + a.reps)][a.warmup:]
                torch.cuda.synchronize()
                probe[f"stride{stride}"] = stats([e0.elapsed_time(e1) / inner for e0, e1 in evs])
                del d_st
            probe["stride1_over_stride2"] = probe["stride1"]["median_us"] / probe["stride2"]["median_us"]
            out["bound_probe"] = probe
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
