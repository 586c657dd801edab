#!/usr/bin/env python3
"""Writes tests/golden/events: the reference's own DEBUG_INSTR text of the event trace's variants
(tests/event_cases.py), as recorded output only.

Run where oracle/_ref is built (make -C oracle ref).  Every variant goes through
oracle/_ref/ref_lockstep_np{4,8}_dbg `packed` -- the reference's handler, issue and replacement
text with its DEBUG_INSTR printfs, under the variant's seeded schedule, inbox limit and round limit
-- and one u64 per system is stored: reference_pins.text_digest of that system's stdout.  For the
five tests/golden/inputs directories the text itself is stored (<test>_instr.txt).  index.json
holds the input's sha256 and the number of systems per variant."""
import json
import os
import sys
import tempfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("tests", "oracle", "hp-assignment-2_amd"):
    sys.path.insert(0, os.path.join(REPO, p))

import adversarial as adv          # noqa: E402
import event_cases as ec           # noqa: E402
import pyoracle as orc             # noqa: E402
import reference_pins as rp        # noqa: E402


def main():
    os.makedirs(ec.DIR, exist_ok=True)
    idx = {"variants": {}, "inputs": {}}
    with tempfile.TemporaryDirectory() as tmp:
        for name, v in ec.VARIANTS.items():
            exe, why = rp.ref_packed(v["np"], dbg=True)
            if exe is None:
                sys.exit(f"gen_event_fixtures: {why}")
            tr, cn = ec.inputs(v)
            seed, thresh = rp.sched(v)
            d = ec.ref_systems(exe, v["np"], tr, cn, tmp, seed, thresh, v["cap"], v["limit"])
            np.save(os.path.join(ec.DIR, name + ".npy"), d)
            idx["variants"][name] = {"systems": int(len(d)), "input_sha256": adv.digest(tr, cn)}
            print(f"{name}: {len(d)} systems", flush=True)
        exe, why = rp.ref_packed(4, dbg=True)
        for test in ec.INPUT_DIRS:
            tr, cn = orc.load_test(os.path.join(REPO, "tests", "golden", "inputs", test))
            text = ec.ref_systems(exe, 4, tr.reshape(1, 4, -1), cn.reshape(1, 4), tmp, keep_text=True)[0]
            with open(os.path.join(ec.DIR, test + "_instr.txt"), "wb") as f:
                f.write(text)
            idx["inputs"][test] = {"bytes": len(text), "digest": "0x%016x" % rp.text_digest(text)}
            print(f"{test}: {len(text)} bytes", flush=True)
    with open(os.path.join(ec.DIR, "index.json"), "w") as f:
        json.dump(idx, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
