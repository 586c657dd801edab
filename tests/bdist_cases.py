"""The reach batch distribution's cases (a helper module beside raudit_cases.py): batches stacked
from fate_cases.py's systems and the generator's hot ensemble, the host loop of each
(pydsm.reach_dist_many = dsm_reach_batch_dist, computed once per argument set and shared
read-only), the figures pinned from the host reference, and the comparison both test files use."""
import numpy as np

import pydsm as dsm
import pyoracle as orc
import raudit_cases as ra
import reach_cases as rc

T3 = (0x8000, 0x1000, 65536)
T16 = tuple(1 + 4369 * j for j in range(15)) + (65536,)       # 16 thresholds, 1 and 65536 among them
GEN_STRIDE = 8                 # the generator's one-instruction systems, padded to the smallest max_instr
HOT_DEADLOCKERS = [16, 21, 24, 28, 30, 31, 34, 45, 50, 55, 61]
HOT_DEADLOCK_MASS = [5600667286118713699, 2578366727733555006, 2747255254561792257, 534885257310912791,
                     2181253775212247885, 1863754535723892359, 4117577664058704075, 4577326193865070301,
                     3441522829276040448, 3510388711085215937, 3116606835071423307]
# edges and rounds at threshold 0x8000, from the host reference
EDGES_ROUNDS = {"S4": (2908, 19), "C3": (129454, 29), "E": (142205, 38), "X": (700, 12), "L2": (116336, 29),
                "L1": (58549, 29), "S8": (273508, 23), "C2x8": (523332, 25)}
_cache = {}


def stack(names):
    return (np.stack([ra.CASES[k][1] for k in names]), np.stack([ra.CASES[k][2] for k in names]))


def idle():
    return np.zeros((4, rc.STRIDE), np.uint16), np.zeros(4, np.uint32)


def hot():
    """generate(4, "hot", seed 11, n_instr 1, first 0, 64), traces [64, 4, GEN_STRIDE]."""
    if "hot" not in _cache:
        tr, cn = orc.generate(4, "hot", 11, 1, 0, 64)
        pad = np.zeros((64, 4, GEN_STRIDE), dtype=np.uint16)
        pad[:, :, :1] = tr
        _cache["hot"] = (pad, cn)
    return _cache["hot"]


def host(key, np_, tr, cn, **kw):
    """pydsm.reach_dist_many (dsm_reach_batch_dist, the host loop) of a batch, once per key."""
    if ("host", key) not in _cache:
        kw.setdefault("term_cap", 256)
        _cache["host", key] = dsm.reach_dist_many(np_, tr, cn, witnesses=True, **kw)
    return _cache["host", key]


def same(d, h, which=None):
    """A batch distribution result (a dict with info, dinfo, terminals, term_mass, parents, masks;
    any may be None) equals the host loop's bit for bit, for the systems in `which` (all)."""
    n = len(h["info"])
    assert (h["info"]["fp_collisions"] == 0).all()
    if d["info"] is not None:
        assert len(d["info"]) == n and (d["info"]["fp_collisions"] == 0).all()
        assert d["info"].tobytes() == h["info"].tobytes(), [s for s in range(n) if d["info"][s] != h["info"][s]][:8]
    if d["dinfo"] is not None:
        assert d["dinfo"].shape == h["dinfo"].shape
        assert d["dinfo"].tobytes() == h["dinfo"].tobytes(), \
            [(s, d["dinfo"][s], h["dinfo"][s]) for s in range(n) if d["dinfo"][s].tobytes() != h["dinfo"][s].tobytes()][:2]
    for s in (range(n) if which is None else which):
        for k in ("terminals", "term_mass", "parents", "masks"):
            if d.get(k) is not None and h.get(k) is not None:
                assert d[k][s].shape == h[k][s].shape and d[k][s].tobytes() == h[k][s].tobytes(), (k, s)
