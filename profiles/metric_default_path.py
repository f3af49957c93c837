"""Times tmc2_metrics_compute_frame on frame 0 of the synthetic longdress case (profiles/metrics_options.txt): two warm-up calls, six
timed ones, one JSON line.  The package, and with it the library, comes from TMC2_PACKAGE_DIR (a copy of tmc2_amd/ next to another
build of libtmc2hip.so, e.g. the parent commit's) or from the tree; run one process per build, alternating.
    python profiles/metric_default_path.py [--modes]      # --modes: one timed pass per non-default parameter set as well"""
import hashlib
import json
import os
import sys
import time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.environ.get("TMC2_PACKAGE_DIR") or os.path.join(ROOT, "mpeg-pcc-tmc2_amd"))
import numpy as np
import tmc2_amd as T
from tmc2_amd.configs import FULL_SIZE_CASES
from tmc2_amd.synth import synth_cloud

c = FULL_SIZE_CASES["longdress_vox10_ai_r3"]
frames = [synth_cloud(c["workload"], 0)]
enc = T.GofEncoder(0, workers=1, iterations=c["iterations"], bits3d=c["bits3d"], occ_precision=c["precision"], min_w=c["min_w"],
                   min_h=c["min_h"], vox_dim=c["vox_dim"])
frs = enc.upload(frames)
enc.phase_a(frs)
enc.phase_b(frs)
res = float((1 << (c["bits3d"] - 1)) - 1)


def timed(**kw):
    t = time.perf_counter()
    q, counts = enc.per_frame(frs[:1], lambda fr, i: fr.metrics_compute(0, True, res, **kw))[0]
    return 1000.0 * (time.perf_counter() - t), q, counts


for _ in range(2):
    timed()
passes, q = [], None
for _ in range(6):
    ms, q, counts = timed()
    passes.append(round(ms, 3))
out = {"lib": T.library_path(), "points": len(frames[0][0]), "passes_ms": passes, "median_ms": float(np.median(passes)),
       "q_md5": hashlib.md5(np.ascontiguousarray(q[:, :8]).tobytes()).hexdigest(), "counts": counts.tolist()}
if "--modes" in sys.argv:
    P = T.MetricsParams
    sets = {"default_ex": P(), "hausdorff": P(compute_hausdorff=True), "dd1": P(drop_duplicates=1), "dd0": P(drop_duplicates=0),
            "np0": P(neighbors_proc=0), "np3": P(neighbors_proc=3), "np4": P(neighbors_proc=4), "no_c2c": P(compute_c2c=False),
            "no_c2p": P(compute_c2p=False), "no_color": P(compute_color=False),
            "combined": P(drop_duplicates=0, neighbors_proc=4, compute_hausdorff=True)}
    out["modes_ms"] = {}
    for name, p in sets.items():
        timed(params=p)                                   # (warm: allocations of this shape)
        ms, qq, _ = timed(params=p)
        out["modes_ms"][name] = round(ms, 3)
        if name == "default_ex":
            out["default_ex_equals_old"] = bool(np.array_equal(qq[:, :8].view(np.uint64), np.ascontiguousarray(q).view(np.uint64)))
print(json.dumps(out), flush=True)
enc.close()
