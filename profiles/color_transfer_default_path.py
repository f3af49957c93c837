"""Times S18 inside tmc2_encoder_generate_attribute_images on frame 0 of the synthetic longdress case
(profiles/color_transfer_options.txt): the device's own stage timers of the two searches and of `transfer_colors`, two warm-up calls, six
timed ones, one JSON line.  The package, and with it the library, comes from TMC2_PACKAGE_DIR (a copy of tmc2_amd/ next to another
build of libtmc2hip.so, e.g. the parent commit's) or from the tree; run one process per build, alternating.
    python profiles/color_transfer_default_path.py [--modes]   # --modes: one timed pass per non-default family as well"""
import hashlib
import json
import os
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.environ.get("TMC2_PACKAGE_DIR") or os.path.join(ROOT, "mpeg-pcc-tmc2_amd"))
import numpy as np
import tmc2_amd as T
from tmc2_amd.configs import FULL_SIZE_CASES
from tmc2_amd.synth import synth_cloud

S18 = ("knn8_recon_in_source", "knn1_source_in_recon", "knn_recon_in_source", "knn_source_in_recon", "transfer_colors")
c = FULL_SIZE_CASES["longdress_vox10_ai_r3"]
frames = [synth_cloud(c["workload"], 0)]
enc = T.GofEncoder(0, workers=1, iterations=c["iterations"], bits3d=c["bits3d"], occ_precision=c["precision"], min_w=c["min_w"],
                   min_h=c["min_h"], vox_dim=c["vox_dim"])
frs = enc.upload(frames)
enc.phase_a(frs)


def timed(*args):
    enc.stage_reset()
    enc.phase_b(frs, *args)
    ms = enc.stage_ms()
    return {k: round(ms[k], 4) for k in S18 if k in ms}


for _ in range(2):
    timed()
passes = [timed() for _ in range(6)]
total = [round(sum(p.values()), 4) for p in passes]
rgb = frs[0].get_reconstruction()[1]
out = {"lib": T.library_path(), "points": len(frames[0][0]), "recon_points": len(rgb), "passes_ms": total, "median_ms": float(np.median(total)),
       "stages_ms": {k: float(np.median([p[k] for p in passes])) for k in passes[0]}, "rgb_md5": hashlib.md5(rgb.tobytes()).hexdigest()}
if "--modes" in sys.argv:
    P = T.ColorTransferParams
    sets = {"ctc_ex": P(),
            "defaults": P(num_neighbors_fwd=1, dist_offset_fwd=0.0001, dist_offset_bwd=0.0001, skip_avg_if_identical_source_point_present_fwd=False,
                          skip_avg_if_identical_source_point_present_bwd=False),
            "fwd32": P(num_neighbors_fwd=32), "bwd4": P(num_neighbors_bwd=4),
            "col100": P(max_color_dist2_fwd=100.0, max_color_dist2_bwd=100.0), "range2": P(search_range=2)}
    out["modes_ms"] = {}
    for name, p in sets.items():
        timed(p)                                              # (warm: allocations of this shape)
        out["modes_ms"][name] = timed(p)
        if name == "ctc_ex":
            out["ctc_ex_equals_old"] = bool(np.array_equal(frs[0].get_reconstruction()[1], rgb))
print(json.dumps(out), flush=True)
enc.close()
