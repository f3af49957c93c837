"""Generate tests/golden/segmenter_params.npz from the UNMODIFIED reference (oracle/_ref): per point of tests/param_cases.py the
MD5 of the input and of the reference's patch records, depth0, depth1 and occupancy, plus the patch count.

    python tests/golden/make_segmenter_params_golden.py              # the table (needs `make -C oracle port ref`)
    python tests/golden/make_segmenter_params_golden.py --outside    # the points left out of the table: do they return?
    python tests/golden/make_segmenter_params_golden.py --outside --oracle-only   # ... and what does the oracle say of them?

Every point runs in a CHILD process under a time limit, the reference first and then the oracle: a point on which either does
not return is outside the domain (param_cases.OUTSIDE) and is reported, never written.  The fixture holds digests and small
integers only -- data produced by running the reference, no reference source text."""
import argparse
import concurrent.futures
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "mpeg-pcc-tmc2_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import oracle_binding as ob  # noqa: E402
import param_cases as pc  # noqa: E402


def child(name, engine):
    p = pc.BY_NAME.get(name) or {q["name"]: q for q in pc.OUTSIDE}[name]
    xyz, rgb = pc.cloud(p["cloud"])
    orc = ob.Oracle()
    sp = pc.oracle_params(orc, p, ob.seg_params)
    eng = ob.Reference() if engine == "reference" else orc
    seg = eng.segment(xyz, rgb, sp)
    print(json.dumps(dict(pc.result_digests(seg), stalled=seg.get("stalled", 0))))


def run(name, engine, limit):
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--point", name, "--engine", engine], timeout=limit,
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    except subprocess.TimeoutExpired:
        return None
    if r.returncode != 0:
        raise RuntimeError("%s (%s): exit %d\n%s" % (name, engine, r.returncode, r.stderr[-2000:]))
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--point")
    ap.add_argument("--engine", default="reference")
    ap.add_argument("--outside", action="store_true")
    ap.add_argument("--oracle-only", action="store_true")
    ap.add_argument("--limit", type=float, default=120.0)
    ap.add_argument("--jobs", type=int, default=8)
    a = ap.parse_args()
    if a.point:
        return child(a.point, a.engine)
    points = pc.OUTSIDE if a.outside else pc.POINTS
    with concurrent.futures.ThreadPoolExecutor(a.jobs) as ex:
        ref = [None] * len(points) if a.oracle_only else list(ex.map(lambda p: run(p["name"], "reference", a.limit), points))
        # (the oracle only where the reference returned -- except for the points known to lie outside, where the question is
        #  which of the two does not)
        orc = list(ex.map(lambda pr: run(pr[0]["name"], "oracle", a.limit) if (pr[1] is not None or a.outside) else None,
                          zip(points, ref)))
    out, bad = {"names": np.array([p["name"] for p in points])}, []
    for p, r, o in zip(points, ref, orc):
        print("%-70s reference %s  oracle %s" % (p["name"], "no return" if r is None else "%d patches" % r["patch_count"],
                                                 "no return" if o is None else ("stalled=%d" % o["stalled"] if o["stalled"] else "same" if o == r else "DIFFERS")))
        if r is None or o is None or o != r:
            bad.append(p["name"])
            continue
        out[p["name"] + "/input_md5"] = np.array(pc.input_digest(p))
        out[p["name"] + "/patch_count"] = np.int32(r["patch_count"])
        for k in ("patches", "depth0", "depth1", "occupancy"):
            out[p["name"] + "/" + k + "_md5"] = np.array(r[k])
    if a.outside:
        return
    if bad:
        sys.exit("no return within %g s, or the oracle differs (move to param_cases.OUTSIDE with the observation): %s" % (a.limit, ", ".join(bad)))
    np.savez_compressed(os.path.join(HERE, "segmenter_params.npz"), **out)
    print("%d points -> segmenter_params.npz" % len(points))


if __name__ == "__main__":
    main()
