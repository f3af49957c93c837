"""Generate tests/golden/color_transfer_options.npz from the UNMODIFIED reference's PCCPointSet3::transferColors.

Run where the reference is (needs oracle/_ref/libtmc2ref.so: `make -C oracle ref`):
    python tests/golden/make_color_transfer_options_golden.py
The oracle's harness runs the transfer at the CTC point only, so a shim of our own (color_transfer_options_shim.cpp, next to this
file) is compiled into a TEMPORARY directory against the reference's headers and oracle/_ref/libtmc2ref.so with the include paths and
flags of oracle/Makefile.  Everything stored is DATA the reference produced (per case and parameter set the target colours, per case
its own seconds, the reconstruction of the `pipeline` case) -- no reference text.  The inputs are rebuilt by the tests from
tests/color_transfer_cases.py; their digests are stored.

What is asserted here, on the reference's results alone, before anything is written -- the (case, set) pairs that tell the readings of
color_transfer_rules.h from the ones the text suggests:
  1. a threshold of 512 is none, 511 is one:      contrast/col512 == contrast/ctc,  contrast/col511 != contrast/ctc
  2. the pairwise maximum starts at DBL_MIN:      contrast/col0_range1 != contrast/coleps_range1 (a threshold of 1e-300 lies between
     DBL_MIN and every non-zero distance: it is what a threshold of 0 would be if the maximum started at 0)
  3. the geometry threshold keeps the first forward result and may empty a backward list:  far/geo2 gives each far target the colour
     of its single nearest source point, more than 2 away
  4. without the skip flag an identical point is averaged:   identical/noskip != identical/ctc
  5. the outlier pass compares with the shrunk length:  contrast/col100_outlier1 holds no colour with a channel below 20 (a list all
     of whose kept entries are outliers keeps its mean; compared with the longer unshrunk length the reference would divide 0 by 0)
     -- and the inputs hold at least one list that is shrunk and whose kept entries are all outliers (all_kept_outliers)
  6, 7. duplicate candidates of the clipped cube are the same colour, and the weighted mean of one colour is that colour: neither
     reading changes a result; clip/range1, clip/range2 and tiny/* hold the paths.
Beside the grid, cc.BOUNDARY: neighbour counts at and just below the size of clouds of fewer than 32 points, in both directions.
At least ten of the non-ctc sets differ from ctc on some case; the host form of the library (tmc2_host_transfer_colors) accepts every
(case, set) pair (a refusal here is a failure of the inputs)."""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "mpeg-pcc-tmc2_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import color_transfer_cases as cc  # noqa: E402

REF = os.environ.get("REF", "/root/reference")
LIBDIRS = ("PccLibCommon", "PccLibBitstreamCommon")


def build_shim(tmp):
    ref_dir = os.path.join(ROOT, "oracle", "_ref")
    out = os.path.join(tmp, "libcolortransferoptionsshim.so")
    inc = ["-I" + os.path.join(ref_dir, "gen")] + ["-I%s/source/lib/%s/include" % (REF, d) for d in LIBDIRS] + \
          ["-I%s/dependencies/nanoflann" % REF, "-I%s/dependencies/libmd5" % REF]
    subprocess.check_call(["g++", "-O3", "-DNDEBUG", "-std=c++14", "-fPIC", "-w", "-shared"] + inc +
                          [os.path.join(HERE, "color_transfer_options_shim.cpp"), "-o", out, "-L" + ref_dir, "-ltmc2ref", "-Wl,-rpath," + ref_dir])
    return C.CDLL(out)


def reference_transfer(shim, src, col, tgt, params):
    """-> (target colours uint8 [m][3], seconds inside transferColors)"""
    a, b, c = np.ascontiguousarray(src, np.int16), np.ascontiguousarray(col, np.uint8), np.ascontiguousarray(tgt, np.int16)
    st = params.struct()
    flags = (C.c_int * 9)(st.searchRange, st.losslessAttribute, st.numNeighborsColorTransferFwd, st.numNeighborsColorTransferBwd,
                          st.useDistWeightedAverageFwd, st.useDistWeightedAverageBwd, st.skipAvgIfIdenticalSourcePointPresentFwd,
                          st.skipAvgIfIdenticalSourcePointPresentBwd, st.excludeColorOutlier)
    reals = (C.c_double * 7)(st.distOffsetFwd, st.distOffsetBwd, st.maxGeometryDist2Fwd, st.maxGeometryDist2Bwd, st.maxColorDist2Fwd,
                             st.maxColorDist2Bwd, st.thresholdColorOutlierDist)
    out, sec = np.zeros((len(c), 3), np.uint8), C.c_double()
    p = lambda x: x.ctypes.data_as(C.c_void_p)  # noqa: E731
    assert shim.cto_transfer(p(a), p(b), C.c_size_t(len(a)), p(c), C.c_size_t(len(c)), flags, reals, p(out), C.byref(sec)) == 0
    return out, sec.value


def pipeline_target():
    """the reconstruction of frame 0 of the tiny GOF, through the reference's own members (as tests/golden/make_golden.py, gof)"""
    import oracle_binding as ob
    from tmc2_amd.synth import synth_cloud
    ref = ob.Reference()
    frames = [synth_cloud("tiny", f) for f in range(2)]
    b = ref.phase_b(frames, ref.phase_a(frames, 10, 11, 4), 4)
    xyz = np.ascontiguousarray(b[0]["recon_xyz"], np.int16)
    g = np.load(os.path.join(HERE, "gof_tiny2.npz"))
    import hashlib
    assert hashlib.md5(np.ascontiguousarray(b[0]["recon_xyz"]).tobytes()).hexdigest() == str(g["f0_recon_xyz_md5"])
    return xyz, np.ascontiguousarray(b[0]["recon_rgb"], np.uint8)


def sq_dists(a, b):
    d = a.astype(np.int64)[:, None, :] - b.astype(np.int64)[None, :, :]
    return (d * d).sum(2)


def check_inputs():
    src, col, tgt = cc.case("far")
    d = sq_dists(tgt[-6:], src)
    assert ((d.min(1) >= 144) & (d.min(1) <= 900 * 3)).all() and ((np.sort(d, 1)[:, 1] > d.min(1))).all(), "far: the far targets"
    assert (sq_dists(src[-6:], tgt).min(1) >= 144).all(), "far: the far sources"
    src, col, tgt = cc.case("crowded")
    assert (sq_dists(src, tgt).argmin(1) == 0).sum() >= 64
    src, col, tgt = cc.case("tiny")
    assert len(src) == 32 and len(tgt) == 5


def all_kept_outliers(name, params):
    """Targets whose backward list is SHRUNK by the colour threshold and whose kept entries ALL lie further than the outlier threshold
    from their weighted mean: the only lists on which comparing the dropped count with the shrunk or with the unshrunk length differs
    (with the unshrunk length the reference would divide 0 by 0).  Brute force from the inputs; candidates of equal distance in index
    order, and only lists whose cut does not fall between equal distances are counted."""
    src, col, tgt = cc.case(name)
    st = params.struct()
    kb, thr, out2 = st.numNeighborsColorTransferBwd, st.maxColorDist2Bwd, st.thresholdColorOutlierDist ** 2
    assert st.skipAvgIfIdenticalSourcePointPresentBwd == 0 and st.useDistWeightedAverageBwd and st.excludeColorOutlier and thr < 512
    d = sq_dists(src, tgt)
    lists = [[] for _ in tgt]
    for s in range(len(src)):
        order = np.argsort(d[s], kind="stable")
        if d[s][order[kb - 1]] == d[s][order[kb]]:
            continue                                   # (which of the equidistant targets the search returns is the tree's business)
        for t in order[:kb]:
            lists[t].append((int(d[s][t]), s))
    found = 0
    for cand in lists:
        cand.sort()
        c = col[[s for _, s in cand]].astype(np.float64)
        kept = len(cand)
        while kept > 1 and max(((c[i] - c[j]) ** 2).sum() for i in range(kept) for j in range(i + 1, kept)) > thr:
            kept -= 1
        if kept < 2 or kept == len(cand) or cand[kept - 1][0] == cand[kept][0]:
            continue
        w = 1.0 / (np.sqrt([float(x) for x, _ in cand[:kept]]) + st.distOffsetBwd)
        mean = (c[:kept] * w[:, None]).sum(0) / w.sum()
        found += bool((((c[:kept] - mean) ** 2).sum(1) > out2).all())
    return found


def check_readings(res):
    same = lambda a, b: np.array_equal(res[a], res[b])  # noqa: E731
    assert same("contrast__col512", "contrast__ctc") and not same("contrast__col511", "contrast__ctc"), "reading 1"
    assert not same("contrast__col0_range1", "contrast__coleps_range1"), "reading 2"
    src, col, tgt = cc.case("far")
    d = sq_dists(tgt[-6:], src)
    assert (d.min(1) > 2).all() and (sq_dists(src, tgt[-6:]).min(0) > 2).all()      # (no source point may vote for them: their lists are empty)
    assert np.array_equal(res["far__geo2"][-6:], col[d.argmin(1)]) and not np.array_equal(res["far__ctc"][-6:], col[d.argmin(1)]), "reading 3"
    assert not same("identical__noskip", "identical__ctc"), "reading 4"
    assert all_kept_outliers("contrast", cc.PARAM_SETS["col100_outlier1"]) >= 1, "reading 5: no list tells the two lengths apart"
    assert cc.case("contrast")[1].min() >= 20 and res["contrast__col100_outlier1"].min() >= 20, "reading 5"
    assert not same("contrast__col100_outlier1", "contrast__ctc")
    differing = [s for s in cc.PARAM_SETS if s != "ctc" and any(not same(cc.key(c, s), cc.key(c, "ctc")) for c in cc.CASES)]
    print("sets that differ from ctc on some case (%d): %s" % (len(differing), " ".join(differing)))
    assert len(differing) >= 10


def check_library(res):
    """every (case, set) pair stays inside the library's refusals (CPU: the host form); report where it disagrees"""
    import tmc2_amd as T
    wrong = []
    for name, set_name in cc.runs():
        src, col, tgt = cc.case(name)
        got = T.host_transfer_colors(src, col, tgt, cc.PARAM_SETS[set_name])       # raises on a refusal
        assert np.array_equal(cc.expected(name, set_name), res[cc.key(name, set_name)])
        if not np.array_equal(got, res[cc.key(name, set_name)]):
            wrong.append("%s (%d)" % (cc.key(name, set_name), int((got != res[cc.key(name, set_name)]).any(1).sum())))
    for name, (_, params) in cc.BOUNDARY.items():
        if not np.array_equal(T.host_transfer_colors(*cc.boundary_case(name), params), res["boundary__" + name]):
            wrong.append("boundary " + name)
    print("host form differs on: %s" % (", ".join(wrong) or "nothing"))


def generate(shim, out):
    res = {}
    for name in cc.CASES:
        src, col, tgt = cc.case(name)
        out[name + "__input_md5"] = np.array(cc.digest(src, col, tgt))
        seconds = []
        for set_name, params in cc.PARAM_SETS.items():
            rgb, sec = reference_transfer(shim, src, col, tgt, params)
            res[cc.key(name, set_name)] = rgb
            # (most targets keep the ctc set's colour under most sets: stored as the byte-wise difference to it, which packs well)
            if set_name == "ctc":
                out[cc.key(name, set_name) + "__rgb"] = rgb
            else:
                out[cc.key(name, set_name) + "__delta"] = rgb - res[cc.key(name, "ctc")]
            seconds.append(sec)
        out[name + "__reference_seconds"] = np.array(seconds)
        print("%-10s %5d -> %5d points, reference per set: %s s" % (name, len(src), len(tgt), " ".join("%.3f" % s for s in seconds)), flush=True)
    out["cases"], out["sets"] = np.array(list(cc.CASES)), np.array(list(cc.PARAM_SETS))
    for name, (_, params) in cc.BOUNDARY.items():      # neighbour counts at and just below the size of a cloud of fewer than 32 points
        src, col, tgt = cc.boundary_case(name)
        out["boundary__" + name + "__input_md5"] = np.array(cc.digest(src, col, tgt))
        res["boundary__" + name], _ = reference_transfer(shim, src, col, tgt, params)
        out["boundary__" + name + "__rgb"] = res["boundary__" + name]
    return res


def main():
    out = {}
    xyz, rgb = pipeline_target()
    out["pipeline__target_xyz"] = xyz
    np.savez_compressed(cc.FIXTURE, **out)             # (tests/color_transfer_cases.py reads the pipeline target from the fixture)
    cc.case.cache_clear()
    check_inputs()
    with tempfile.TemporaryDirectory() as tmp:
        res = generate(build_shim(tmp), out)
    assert np.array_equal(res["pipeline__ctc"], rgb), "the pipeline's own transfer"
    check_readings(res)
    np.savez_compressed(cc.FIXTURE, **out)
    cc.fixture.cache_clear()
    check_library(res)
    print(cc.FIXTURE, os.path.getsize(cc.FIXTURE), "bytes")


if __name__ == "__main__":
    main()
