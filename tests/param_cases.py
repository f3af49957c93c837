"""Parameter points OFF the common test conditions for the segmenter (tests/test_oracle_golden.py, tests/test_gpu_params.py,
tests/golden/make_segmenter_params_golden.py): every field of the parameter struct that the C-ABI accepts and hands to a
kernel or to the host loop, one field at a time and a dozen seeded combinations, on synthetic and degenerate clouds.

A point is (name, cloud, iterations, overrides of the CTC struct).  The fixture tests/golden/segmenter_params.npz stores, per
point, the MD5 of the input and of what the unmodified reference made of it.

Domain rule: a point is listed in POINTS only if the unmodified reference, run on the CPU in a child process under a
time limit (the generator does that), returns on it.  OUTSIDE lists what was tried and left out, with the observation; those
points are never handed to the oracle in-process nor to the GPU."""
import hashlib

import numpy as np

from tmc2_amd.synth import synth_cloud

# the CTC values of the fields below (tmc2_amd.ctc_params / oracle_binding.seg_params), for the "differs from CTC" checks
CTC = dict(surfaceThickness=4, minLevel=64, maxPatchSize=1024, enablePatchSplitting=1, quantizerSizeX=16, quantizerSizeY=16,
           minPointCountPerCC=16, maxAllowedDepth=255, geometryBitDepth2D=8, geometryBitDepth3D=11,
           maxAllowedDist2RawPointsDetection=9.0, maxAllowedDist2RawPointsSelection=1.0, lambdaRefineSegmentation=3.0,
           maxNNCountRefineSegmentation=1024, searchRadiusRefineSegmentation=192, voxelDimensionRefineSegmentation=4,
           normalOrientation=1)

# searchRadius >> log2(voxel) is the squared cell radius of the refinement's ball; the neighbourhood tile in LDS holds a ball of
# 3 936 cells: 97 (3 911 cells) is the last that fits, 98 (3 959) is refused -- with voxels of 4 that is 391 / 392
LARGEST_RADIUS_VOX4 = 391

SINGLE = [
    ("surfaceThickness", (0, 1, 8, 16)),
    ("minLevel", (1, 16, 32, 128)),
    ("maxPatchSize", (32, 64, 100)),
    ("enablePatchSplitting", (0,)),
    ("quantizer", (1, 4, 64)),                                 # both of quantizerSizeX / quantizerSizeY
    ("minPointCountPerCC", (1, 4, 64, 300)),
    ("maxAllowedDepth", (67, 96, 127)),                        # (67 = surfaceThickness + minLevel - 1: the least that is accepted)
    ("geometryBitDepth3D", (10, 12)),
    ("maxAllowedDist2RawPointsDetection", (1.0, 4.0, 9.5, 27.0)),
    ("maxAllowedDist2RawPointsSelection", (0.0, 5.0, 9.0)),
    ("lambdaRefineSegmentation", (0.0, 1.5, 10.0)),
    ("maxNNCountRefineSegmentation", (16, 64, 256)),
    ("searchRadiusRefineSegmentation", (32, 64, 96, LARGEST_RADIUS_VOX4)),
    ("voxelDimensionRefineSegmentation", (8,)),
    ("iterationCountRefineSegmentation", (0, 1)),
    ("normalOrientation", (0,)),
]
REFINE_FIELDS = ("lambdaRefineSegmentation", "maxNNCountRefineSegmentation", "searchRadiusRefineSegmentation",
                 "voxelDimensionRefineSegmentation", "iterationCountRefineSegmentation")
DEPTH_FIELDS = ("surfaceThickness", "maxAllowedDepth", "minLevel")
DEGENERATE = ("plane", "two_sheets", "lattice")
ITERATIONS = 3


def _fmt(v):
    return ("%g" % v).replace(".", "p") if isinstance(v, float) else str(v)


def _over(field, v):
    if field == "quantizer":
        return dict(quantizerSizeX=v, quantizerSizeY=v)
    return {field: v}


def _build():
    pts = []

    def add(name, cloud, over, iters=ITERATIONS):
        over = dict(over)
        iters = over.pop("iterationCountRefineSegmentation", iters)
        pts.append(dict(name="%s-%s" % (name, cloud), cloud=cloud, iterations=int(iters), overrides=over))

    for cloud in ("tiny", "small", "medium") + DEGENERATE + ("slope",):   # the CTC point itself: what the others are compared with
        add("ctc", cloud, {})
    for field, values in SINGLE:
        for v in values:
            for cloud in ("tiny", "small"):
                add("%s=%s" % (field, _fmt(v)), cloud, _over(field, v))
            if field in DEPTH_FIELDS:
                for cloud in DEGENERATE + (("slope",) if field == "maxAllowedDepth" else ()):
                    add("%s=%s" % (field, _fmt(v)), cloud, _over(field, v))
    # the depth range of 10-bit geometry video
    for v in (63, 31):                                         # (below surfaceThickness + minLevel - 1: see OUTSIDE)
        add("maxAllowedDepth=%d" % v, "tiny", dict(maxAllowedDepth=v))
    for cloud in ("tiny", "small") + DEGENERATE + ("slope",):
        add("maxAllowedDepth=1023,geometryBitDepth2D=10", cloud, dict(maxAllowedDepth=1023, geometryBitDepth2D=10))
    # surfaceThickness inside the depth filter ("surfaceThickness + d > d1 + maxAllowedDepth"): at the CTC's maxAllowedDepth no
    # pixel of these clouds comes near the limit, so the term shows only next to a small maxAllowedDepth
    for st, mad in ((0, 67), (8, 71), (16, 96), (16, 127), (1, 96)):
        for cloud in ("tiny", "small") + DEGENERATE:
            add("surfaceThickness=%d,maxAllowedDepth=%d" % (st, mad), cloud, dict(surfaceThickness=st, maxAllowedDepth=mad))
    # splitting off while maxPatchSize is small: the size must then be ignored (on these clouds, all narrower than the CTC's
    # 1 024, enablePatchSplitting = 0 alone changes nothing)
    for cloud, size in (("tiny", 32), ("small", 32), ("small", 64), ("medium", 64)):
        add("enablePatchSplitting=0,maxPatchSize=%d" % size, cloud, dict(enablePatchSplitting=0, maxPatchSize=size))
    # the two quantizers apart (a pair that is swapped shows)
    for cloud in ("tiny", "small"):
        add("quantizerSizeX=4,quantizerSizeY=64", cloud, dict(quantizerSizeX=4, quantizerSizeY=64))
        add("quantizerSizeX=64,quantizerSizeY=1", cloud, dict(quantizerSizeX=64, quantizerSizeY=1))
    # a handful at 209 142 points
    for over in (dict(surfaceThickness=1), dict(maxPatchSize=64), dict(maxPatchSize=100), dict(enablePatchSplitting=0), dict(minLevel=16), dict(minPointCountPerCC=1),
                 dict(maxNNCountRefineSegmentation=64), dict(searchRadiusRefineSegmentation=96, lambdaRefineSegmentation=1.5)):
        add(",".join("%s=%s" % (k, _fmt(v)) for k, v in over.items()), "medium", over)
    # seeded combinations: several fields at once from the sets above (minLevel and surfaceThickness drawn so that
    # surfaceThickness + minLevel - 1 <= maxAllowedDepth, the accepted range)
    for seed in range(13):
        rng = np.random.default_rng(4100 + seed)
        fields = [f for f, _ in SINGLE if f != "maxAllowedDepth"]
        over = {}
        for i in rng.choice(len(fields), int(rng.integers(3, 7)), replace=False):
            f = fields[int(i)]
            vals = dict(SINGLE)[f]
            v = vals[int(rng.integers(0, len(vals)))]
            if f == "quantizer":
                over["quantizerSizeX"] = v
                over["quantizerSizeY"] = (1, 4, 64)[int(rng.integers(0, 3))]
            else:
                over[f] = v
        if rng.random() < 0.5:
            st, lv = over.get("surfaceThickness", 4), over.get("minLevel", 64)
            ok = [d for d in (67, 96, 127, 1023) if st + lv - 1 <= d]
            over["maxAllowedDepth"] = ok[int(rng.integers(0, len(ok)))]
            if over["maxAllowedDepth"] == 1023:
                over["geometryBitDepth2D"] = 10
        add("combined%02d" % seed, ("tiny", "small")[seed % 2], over)
    return pts


# Tried and left out of the table: the unmodified reference does not return (each point in a child process with a time limit
# of 120 s; the oracle of before this table, given the same limit, did not return either).  Two mechanisms, both in the loop
# "while there are raw points" of the patch segmentation, both a round that changes nothing and is therefore repeated for ever:
#   depth filter   -- with surfaceThickness + minLevel - 1 > maxAllowedDepth a component can hold a point whose depth, counted
#                     from the patch's quantised depth origin, fails "surfaceThickness + d > d1 + maxAllowedDepth" even in a
#                     patch of its own.  tmc2_segmenter_params_check refuses that range; inside it every component's extreme
#                     point passes, so every round takes a point off the list.
#   patch splitting -- a component keeps the points within maxPatchSize of its (min u, min v) corner; a component with no point
#                     in that corner box (an L or a diagonal band) keeps none.  This depends on the cloud, not on the
#                     parameters alone: the library ends the call with TMC2_E_UNSUPPORTED when it meets such a component.
# The oracle now leaves its loop in both cases and says so (result["stalled"]); tests hand these points to it in a child process
# under a time limit only, and nothing hands them to the GPU.
OUTSIDE_OBSERVED = {
    "maxAllowedDepth=63-tiny": "depth filter: reference no return within 100 s (none within 25 minutes in an earlier trial), oracle the same",
    "maxAllowedDepth=31-tiny": "depth filter: reference no return within 100 s, oracle the same",
    "maxPatchSize=32-small": "patch splitting: reference no return within 120 s, oracle the same",
    "maxPatchSize=64-medium": "patch splitting: reference no return within 120 s, oracle the same",
    "maxPatchSize=100-medium": "patch splitting: reference no return within 120 s",
    "combined05-small": "patch splitting (maxPatchSize=32 on small): reference no return within 120 s, oracle the same",
}
OUTSIDE_STALL = {"maxAllowedDepth=63-tiny": 2, "maxAllowedDepth=31-tiny": 2, "maxPatchSize=32-small": 1, "maxPatchSize=64-medium": 1,
                 "maxPatchSize=100-medium": 1,                  "combined05-small": 1}      # what the oracle's "stalled" says there

_all = _build()
POINTS = [p for p in _all if p["name"] not in OUTSIDE_OBSERVED]
OUTSIDE = [dict(p, observed=OUTSIDE_OBSERVED[p["name"]]) for p in _all if p["name"] in OUTSIDE_OBSERVED]
BY_NAME = {p["name"]: p for p in POINTS}
assert len(BY_NAME) == len(POINTS) and len(OUTSIDE) == len(OUTSIDE_OBSERVED)


def point_id(p):
    return p["name"]


def is_refine_point(p):
    return any(f in p["overrides"] for f in REFINE_FIELDS) or p["iterations"] != ITERATIONS


def digest(a):
    return hashlib.md5(np.ascontiguousarray(a).tobytes()).hexdigest()


def degenerate(kind):
    """plane (rank-deficient covariance everywhere), two sheets two voxels apart, lattice (exact distance ties everywhere), in
    the style of test_oracle_golden.degenerate_cloud but by name: unique positions in random order, random colours.  slope: one
    sheet that climbs 300 in depth over 400 across -- a single component far deeper than any maxAllowedDepth of the table but
    1 023 (the shells of synth_cloud never come near the CTC's 255, nor near 96)."""
    rng = np.random.default_rng({"plane": 31, "two_sheets": 32, "lattice": 33, "slope": 34}[kind])
    if kind == "slope":
        x, y = np.meshgrid(np.arange(100, 500), np.arange(100, 140))
        base = np.stack([x.ravel(), y.ravel(), 50 + 3 * (x.ravel() - 100) // 4], 1)
    elif kind == "plane":
        base = rng.integers(100, 400, (2500, 3))
        base[:, 2] = 7
    elif kind == "two_sheets":
        base = rng.integers(200, 320, (2500, 3))
        base[:, 1] = np.where(rng.random(2500) < 0.5, 210, 212)
    else:
        base = 130 + 3 * np.stack(np.meshgrid(np.arange(12), np.arange(12), np.arange(14)), -1).reshape(-1, 3)
    xyz = np.unique(np.clip(base, 0, 1023).astype(np.int16), axis=0)
    xyz = np.ascontiguousarray(xyz[rng.permutation(len(xyz))])
    return xyz, rng.integers(0, 256, (len(xyz), 3), dtype=np.uint8)


_clouds = {}


def cloud(name):
    if name not in _clouds:
        _clouds[name] = degenerate(name) if name in DEGENERATE + ("slope",) else synth_cloud(name)
    return _clouds[name]


def input_digest(p):
    xyz, rgb = cloud(p["cloud"])
    return digest(xyz) + digest(rgb)


_ALIAS = {"minPointCountPerCC": ("minPointCountPerCC", "minPointCountPerCCPatchSegmentation")}


def apply(params, p):
    """the point's overrides on a parameter struct of either binding (oracle_binding.SegParams, tmc2_amd.SegmenterParams)"""
    params.iterationCountRefineSegmentation = p["iterations"]
    for k, v in p["overrides"].items():
        names = [n for n in _ALIAS.get(k, (k,)) if hasattr(params, n)]
        assert len(names) == 1, k
        setattr(params, names[0], v)
    return params


def oracle_params(oracle, p, make):
    """make = oracle_binding.seg_params or tmc2_amd.ctc_params: CTC, the cloud's projection weights, then the overrides"""
    xyz, _ = cloud(p["cloud"])
    bits3d = p["overrides"].get("geometryBitDepth3D", CTC["geometryBitDepth3D"])
    return apply(make(p["iterations"], bits3d, oracle.weight_normal(xyz, bits3d, 0.6)), p)


PATCH_FIELDS = ("index", "viewId", "normalAxis", "tangentAxis", "bitangentAxis", "projectionMode", "u1", "v1", "d1", "sizeU",
                "sizeV", "sizeD", "sizeDPixel", "sizeU0", "sizeV0", "size2DXInPixel", "size2DYInPixel", "d0Count",
                "eomAndD1Count", "u0", "v0", "patchOrientation")


def patch_matrix(patches):
    """every patch field except the two pool offsets, [patch][field] int32"""
    return np.ascontiguousarray(np.stack([patches[n] for n in PATCH_FIELDS], 1).astype(np.int32)).reshape(len(patches), len(PATCH_FIELDS))


def result_digests(seg):
    """what the fixture keeps of a segmentation (dict with patches, depth0, depth1, occupancy)"""
    return dict(patches=digest(patch_matrix(seg["patches"])), depth0=digest(seg["depth0"].astype(np.int16)),
                depth1=digest(seg["depth1"].astype(np.int16)), occupancy=digest(seg["occupancy"].astype(np.uint8)),
                patch_count=len(seg["patches"]))
