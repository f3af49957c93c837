"""GPU tier (-m gpu) of the k-NN refinement of the segmentation (the reference's non-grid mode): the wave-per-query search
(csrc/knn_wide.hip), the voting rounds (csrc/refine_knn.hip) and Frame.segmenter_compute( knn_refine_params[, grid_based] ).

The reference is not where these tests run and the oracle's search ends at k = 64, so the yardsticks are: the oracle for K <= 64,
the host restatement (tmc2_host_refine_segmentation; the CPU tier holds it against the reference), the fixture
tests/golden/knn_refine_segmentation.npz (rows as CRC32 of the sorted row, partitions as bytes, chain digests of the UNMODIFIED
reference) and the brute-force bound.  Rows are compared as sets; everything is exact equality."""
import ctypes

import numpy as np
import pytest

import knn_refine_cases as kc
import param_cases as pc
import tmc2_amd as T

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def golden():
    return np.load(kc.FIXTURE)


_frames = {}


def frame_of(gpu_ctx, name):
    """one frame per cloud for the searches (the tree is built once)"""
    if name not in _frames:
        _frames[name] = gpu_ctx.frame(*kc.cloud(name))
    return _frames[name]


def state(fr):
    patches, d0, d1, occ = fr.get_patches()
    return dict(normals=fr.get_normals(), partition=fr.get_partition(), knn=fr.get_adjacency(16), patches=patches, depth0=d0, depth1=d1, occupancy=occ)


def assert_same_state(a, b):
    assert np.array_equal(bits(a["normals"]), bits(b["normals"])) and np.array_equal(a["partition"], b["partition"])
    assert np.array_equal(a["knn"], b["knn"]) and len(a["patches"]) == len(b["patches"])
    for n in pc.PATCH_FIELDS:
        assert np.array_equal(a["patches"][n], b["patches"][n]), n
    for k in ("depth0", "depth1", "occupancy"):
        assert np.array_equal(a[k], b[k]), k


def assert_is_chain(got, y):
    assert np.array_equal(bits(got["normals"]), bits(y["normals"])), "normals of the points"
    assert np.array_equal(got["partition"], y["partition"]), "partition: %d points differ" % (got["partition"] != y["partition"]).sum()
    assert np.array_equal(got["knn"], y["knn"]), "adjacency (the full cloud's k = 16)"
    seg = y["seg"]
    assert len(got["patches"]) == len(seg["patches"])
    for n in pc.PATCH_FIELDS:
        assert np.array_equal(got["patches"][n], seg["patches"][n]), n
    assert np.array_equal(got["depth0"], seg["depth0"]) and np.array_equal(got["depth1"], seg["depth1"]), "depth pools"
    assert np.array_equal(got["occupancy"], seg["occupancy"]), "occupancy"


def knn_params(fr, oracle, xyz, orientation=1):
    w = fr.weight_normal(kc.BITS3D, 0.6)
    assert np.array_equal(bits(w), bits(oracle.weight_normal(xyz, kc.BITS3D, 0.6)))
    return kc.overrides(T.knn_refine_params(kc.ITERATIONS, kc.BITS3D, w), orientation)


# ---- the wide search
@pytest.mark.parametrize("case", kc.ADJACENCY, ids=kc.adjacency_id)
def test_gpu_wide_search_matches_reference_rows(gpu_ctx, golden, case):
    name = "adjacency/" + kc.adjacency_id(case)
    q = kc.queries_of(case)
    rows = frame_of(gpu_ctx, case[0]).kdtree_search_wide(case[1], q)
    assert rows.shape == (len(kc.cloud(case[0])[0]) if q is None else len(q), case[1])
    assert rows.max() < len(kc.cloud(case[0])[0])
    assert kc.first_bad_row(rows, golden[name + "/row_crc"]) == -1, "first row whose set differs from the reference's"
    assert pc.digest(kc.sorted_rows(rows)) == str(golden[name + "/rows_md5"])


@pytest.mark.parametrize("k", [1, 16, 64])
@pytest.mark.parametrize("foreign", [False, True], ids=["self", "foreign"])
def test_gpu_wide_search_matches_oracle(gpu_ctx, oracle, k, foreign):
    xyz = kc.cloud("tiny")[0]
    q = kc.queries_of(("tiny", k, True)) if foreign else None
    rows = frame_of(gpu_ctx, "tiny").kdtree_search_wide(k, q)
    assert np.array_equal(kc.sorted_rows(rows), kc.sorted_rows(oracle.knn(xyz, xyz if q is None else q, k)))


@pytest.mark.parametrize("case", [c for c in kc.ADJACENCY if not c[2] and c[1] > 64], ids=kc.adjacency_id)
def test_gpu_wide_search_matches_host_entry(gpu_ctx, case):
    xyz = kc.cloud(case[0])[0]
    host = T.host_refine_segmentation(xyz, np.zeros((len(xyz), 3)), np.zeros(len(xyz), np.uint32), case[1], 0.0, 0, with_adjacency=True)[1]
    rows = frame_of(gpu_ctx, case[0]).kdtree_search_wide(case[1])
    a, b = kc.sorted_rows(rows), kc.sorted_rows(host)
    bad = np.nonzero((a != b).any(1))[0]
    assert len(bad) == 0, "%d rows differ from the host entry's, first %d" % (len(bad), bad[0])


def test_gpu_wide_search_keeps_the_brute_force_bound(gpu_ctx):
    xyz = kc.cloud("lattice")[0]
    kc.brute_force_bound(xyz, None, frame_of(gpu_ctx, "lattice").kdtree_search_wide(256))
    q = kc.queries_of(("lattice", 100, True))
    kc.brute_force_bound(xyz, q, frame_of(gpu_ctx, "lattice").kdtree_search_wide(100, q))


def test_gpu_wide_search_refusals(gpu_ctx):
    fr = frame_of(gpu_ctx, "tiny[:257]")
    for k in (0, -1, 258):
        with pytest.raises(T.Tmc2Error, match="error -3: kdtree_search_wide: k=%d larger than the cloud \\(257 points\\), or below 1" % k):
            fr.kdtree_search_wide(k)
    with pytest.raises(T.Tmc2Error, match="error -4: kdtree_search_wide: k=1025 above 1024"):
        frame_of(gpu_ctx, "tiny").kdtree_search_wide(1025)
    with pytest.raises(T.Tmc2Error, match="error -4: kdtree_search_wide: coordinate -5000 below -4096"):
        fr.kdtree_search_wide(4, np.array([[1, 2, 3], [0, -5000, 0]], np.int16))
    assert fr.kdtree_search_wide(257).shape == (257, 257)


# ---- the rounds
@pytest.mark.parametrize("case", kc.ROUNDS, ids=kc.rounds_id)
def test_gpu_segmenter_refine_matches_reference(gpu_ctx, oracle, golden, case):
    cloud, k, lam, counts = case
    name = "rounds/" + kc.rounds_id(case)
    xyz, nrm, part, _ = kc.start(oracle, cloud)
    assert np.array_equal(part, golden[name + "/initial"])
    fr = gpu_ctx.frame(*kc.cloud(cloud))
    fr.set_normals(nrm)
    for c in counts:
        fr.set_partition(part)
        fr.segmenter_refine(k, lam, c)
        got, want = fr.get_partition(), golden[name + "/after_%d" % c]
        assert np.array_equal(got, want), "after %d rounds: %d points differ, first %d" % (c, (got != want).sum(), int(np.argmax(got != want)))
    assert np.array_equal(bits(fr.get_normals()), bits(nrm))


def test_gpu_segmenter_refine_leaves_what_it_must(gpu_ctx, oracle):
    """0 rounds and (all-zero normals, lambda 0) return the partition as it was; the k = 16 adjacency of the frame is not touched"""
    xyz, nrm, part, _ = kc.start(oracle, "tiny")
    fr = gpu_ctx.frame(*kc.cloud("tiny"))
    fr.normals_compute(16, 1)
    knn = fr.get_adjacency(16)
    assert np.array_equal(knn, oracle.knn_self(xyz, 16))
    fr.set_partition(part)
    fr.segmenter_refine(256, 3.0, 0)
    assert np.array_equal(fr.get_partition(), part)
    fr.set_normals(np.zeros_like(nrm))
    fr.segmenter_refine(256, 0.0, 7)
    assert np.array_equal(fr.get_partition(), part)
    fr.set_normals(nrm)
    fr.segmenter_refine(256, 3.0, 3)
    assert np.array_equal(fr.get_partition(), T.host_refine_segmentation(xyz, nrm, part, 256, 3.0, 3))
    assert np.array_equal(fr.get_adjacency(16), knn)


def test_gpu_segmenter_refine_refusals_leave_the_frame_unchanged(gpu_ctx, oracle):
    xyz, nrm, part, _ = kc.start(oracle, "lattice")
    fr = gpu_ctx.frame(*kc.cloud("lattice"))
    with pytest.raises(T.Tmc2Error, match="error -5: segmenter_refine: the frame has no normals / partition"):
        fr.segmenter_refine(16, 3.0, 1)
    fr.set_normals(nrm), fr.set_partition(part)
    n = len(xyz)
    for args, message in (((n + 1 if n < 1024 else 1025, 3.0, 1), "maxNNCountRefineSegmentation %d" % (n + 1 if n < 1024 else 1025)),
                          ((0, 3.0, 1), "maxNNCountRefineSegmentation 0 outside 1..1024"), ((1025, 3.0, 1), "maxNNCountRefineSegmentation 1025 outside 1..1024"),
                          ((16, 3.0, -1), "iterationCountRefineSegmentation -1 is negative"), ((16, -0.5, 1), "lambdaRefineSegmentation is negative")):
        with pytest.raises(T.Tmc2Error, match="error -4: segmenter_refine: .*" + message):
            fr.segmenter_refine(*args)
        assert np.array_equal(fr.get_partition(), part) and np.array_equal(bits(fr.get_normals()), bits(nrm))
    small = gpu_ctx.frame(*kc.cloud("tiny[:256]"))
    small.set_normals(np.zeros((256, 3))), small.set_partition(np.zeros(256, np.uint32))
    with pytest.raises(T.Tmc2Error, match="error -4: segmenter_refine: maxNNCountRefineSegmentation 257 larger than the cloud \\(256 points\\)"):
        small.segmenter_refine(257, 3.0, 1)


# ---- the chain
@pytest.mark.parametrize("case", kc.CHAIN, ids=kc.chain_id)
def test_gpu_knn_refine_chain_matches_reference_and_host(gpu_ctx, oracle, golden, case):
    cloud, vox_dim, orientation = case
    name = "chain/" + kc.chain_id(case)
    xyz, rgb = kc.cloud(cloud)
    assert kc.input_digest(cloud) == str(golden[name + "/input_md5"])
    fr = gpu_ctx.frame(xyz, rgb)
    p = knn_params(fr, oracle, xyz, orientation)
    gpu_ctx.stage_reset()
    fr.segmenter_compute(p, grid_based=vox_dim or None)
    calls = gpu_ctx.stage_calls()
    got = state(fr)
    d = kc.digests(got["partition"], dict(patches=got["patches"], depth0=got["depth0"], depth1=got["depth1"], occupancy=got["occupancy"]))
    for k in ("partition", "patches", "depth0", "depth1", "occupancy"):
        assert d[k] == str(golden[name + "/" + k + "_md5"]), "reference: " + k
    assert d["patch_count"] == int(golden[name + "/patch_count"])
    assert calls.get("knn_wide", 0) == 1 and calls.get("refine_knn", 0) == 1 and calls.get("knn_self", 0) == (2 if vox_dim else 1)
    assert calls.get("voxelize", 0) == (1 if vox_dim else 0)
    assert_is_chain(got, kc.host_chain(oracle, case))
    assert np.array_equal(got["knn"], oracle.knn_self(xyz, 16)), "get_adjacency( 16 ) is still the full cloud's"


def test_gpu_plain_compute_after_reset_gives_the_plain_result(gpu_ctx, oracle):
    import oracle_binding as ob
    xyz, rgb = kc.cloud("tiny")
    w = oracle.weight_normal(xyz, kc.BITS3D, 0.6)
    plain = oracle.segment(xyz, rgb, ob.seg_params(3, kc.BITS3D, w))
    fr = gpu_ctx.frame(xyz, rgb)
    fr.segmenter_compute(knn_params(fr, oracle, xyz))
    assert_is_chain(state(fr), kc.host_chain(oracle, ("tiny", 0, 1)))
    fr.reset()
    fr.segmenter_compute(T.ctc_params(3, kc.BITS3D, w))
    got = state(fr)
    assert len(got["patches"]) == len(plain["patches"])
    for n in pc.PATCH_FIELDS:
        assert np.array_equal(got["patches"][n], plain["patches"][n]), n
    assert np.array_equal(got["depth0"], plain["depth0"]) and np.array_equal(got["depth1"], plain["depth1"]) and np.array_equal(got["occupancy"], plain["occupancy"])
    fr.segmenter_compute(knn_params(fr, oracle, xyz), grid_based=2)            # and back, without a reset
    assert_is_chain(state(fr), kc.host_chain(oracle, ("tiny", 2, 1)))


def test_gpu_two_frames_of_different_size_on_one_context(oracle):
    """the context's scratch grows, then serves a smaller frame, then the larger one again"""
    ctx = T.Context(0)
    for cloud in ("lattice", "tiny", "lattice", "tiny"):
        xyz, rgb = kc.cloud(cloud)
        fr = ctx.frame(xyz, rgb)
        fr.segmenter_compute(knn_params(fr, oracle, xyz))
        assert_is_chain(state(fr), kc.host_chain(oracle, (cloud, 0, 1)))
    held = ctx.pool_stats()["bytes_held"]
    fr.segmenter_compute(knn_params(fr, oracle, xyz))
    assert ctx.pool_stats()["bytes_held"] == held


def test_gpu_chain_refusals_leave_the_frame_unchanged(gpu_ctx, oracle):
    xyz, rgb = kc.cloud("tiny")
    fr = gpu_ctx.frame(xyz, rgb)
    w = fr.weight_normal(kc.BITS3D, 0.6)
    fr.segmenter_compute(T.ctc_params(3, kc.BITS3D, w))
    before = state(fr)

    def refused(message, grid_based=None, **over):
        p = knn_params(fr, oracle, xyz)
        for k, v in over.items():
            setattr(p, k, v)
        with pytest.raises(T.Tmc2Error, match="error -4: .*" + message):
            if over.get("gridBasedRefineSegmentation"):
                # (the Python method would go to the plain entry)
                T.lib._check(fr.L.tmc2_segmenter_compute_knn_refine(fr.h, ctypes.byref(p), 0))
            else:
                fr.segmenter_compute(p, grid_based=grid_based)
        assert_same_state(state(fr), before)

    refused("params: gridBasedRefineSegmentation must be 0", gridBasedRefineSegmentation=1)
    refused("maxNNCountRefineSegmentation 1025 outside 1..1024", maxNNCountRefineSegmentation=1025)
    refused("params: maxNNCountRefineSegmentation 0 must be at least 1", maxNNCountRefineSegmentation=0)
    refused("iterationCountRefineSegmentation -1 is negative", iterationCountRefineSegmentation=-1)
    refused("params: occupancyResolution", occupancyResolution=8)
    refused("voxelDimensionGridBasedSegmentation 3 unsupported", grid_based=3)
    p = knn_params(fr, oracle, xyz)
    p.voxelDimensionRefineSegmentation, p.searchRadiusRefineSegmentation = 3, 1       # not read by this chain
    fr.segmenter_compute(p)
    assert_is_chain(state(fr), kc.host_chain(oracle, ("tiny", 0, 1)))
    few = gpu_ctx.frame(*kc.cloud("tiny[:256]"))
    nrm = np.random.default_rng(5).random((256, 3))
    few.set_normals(nrm)
    q = T.knn_refine_params(bits3d=kc.BITS3D)
    q.maxNNCountRefineSegmentation = 257
    with pytest.raises(T.Tmc2Error, match="error -4: segmenter_compute_knn_refine: maxNNCountRefineSegmentation 257 larger than the cloud \\(256 points\\)"):
        few.segmenter_compute(q)
    assert np.array_equal(bits(few.get_normals()), bits(nrm))
    # a cloud that holds K points whose voxel cloud does not: known after the voxelisation, which writes to scratch buffers only
    import grid_based_cases as gc
    mid_xyz, mid_rgb = kc.cloud("tiny[:600]")
    voxels = len(gc.voxelize(mid_xyz, 2)[0])
    assert 16 <= voxels < 256 <= len(mid_xyz)
    mid = gpu_ctx.frame(mid_xyz, mid_rgb)
    nrm = np.random.default_rng(6).random((len(mid_xyz), 3))
    mid.set_normals(nrm)
    with pytest.raises(T.Tmc2Error, match="error -4: .*leaves a voxel cloud of %d points, fewer than maxNNCountRefineSegmentation 256" % voxels):
        mid.segmenter_compute(T.knn_refine_params(bits3d=kc.BITS3D), grid_based=2)
    assert np.array_equal(bits(mid.get_normals()), bits(nrm))


# ---- GOF
def test_gpu_gof_phase_a_with_knn_refine_equals_single_frames(oracle):
    from tmc2_amd.synth import synth_cloud
    clouds = [synth_cloud("tiny", f) for f in range(2)]
    for grid in (None, 2):
        enc = T.GofEncoder(0, workers=2, bits3d=kc.BITS3D)
        frames = enc.upload(clouds)
        enc.phase_a(frames, grid_based_segmentation=grid, knn_refine_segmentation=(64, 10))
        weight = frames[0].weight_normal(kc.BITS3D, 0.6)
        gof_patches = enc.per_frame(frames, lambda g, i: g.get_patches())
        ctx = T.Context(0)
        for (xyz, rgb), b in zip(clouds, gof_patches):
            fr = ctx.frame(xyz, rgb)
            p = T.knn_refine_params(10, kc.BITS3D, weight)
            p.maxNNCountRefineSegmentation = 64
            fr.segmenter_compute(p, grid_based=grid)
            fr.encoder_pack_flexible(1280, 2, 1.0)
            a = fr.get_patches()
            assert len(a[0]) == len(b[0]) and all(np.array_equal(a[0][n], b[0][n]) for n in pc.PATCH_FIELDS + ("depthOffset", "occOffset"))
            assert all(np.array_equal(x, y) for x, y in zip(a[1:], b[1:]))
