"""GPU tier (-m gpu) of the grid-based segmentation (the reference's fast mode): the device voxelisation on its own against the
host restatement, and Frame.segmenter_compute( params, grid_based = voxDim ) against yardstick (a) -- the oracle's verified stages
composed around the numpy voxelisation (tests/grid_based_cases.py) -- and yardstick (b) -- the digests of the unmodified reference
with gridBasedSegmentation_ set (tests/golden/grid_based_segmentation.npz; the CPU tier shows that (a) == (b)).  Everything is
exact equality.  Every chain case has a voxel cloud of at least 16 points (checked on the CPU tier against the fixture); the clouds
that have not are the refusal cases here."""
import numpy as np
import pytest

import grid_based_cases as gc
import param_cases as pc
import tmc2_amd as T

pytestmark = pytest.mark.gpu

VOXEL_CASES = gc.voxel_cases()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def golden():
    return np.load(gc.FIXTURE)


def fast_params(fr, oracle, xyz, orientation=1):
    """fast_params() with the projection weights of the ORIGINAL cloud (S0), checked against the oracle's"""
    w = fr.weight_normal(gc.BITS3D, 0.6)
    assert np.array_equal(bits(w), bits(oracle.weight_normal(xyz, gc.BITS3D, 0.6)))
    p = T.fast_params(bits3d=gc.BITS3D, weight=w)
    p.normalOrientation = orientation
    return p


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


def assert_is_yardstick(got, y):
    """normals as bit patterns (copies of the voxels'), partition, the FULL cloud's adjacency, patch records, pools"""
    assert np.array_equal(bits(got["normals"]), bits(y["normals"])), "normals of the points"
    assert np.array_equal(got["partition"], y["partition"]), "partition"
    assert np.array_equal(got["knn"], y["knn"]), "adjacency (the full cloud's)"
    seg = y["seg"]
    assert len(got["patches"]) == len(seg["patches"])
    for n in pc.PATCH_FIELDS:
        assert np.array_equal(got["patches"][n], seg["patches"][n]), n
    assert np.array_equal(got["depth0"], seg["depth0"]) and np.array_equal(got["depth1"], seg["depth1"]), "depth pools"
    assert np.array_equal(got["occupancy"], seg["occupancy"]), "occupancy"


# ---- the voxelisation alone
@pytest.mark.parametrize("name", list(VOXEL_CASES))
def test_gpu_convert_points_to_voxels_matches_host(gpu_ctx, name):
    """device against the host entry and the numpy restatement: the voxel list with its order, and the rank per point"""
    xyz, vox_dim, nbits = VOXEL_CASES[name]
    vox, rank = gpu_ctx.convert_points_to_voxels(xyz, vox_dim, nbits)
    host_vox, host_rank = T.host_convert_points_to_voxels(xyz, vox_dim, nbits)
    want_vox, want_rank = gc.voxelize(xyz, vox_dim)
    assert np.array_equal(host_vox, want_vox) and np.array_equal(host_rank, want_rank)
    assert np.array_equal(vox, want_vox), "voxel list (positions or order)"
    assert np.array_equal(rank, want_rank), "rank of the points' voxels"


def test_gpu_convert_points_to_voxels_refuses_like_the_host(gpu_ctx):
    xyz = VOXEL_CASES["n=257"][0]
    for vox_dim in gc.REFUSED_VOXEL_DIMENSIONS:
        with pytest.raises(T.Tmc2Error, match="voxelDimensionGridBasedSegmentation %d unsupported" % vox_dim):
            gpu_ctx.convert_points_to_voxels(xyz, vox_dim, 10)
    with pytest.raises(T.Tmc2Error, match="voxel coordinate 1024 does not fit geometryBitDepth3D 10 bits"):
        gpu_ctx.convert_points_to_voxels(np.array([[1, 2, 3], [5, 2047, 7]], np.int16), 2, 10)


# ---- the whole chain
@pytest.mark.parametrize("case", gc.CHAIN, ids=gc.chain_id)
def test_gpu_grid_based_segmentation_matches_oracle_and_reference(gpu_ctx, oracle, golden, case):
    cloud, vox_dim, orientation = case
    name = gc.chain_id(case)
    xyz, rgb = gc.cloud(cloud)
    assert gc.input_digest(case) == str(golden[name + "/input_md5"]), "generated input differs from the fixture's"
    y = gc.yardstick(oracle, case)
    fr = gpu_ctx.frame(xyz, rgb)
    p = fast_params(fr, oracle, xyz, orientation)
    gpu_ctx.stage_reset()
    fr.segmenter_compute(p, grid_based=vox_dim)
    calls = gpu_ctx.stage_calls()
    got = state(fr)
    assert_is_yardstick(got, y)
    assert calls.get("patches_build", 0) == len(y["seg"]["round_raw"])
    assert calls.get("voxelize", 0) == 1 and calls.get("voxels_to_points", 0) == 1 and calls.get("knn_self", 0) == 2   # voxels, then points
    d = gc.digests(len(y["voxels"]), got["partition"], dict(patches=got["patches"], depth0=got["depth0"], depth1=got["depth1"], occupancy=got["occupancy"]))
    assert pc.digest(got["normals"]) == str(golden[name + "/normals_md5"])
    for k in ("partition", "patches", "depth0", "depth1", "occupancy"):
        assert d[k] == str(golden[name + "/" + k + "_md5"]), "reference: " + k
    assert d["patch_count"] == int(golden[name + "/patch_count"])


# ---- refusals: by name, before anything is launched, the frame left as it was
def test_gpu_grid_based_segmentation_refusals_leave_the_frame_unchanged(gpu_ctx, oracle):
    xyz, rgb = gc.cloud("tiny")
    fr = gpu_ctx.frame(xyz, rgb)
    p = fast_params(fr, oracle, xyz)
    fr.segmenter_compute(T.ctc_params(3, gc.BITS3D, fr.weight_normal(gc.BITS3D, 0.6)))
    before = state(fr)
    for vox_dim in gc.REFUSED_VOXEL_DIMENSIONS:
        with pytest.raises(T.Tmc2Error, match="error -?\\d+: .*voxelDimensionGridBasedSegmentation %d unsupported" % vox_dim):
            fr.segmenter_compute(p, grid_based=vox_dim)
        assert_same_state(state(fr), before)
    p.geometryBitDepth3D = 8                                        # tiny reaches beyond 2 * 255: its voxels do not fit 8 bits
    assert xyz.max() > 511
    with pytest.raises(T.Tmc2Error, match="does not fit geometryBitDepth3D 8 bits"):
        fr.segmenter_compute(p, grid_based=2)
    assert_same_state(state(fr), before)
    bad = T.fast_params(bits3d=gc.BITS3D)
    bad.occupancyResolution = 8                                     # the parameter check comes first and refuses what it refuses today
    with pytest.raises(T.Tmc2Error, match="params: occupancyResolution"):
        fr.segmenter_compute(bad, grid_based=2)
    assert_same_state(state(fr), before)


def test_gpu_grid_based_segmentation_refuses_a_voxel_cloud_below_sixteen_points(gpu_ctx):
    """40 points inside one voxel, and 40 points in 15 voxels: refused by name; 16 voxels are the k-NN's own limit"""
    rng = np.random.default_rng(3)
    one = np.ascontiguousarray((99 + rng.integers(0, 2, (40, 3))).astype(np.int16))
    fifteen = np.ascontiguousarray(np.concatenate([np.array([[10 + 2 * k, 20, 30] for k in range(15)]), 10 + 2 * rng.integers(0, 15, (25, 1)) * [1, 0, 0] + [0, 10, 20]]).astype(np.int16))
    assert len(gc.voxelize(one, 2)[0]) == 1 and len(gc.voxelize(fifteen, 2)[0]) == 15
    for xyz in (one, fifteen):
        rgb = rng.integers(0, 256, (len(xyz), 3), dtype=np.uint8)
        fr = gpu_ctx.frame(xyz, rgb)
        nrm = rng.random((len(xyz), 3))                          # (a state to find unchanged; no stage runs on these degenerate clouds)
        fr.set_normals(nrm)
        with pytest.raises(T.Tmc2Error, match="voxelDimensionGridBasedSegmentation 2 leaves a voxel cloud of %d points" % len(gc.voxelize(xyz, 2)[0])):
            fr.segmenter_compute(T.fast_params(bits3d=gc.BITS3D), grid_based=2)
        assert np.array_equal(bits(fr.get_normals()), bits(nrm))


# ---- no state leaks
def test_gpu_fast_and_plain_on_one_frame_give_their_own_results(gpu_ctx, oracle):
    import oracle_binding as ob
    case = ("tiny", 2, 1)
    xyz, rgb = gc.cloud("tiny")
    y = gc.yardstick(oracle, case)
    w = oracle.weight_normal(xyz, gc.BITS3D, 0.6)
    plain = oracle.segment(xyz, rgb, ob.seg_params(3, gc.BITS3D, w))
    assert len(plain["patches"]) != len(y["seg"]["patches"])           # the two yardsticks differ on this cloud

    def check_plain(fr):
        fr.segmenter_compute(T.ctc_params(3, gc.BITS3D, w))
        got = state(fr)
        assert len(got["patches"]) == len(plain["patches"])
        for n in pc.PATCH_FIELDS:
            assert np.array_equal(got["patches"][n], plain["patches"][n]), n
        assert np.array_equal(got["depth0"], plain["depth0"]) and np.array_equal(got["depth1"], plain["depth1"]) and np.array_equal(got["occupancy"], plain["occupancy"])
        assert np.array_equal(bits(got["normals"]), bits(oracle.normals(xyz)))

    def check_fast(fr):
        fr.segmenter_compute(fast_params(fr, oracle, xyz), grid_based=2)
        assert_is_yardstick(state(fr), y)

    a = gpu_ctx.frame(xyz, rgb)
    check_fast(a), check_plain(a), check_fast(a)
    b = gpu_ctx.frame(xyz, rgb)
    check_plain(b), check_fast(b), check_plain(b)


def test_gpu_three_fast_calls_are_identical_and_the_pool_stops_growing(oracle):
    ctx = T.Context(0)
    xyz, rgb = gc.cloud("small")
    fr = ctx.frame(xyz, rgb)
    p = fast_params(fr, oracle, xyz)
    results, stats = [], []
    for _ in range(3):
        fr.segmenter_compute(p, grid_based=2)
        results.append(state(fr))
        stats.append(ctx.pool_stats())
    assert_same_state(results[0], results[1]), assert_same_state(results[1], results[2])
    assert_is_yardstick(results[2], gc.yardstick(oracle, ("small", 2, 1)))
    assert stats[2]["bytes_held"] == stats[1]["bytes_held"] and stats[2]["hipmalloc_calls"] == stats[1]["hipmalloc_calls"], stats


# ---- downstream once
def test_gpu_fast_result_packs_and_rasterises_like_the_oracle(gpu_ctx, oracle):
    xyz, rgb = gc.cloud("tiny")
    seg = gc.yardstick(oracle, ("tiny", 2, 1))["seg"]
    fr = gpu_ctx.frame(xyz, rgb)
    fr.segmenter_compute(fast_params(fr, oracle, xyz), grid_based=2)
    h = fr.encoder_pack_flexible(1280, 2, 1.0)
    placed, order, oh = oracle.pack_flexible(seg["patches"], seg["occupancy"], 1280)
    assert h == oh and np.array_equal(fr.get_patch_order(), order)
    got = fr.get_patches()[0]
    for k in ("u0", "v0", "patchOrientation"):
        assert np.array_equal(got[k], placed[k]), k
    W, H = T.encoder_canvas_size([h], 1280, 1280, 1280)
    fr.encoder_generate_geometry_images(W, H, 4)
    img, want = fr.get_geometry_images(), oracle.geometry_images(placed, order, seg["depth0"], seg["depth1"], W, H, 16, 4)
    for k in ("occupancy", "occ_video", "block_to_patch", "geo0", "geo1"):
        assert np.array_equal(img[k], want[k]), k


# ---- GOF
def test_gpu_gof_phase_a_with_grid_based_segmentation_equals_single_frames(oracle):
    from tmc2_amd.synth import synth_cloud
    clouds = [synth_cloud("tiny", f) for f in range(2)]
    enc = T.GofEncoder(0, workers=2, bits3d=gc.BITS3D)
    frames = enc.upload(clouds)
    W, H = enc.phase_a(frames, grid_based_segmentation=2)
    imgs = enc.per_frame(frames, lambda fr, i: fr.get_geometry_images())
    weight = frames[0].weight_normal(gc.BITS3D, 0.6)
    ctx = T.Context(0)
    heights, singles = [], []
    for xyz, rgb in clouds:
        fr = ctx.frame(xyz, rgb)
        fr.segmenter_compute(T.fast_params(bits3d=gc.BITS3D, weight=weight), grid_based=2)
        heights.append(fr.encoder_pack_flexible(1280, 2, 1.0))
        singles.append(fr)
    assert (W, H) == T.encoder_canvas_size([max(heights)], 1280, 1280, 1280)
    gof_patches = enc.per_frame(frames, lambda g, i: g.get_patches())
    for fr, b, img in zip(singles, gof_patches, imgs):
        a = fr.get_patches()
        assert len(a[0]) == len(b[0]) and all(np.array_equal(a[0][n], b[0][n]) for n in pc.PATCH_FIELDS + ("depthOffset", "occOffset"))
        assert all(np.array_equal(x, y) for x, y in zip(a[1:], b[1:]))
        fr.encoder_generate_geometry_images(W, H, enc.occ_precision)
        want = fr.get_geometry_images()
        for k in ("occupancy", "occ_video", "block_to_patch", "geo0", "geo1"):
            assert np.array_equal(img[k], want[k]), k
