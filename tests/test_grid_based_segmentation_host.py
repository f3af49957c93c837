"""CPU tier of the grid-based segmentation (the reference's fast mode, PCCPatchSegmenter3::compute with gridBasedSegmentation_:
PCCPatchSegmenter.cpp:78-149, convertPointsToVoxels :152-181, applyVoxelsDataToPoints :183-215).

tmc2_host_convert_points_to_voxels -- csrc/voxelize.h, the rule the device kernels run, compiled for the host -- against the numpy
restatement of tests/grid_based_cases.py; the oracle's stages composed around that restatement (yardstick (a) of the GPU tier)
against what the UNMODIFIED reference made of the same clouds with the flag set (tests/golden/grid_based_segmentation.npz, generated
by tests/golden/make_grid_based_segmentation_golden.py); the refusals that need no device.  Everything is exact equality.
The refusals of tmc2_segmenter_compute_grid_based on a frame (message, frame left unchanged) need a frame, hence a device: they
are in tests/test_gpu_grid_based_segmentation.py."""
import numpy as np
import pytest

import grid_based_cases as gc
import param_cases as pc
import tmc2_amd as T

VOXEL_CASES = gc.voxel_cases()


@pytest.fixture(scope="module")
def golden():
    return np.load(gc.FIXTURE)


@pytest.mark.parametrize("name", [n for n, c in VOXEL_CASES.items() if len(c[0]) <= 5000])
def test_numpy_restatement_is_the_plain_loop(name):
    """the vectorised restatement against the reference's own form, a loop over the points with a dictionary"""
    xyz, vox_dim, _ = VOXEL_CASES[name]
    vox, rank = gc.voxelize(xyz, vox_dim)
    vox2, rank2 = gc.voxelize_loop(xyz, vox_dim)
    assert np.array_equal(vox, vox2) and np.array_equal(rank, rank2)


def test_cases_hold_the_traps():
    """The shapes say what their names promise: a list that is not in key order, rounding that a floor rule gets wrong, voxels
    beyond a floor rule's range."""
    xyz, vd, _ = VOXEL_CASES["descending_keys"]
    vox, rank = gc.voxelize(xyz, vd)
    key = vox[:, 0].astype(np.int64) | (vox[:, 1].astype(np.int64) << 16) | (vox[:, 2].astype(np.int64) << 32)
    assert (np.diff(key) < 0).sum() > len(key) // 2                      # first-occurrence order here is far from ascending key order
    assert len(gc.voxelize(VOXEL_CASES["one_voxel"][0], 2)[0]) == 1
    assert len(gc.voxelize(VOXEL_CASES["own_voxel"][0], 8)[0]) == len(VOXEL_CASES["own_voxel"][0])
    assert len(gc.voxelize(VOXEL_CASES["duplicates"][0], 4)[0]) < 300
    for vd in (2, 4, 8):
        xyz = VOXEL_CASES["rounding_%d" % vd][0]
        vox, rank = gc.voxelize(xyz, vd)
        of = {int(x): int(vox[r][0]) for (x, _, _), r in zip(xyz.tolist(), rank)}
        half = vd >> 1
        assert of[half - 1] == 0 and of[half] == 1 and of[1023] == 1024 // vd     # a floor rule: 0, 0 (voxels of 2: x = 1) and 1024 / vd - 1
    for bits in (10, 11, 12):
        vox, _ = gc.voxelize(VOXEL_CASES["top_%d" % bits][0], 2)
        assert vox.max() == 1 << (bits - 1)                               # one beyond what fits bits - 1 bits


@pytest.mark.parametrize("name", list(VOXEL_CASES))
def test_host_convert_points_to_voxels_matches_restatement(name):
    xyz, vox_dim, bits = VOXEL_CASES[name]
    vox, rank = T.host_convert_points_to_voxels(xyz, vox_dim, bits)
    want_vox, want_rank = gc.voxelize(xyz, vox_dim)
    assert np.array_equal(vox, want_vox), "voxel list (positions or order)"
    assert np.array_equal(rank, want_rank), "rank of the points' voxels"


@pytest.mark.parametrize("vox_dim", gc.REFUSED_VOXEL_DIMENSIONS)
def test_host_refuses_voxel_dimension(vox_dim):
    xyz = VOXEL_CASES["n=257"][0]
    with pytest.raises(T.Tmc2Error, match="voxelDimensionGridBasedSegmentation %d unsupported" % vox_dim):
        T.host_convert_points_to_voxels(xyz, vox_dim, 10)


def test_host_refuses_voxel_coordinates_beyond_the_bit_depth():
    """2^bits - 1 itself is fine (its voxel is 2^(bits-1)), and so is any coordinate whose voxel still fits bits bits; a voxel
    coordinate that needs more is refused by name, and so is a negative coordinate."""
    xyz = np.array([[1, 2, 3], [1023, 0, 0], [5, 2046, 7]], np.int16)
    assert T.host_convert_points_to_voxels(xyz, 2, 10)[0].tolist() == [[1, 1, 2], [512, 0, 0], [3, 1023, 4]]
    with pytest.raises(T.Tmc2Error, match="voxel coordinate 1024 does not fit geometryBitDepth3D 10 bits"):
        T.host_convert_points_to_voxels(np.array([[1, 2, 3], [5, 2047, 7]], np.int16), 2, 10)
    with pytest.raises(T.Tmc2Error, match="voxel coordinate 512 does not fit geometryBitDepth3D 9 bits"):
        T.host_convert_points_to_voxels(xyz[:2], 2, 9)
    with pytest.raises(T.Tmc2Error, match="negative.*geometryBitDepth3D 10"):
        T.host_convert_points_to_voxels(np.array([[0, -1, 5]], np.int16), 2, 10)


def test_forty_points_in_one_voxel_are_one_voxel():
    """what the chain refuses (fewer than 16 voxels; GPU tier) is, on the host, a voxel cloud of one point"""
    xyz = np.ascontiguousarray((99 + np.random.default_rng(3).integers(0, 2, (40, 3))).astype(np.int16))
    vox, rank = T.host_convert_points_to_voxels(xyz, 2, 10)
    assert vox.tolist() == [[50, 50, 50]] and not rank.any()


def test_fixture_is_not_vacuous(golden):
    names = [str(n) for n in golden["names"]]
    assert names == [gc.chain_id(c) for c in gc.CHAIN]
    counts = {n: (int(golden[n + "/voxel_count"]), int(golden[n + "/patch_count"])) for n in names}
    for case in gc.CHAIN:
        n = gc.chain_id(case)
        assert 16 <= counts[n][0] <= len(gc.cloud(case[0])[0]) and counts[n][1] >= 1
        assert float(golden[n + "/reference_seconds"][0]) > 0
    assert counts["tiny-vox2"][0] < len(gc.cloud("tiny")[0]) // 3            # the front of the segmenter sees a third of the points
    assert counts["tiny-vox2"] != counts["tiny-vox4"]


@pytest.mark.parametrize("case", gc.CHAIN, ids=gc.chain_id)
def test_composed_oracle_stages_match_reference_fast_mode(oracle, golden, case):
    """yardstick (a) == yardstick (b): voxel count, partition of the points, patch records, both depth pools, occupancy"""
    name = gc.chain_id(case)
    assert gc.input_digest(case) == str(golden[name + "/input_md5"]), "generated input differs from the fixture's"
    y = gc.yardstick(oracle, case)
    got = gc.digests(len(y["voxels"]), y["partition"], y["seg"])
    assert got["voxel_count"] == int(golden[name + "/voxel_count"])
    assert pc.digest(y["normals"]) == str(golden[name + "/normals_md5"]), "normals of the points"
    for k in ("partition", "patches", "depth0", "depth1", "occupancy"):
        assert got[k] == str(golden[name + "/" + k + "_md5"]), k
    assert got["patch_count"] == int(golden[name + "/patch_count"])
