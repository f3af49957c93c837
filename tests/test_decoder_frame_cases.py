"""CPU tier: the hand-built decoder frames of tests/decoder_frame_cases.py.  The numpy references against the oracle's restatement
(two texts of the same reference functions written apart), every scene's condition from the references alone, and the oracle's T3 +
T4 against the unmodified reference on every scene and (grid, threshold) pair -- what pins the oracle at these edges before
tests/test_gpu_decoder_frames.py holds the device against it."""
import numpy as np
import pytest

import decoder_frame_cases as dc


def _image(s, r):
    return dict(patches=s["patches"], width=s["W"], height=s["H"], occ_video=s["occ_video"], block_to_patch=r["block_to_patch"],
                geo0=s["geo0"], geo1=s["geo1"])


def _moved(oracle, r, pair):
    if len(r["xyz"]) == 0:
        return 0
    return int((oracle.smooth_point_cloud_grid(r["xyz"], r["boundary"], r["partition"], *pair)[1] == 3).sum())


@pytest.mark.parametrize("name", dc.NAMES + dc.OVERFLOW_NAMES)
def test_numpy_references_equal_the_oracle(oracle, name):
    s, r = dc.scene(name), dc.scene_references(name)
    xyz, p2p = oracle.generate_point_cloud(_image(s, r))
    assert np.array_equal(xyz, r["xyz"]) and np.array_equal(p2p, r["point_to_pixel"])
    assert np.array_equal(oracle.identify_boundary_points(r["point_to_pixel"], s["occ_video"], s["W"], s["H"], s["prec"]), r["boundary"])
    assert int(r["per_patch"].sum()) == len(r["xyz"]) and r["xyz"].min() >= 0 and r["xyz"].max() < 2048
    assert max(s["W"], s["H"]) <= (256 if name in dc.OVERFLOW_NAMES else 128)
    assert np.array_equal(np.bincount(r["partition"], minlength=len(s["patches"])), r["per_patch"])


@pytest.mark.parametrize("name", dc.NAMES)
def test_moved_points_at_the_grid_threshold_pairs(oracle, name):
    """where a scene is meant to move points the oracle alone moves at least 20, where it is meant not to exactly 0"""
    r = dc.scene_references(name)
    for pair in dc.PAIRS:
        want, moved = dc.expectation(name, pair), _moved(oracle, r, pair)
        assert want is None or (moved >= 20 if want == "moves" else moved == 0), (pair, want, moved)


def test_borders_condition():
    s, r = dc.scene("borders"), dc.scene_references("borders")
    x, y = r["point_to_pixel"][:, 0].astype(int), r["point_to_pixel"][:, 1].astype(int)
    for near in (x < 2, y < 2, x >= s["W"] - 2, y >= s["H"] - 2):
        assert near.any() and (r["boundary"][near] == 1).all()
    for cx, cy in ((0, 0), (s["W"] - 1, 0), (0, s["H"] - 1), (s["W"] - 1, s["H"] - 1)):
        assert ((x == cx) & (y == cy)).any()                          # all four corner pixels emit points
    assert set(s["patches"]["patchOrientation"]) == {0, 1}
    turned = [(int(p["sizeU0"]), int(p["sizeV0"])) for p in s["patches"] if p["patchOrientation"] == 1]
    assert (3, 1) in turned and (1, 3) in turned


def test_overlap_condition():
    s, r = dc.scene("overlap"), dc.scene_references("overlap")
    n = r["per_patch"]
    assert any(n[k] == 0 and n[:k].any() and n[k + 1:].any() for k in range(len(n)))
    assert r["block_to_patch"][1, 1] == 3                                  # the block patches 0 and 2 share goes to the later one
    assert n[1] == 0 and not (r["block_to_patch"] == 2).any()              # patch 1's blocks are all patch 4's
    assert n[3] == 0 and not s["occ_video"][48 // s["prec"]:, :32 // s["prec"]].any()      # patch 3: wholly empty occupancy


def test_axes_condition():
    s, r = dc.scene("axes"), dc.scene_references("axes")
    p = s["patches"]
    seen = {(int(p["normalAxis"][k]), int(p["projectionMode"][k])) for k in range(len(p)) if r["per_patch"][k] > 0}
    assert seen == {(a, m) for a in range(3) for m in range(2)}
    for k in range(len(p)):
        assert (int(p["tangentAxis"][k]), int(p["bitangentAxis"][k])) == dc.AXES[int(p["normalAxis"][k])]
    clamp = len(p) - 1                                                     # depth > d1 on both layers: one point per pixel, at 0
    mine = r["partition"] == clamp
    assert r["per_patch"][clamp] == 512 and (r["xyz"][mine, 2] == 0).all() and (r["point_to_pixel"][mine, 2] == 0).all()
    assert (s["geo0"][16:32, 32:64] > 10).all() and (s["geo1"][16:32, 32:64] > 10).all()


def test_layers_condition():
    s, r = dc.scene("layers"), dc.scene_references("layers")
    p2p = r["point_to_pixel"].astype(int)
    tile = (p2p[:, 1] // 16) * 4 + p2p[:, 0] // 16
    mine = r["partition"] == 0
    per_tile = np.bincount(tile[mine], minlength=8)
    assert per_tile[0] == 512 and per_tile[1] == 256 and per_tile[2] == 512 and per_tile[7] == 0
    below = mine & (tile == 2) & (p2p[:, 2] == 1)
    assert (r["xyz"][below, 2] < r["xyz"][np.flatnonzero(below) - 1, 2]).all()     # D1 under D0
    for t, lane in zip((3, 4, 5, 6), dc.LAYER_LANES):
        q = p2p[mine & (tile == t)]
        assert len({(a, b) for a, b, _ in q}) == 1 and (q[0, 1] % 16) * 16 + q[0, 0] % 16 == lane


def test_precisions_condition():
    lists = [dc.scene("precisions-%d" % p)["patches"] for p in dc.PRECISIONS]
    assert all(np.array_equal(lists[0], l) for l in lists[1:])
    share = []
    for p in dc.PRECISIONS:
        s, r = dc.scene("precisions-%d" % p), dc.scene_references("precisions-%d" % p)
        assert s["prec"] == p and s["occ_video"].shape == (64 // p, 64 // p)
        share.append(r["boundary"].mean())
    assert all(a > b for a, b in zip(share, share[1:]))                    # coarser occupancy: fewer boundary points


def test_coincident_condition():
    r = dc.scene_references("coincident")
    _, inverse, count = np.unique(r["xyz"], axis=0, return_inverse=True, return_counts=True)
    assert (count[inverse.ravel()] > 1).mean() >= 0.3


@pytest.mark.parametrize("variant", dc.FACE_VARIANTS)
@pytest.mark.parametrize("grid", dc.FACE_GRIDS)
def test_faces_condition(grid, variant):
    name = "faces-g%d-%+d" % (grid, variant)
    r = dc.scene_references(name)
    top, targets = dc.face_targets(grid, variant)
    w, th, disth = dc.grid_geometry(r["xyz"], grid)
    assert int(r["xyz"].max()) == top and w == (top + grid - 1) // grid
    assert [c for c in (disth - 1, disth, th - disth - 1, th - disth) if c <= top] == targets and len(targets) >= 2
    P = r["xyz"].astype(int)
    for axis in range(3):
        others = [a for a in range(3) if a != axis]
        clear = ((P[:, others] >= disth) & (P[:, others] + disth < th)).all(axis=1)      # only this axis decides "outside"
        for c in targets:
            assert ((P[:, axis] == c) & clear & (r["boundary"] == 1)).any(), (axis, c)
    if th - disth - 1 <= top:                                             # the cells at the upper faces see two patches
        at = (P[:, 2] == th - disth - 1) & ~dc.outside(r["xyz"], grid)
        assert len(set(r["partition"][at])) >= 2


def test_single_condition(oracle):
    for name in dc.STILL_EVERYWHERE:
        r = dc.scene_references(name)
        assert len(dc.scene(name)["patches"]) == 1 and all(_moved(oracle, r, pair) == 0 for pair in dc.PAIRS)
    assert len(dc.scene_references("single-small")["xyz"]) < 8


def test_sparse_condition():
    r = dc.scene_references("sparse")
    who, count, armed = dc.blend_counts(r["xyz"], r["boundary"], 16, r["partition"])
    assert (armed & (count == 0)).any() and (armed & (count > 0)).any()     # the 0 / 0 path is reached, and so is the other one


def test_blend_counts_is_the_oracles_count(oracle):
    """blend_counts against the oracle's own arithmetic: with a threshold of 0 a point moves iff dist2 >= 2 count, and a blended
    count of 0 never moves -- so no point that blend_counts puts at 0 may be moved by the oracle at any threshold"""
    for name in ("sparse", "faces-g8-+1", "coincident"):
        r = dc.scene_references(name)
        who, count, armed = dc.blend_counts(r["xyz"], r["boundary"], 16, r["partition"])
        bt = oracle.smooth_point_cloud_grid(r["xyz"], r["boundary"], r["partition"], 16, 0.0)[1]
        assert (bt[who[count == 0]] == 1).all() and (bt[who[~armed]] == 1).all()


def test_random_condition():
    assert len(dc.RANDOM_NAMES) == 60
    for c, (W, H, prec) in enumerate(dc.RANDOM_CANVASES):
        for seed in dc.RANDOM_SEEDS[c]:
            s = dc.scene("random-%d-%dx%d-p%d" % (seed, W, H, prec))
            assert (s["W"], s["H"], s["prec"], len(s["patches"])) == (W, H, prec, 5)


@pytest.mark.parametrize("name", dc.OVERFLOW_NAMES)
def test_cell_overflow_condition(name):
    r = dc.scene_references(name)
    P = r["xyz"].astype(np.int64)
    assert not dc.outside(r["xyz"], 64).any() and len({tuple(c) for c in P // 64}) == 1      # one cell, inside the faces
    assert (r["boundary"] == 1).any()
    if name.endswith("count"):
        assert len(P) > 65535 and P.sum(axis=0).max() < 1 << 24
    else:
        assert len(P) <= 65535 and P.sum(axis=0).max() >= 1 << 24


@pytest.mark.parametrize("name", dc.NAMES)
def test_oracle_tail_matches_reference_on_decoder_frames(oracle, reference, name):
    """smoothPointCloudPostprocess + transferColors16bitBP of the unmodified reference on every scene's points against the oracle's
    T3 + T4 at every pair: positions, boundary types, colours"""
    s, r = dc.scene(name), dc.scene_references(name)
    c16 = oracle.color_point_cloud(r["point_to_pixel"], dc.attribute_planes(s, "random"))
    for grid, threshold in dc.PAIRS:
        rx, rb, rc = reference.smooth_and_transfer(r["xyz"], r["boundary"], r["partition"], c16, grid, threshold)
        ox, ob_ = oracle.smooth_point_cloud_grid(r["xyz"], r["boundary"], r["partition"], grid, threshold)
        assert np.array_equal(rx, ox) and np.array_equal(rb, ob_), (grid, threshold)
        assert np.array_equal(rc, oracle.transfer_colors16_bp(r["xyz"], c16, ox, ob_)), (grid, threshold)


def test_oracle_refuses_an_odd_grid_size(oracle):
    r = dc.scene_references("borders")
    for grid in (3, 5, 63, 1):
        with pytest.raises(ValueError):
            oracle.smooth_point_cloud_grid(r["xyz"], r["boundary"], r["partition"], grid, 64.0)
    x, bt = oracle.smooth_point_cloud_grid(r["xyz"], r["boundary"], r["partition"], 8, 64.0)
    assert (bt == 3).sum() >= 20
