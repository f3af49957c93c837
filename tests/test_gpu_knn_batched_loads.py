"""The k-NN kernels' loads (knn.hip): a node record in one 16-byte load, a leaf's points in one batch of pair loads, the last pair
of an odd-sized cloud reaching into the spare element behind the tree-order points.  Everything against the oracle, bit for bit,
on the smallest clouds at which these loads can go wrong: leaves that start at an odd tree position, leaves of exactly 10 points,
clouds of odd and even size whose last leaf ends at n, ties and duplicates.  The widest list (k = 32) has no entry point of its own
(tmc2_kdtree_search takes 1, 4, 8, 16): the metric's wide search runs it, tests/test_gpu_metrics_options.py."""
import numpy as np
import pytest

import tmc2_amd as T
from tmc2_amd.synth import synth_cloud

LEAF_MAX = 10


def cloud(name):
    rng = np.random.default_rng(5)
    if name == "duplicates":                         # 40 positions, 300 times each: every split falls back to count / 2
        return np.repeat(rng.integers(0, 1024, (40, 3)).astype(np.int16), 300, axis=0)
    if name == "eleven":                             # the smallest cloud that splits
        return rng.integers(0, 1024, (11, 3)).astype(np.int16)
    kind, frame, start, n = name.split(":")                 # n points of a synthetic frame from `start` on
    return np.ascontiguousarray(synth_cloud(kind, int(frame))[0][int(start):int(start) + int(n)])


# 17, 18, 33 and 1001 points; the frames / the offset are the first at which the oracle's tree has BOTH a leaf at an odd position
# and a leaf of 10 points (17: 7 + 10; 18: 7 + 1 + 10; 33: .. + 10 at 23; see the first test)
TAIL_CLOUDS = ["tiny:8:0:17", "tiny:0:69:18", "tiny:3:0:33", "small:0:0:1001"]
ALL_CLOUDS = TAIL_CLOUDS + ["duplicates", "eleven"]


def leaf_ranges(xyz, perm):
    """[a, b) of every leaf, in tree order: nanoflann's divideTree / middleSplit_ replayed over the permutation the build left (the
    points of a subtree are a contiguous range of it, so only the split INDEX has to be recomputed, not the swaps)."""
    pts = xyz[perm].astype(np.int64)
    out = []

    def divide(left, right, lo, hi):
        if right - left <= LEAF_MAX:
            out.append((left, right))
            return
        seg, span = pts[left:right], hi - lo
        mn, mx = seg.min(0), seg.max(0)
        dim, spread = 0, -1
        for d in range(3):
            if float(span[d]) > (1.0 - 0.00001) * float(span.max()) and mx[d] - mn[d] > spread:
                dim, spread = d, mx[d] - mn[d]
        cut = min(max(int((lo[dim] + hi[dim]) / 2), mn[dim]), mx[dim])
        count, lim1, lim2 = right - left, int((seg[:, dim] < cut).sum()), int((seg[:, dim] <= cut).sum())
        idx = lim1 if lim1 > count // 2 else (lim2 if lim2 < count // 2 else count // 2)
        assert seg[:idx, dim].max() <= cut <= seg[idx:, dim].min(), "the replay does not follow the permutation"
        lhi, rlo = hi.copy(), lo.copy()
        lhi[dim], rlo[dim] = cut, cut
        divide(left, left + idx, lo, lhi)
        divide(left + idx, right, rlo, hi)

    divide(0, len(pts), pts.min(0), pts.max(0))
    return out


@pytest.fixture(scope="module")
def trees(oracle):
    """name -> (xyz, perm, leaves), computed once"""
    out = {}
    for name in ALL_CLOUDS:
        xyz = cloud(name)
        perm = oracle.kdtree_perm(xyz)[0]
        out[name] = (xyz, perm, leaf_ranges(xyz, perm))
    return out


def test_the_clouds_have_the_leaves_the_loads_can_trip_over(trees):
    """No GPU: the oracle's own trees.  Every cloud has a leaf that starts at an odd tree position (its first pair begins one point
    before the leaf); every cloud but `eleven` (leaves of 5 and 6) has a leaf of exactly 10 points; a 10-point leaf at an odd
    position -- six pairs, the whole batch -- is there too; the host builder leaves the same permutation."""
    six_pairs = 0
    for name, (xyz, perm, leaves) in trees.items():
        assert leaves[0][0] == 0 and leaves[-1][1] == len(xyz) and all(a[1] == b[0] for a, b in zip(leaves, leaves[1:]))
        assert np.array_equal(T.host_kdtree_build(xyz)[0], perm), name
        assert any(a & 1 for a, b in leaves), name
        assert name == "eleven" or any(b - a == LEAF_MAX for a, b in leaves), name
        six_pairs += sum(1 for a, b in leaves if (a & 1) and b - a == LEAF_MAX)
    assert six_pairs > 0
    assert [len(trees[n][0]) & 1 for n in TAIL_CLOUDS] == [1, 0, 1, 1]


def queries_for(xyz, perm):
    """the cloud's last point in tree order first (its leaf's last pair is the one that reaches the spare element), every point of a
    small cloud / a spread of a larger one, and the same moved off the cloud"""
    own = xyz if len(xyz) <= 1001 else xyz[::37]
    off = (own.astype(np.int32) + np.array([3, -2, 5])).astype(np.int16)
    return np.concatenate([xyz[perm[-1:]], xyz[perm[-3:]], own, off])


def ks_for(n):
    return [k for k in (1, 4, 8, 16) if k <= n]


@pytest.mark.gpu
@pytest.mark.parametrize("name", TAIL_CLOUDS)
def test_gpu_tail_pair(gpu_ctx, oracle, trees, name):
    xyz, perm, _ = trees[name]
    fr = gpu_ctx.frame(xyz)
    q = queries_for(xyz, perm)
    for k in ks_for(len(xyz)):
        idx, d = fr.kdtree_search(q, k, with_dist=True)
        oi, od = oracle.knn(xyz, q, k, with_dist=True)
        assert np.array_equal(idx, oi) and np.array_equal(d.astype(np.float64), od), (name, k)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["duplicates", "eleven"])
def test_gpu_duplicates_and_ties_every_width(gpu_ctx, oracle, trees, name):
    xyz, perm, _ = trees[name]
    fr = gpu_ctx.frame(xyz)
    q = queries_for(xyz, perm)
    for k in ks_for(len(xyz)):
        idx, d = fr.kdtree_search(q, k, with_dist=True)
        oi, od = oracle.knn(xyz, q, k, with_dist=True)
        assert np.array_equal(idx, oi) and np.array_equal(d.astype(np.float64), od), (name, k)


@pytest.mark.gpu
@pytest.mark.parametrize("name", TAIL_CLOUDS + ["duplicates"])
def test_gpu_self_search(gpu_ctx, oracle, trees, name):
    xyz = trees[name][0]
    fr = gpu_ctx.frame(xyz)
    fr.normals_compute_normals(16)
    assert np.array_equal(fr.get_adjacency(16), oracle.knn(xyz, xyz, 16))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["tiny:3:0:33", "small:0:0:1001", "duplicates"])
def test_gpu_scratch_stack_form_and_root_box(gpu_ctx, oracle, trees, name):
    """queries beyond the packed-offset window take the scratch-stack kernel (the whole launch does); queries outside the root box
    start with non-zero offsets"""
    xyz, perm, _ = trees[name]
    fr = gpu_ctx.frame(xyz)
    wide = np.array([[-6000, 10, 10], [20000, 5, 5], [512, 512, -32768]], np.int16)
    wide = np.concatenate([wide, xyz[perm[-1:]], xyz[::max(1, len(xyz) // 50)]])
    far = np.array([[0, 0, 0], [1023, 1023, 1023], [500, -20, 2000], [-1, 300, 300], [1500, 1500, 1500]], np.int16)
    for q in (wide, far):
        for k in (1, 8, 16):
            idx, d = fr.kdtree_search(q, k, with_dist=True)
            oi, od = oracle.knn(xyz, q, k, with_dist=True)
            assert np.array_equal(idx, oi) and np.array_equal(d.astype(np.float64), od), (name, k)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["tiny:3:0:33", "small:0:0:1001"])
def test_gpu_split_path(gpu_ctx, oracle, trees, name):
    """transfer_colors: the easy pass's hit (targets that are source points, the last one in tree order among them), its "first
    identical point" rule (duplicate source positions with different colours), its miss (off-grid targets)"""
    xyz, perm, _ = trees[name]
    rng = np.random.default_rng(3)
    dup = rng.integers(0, len(xyz), max(4, len(xyz) // 8))
    src = np.concatenate([xyz, xyz[dup], xyz[dup[::2]]])
    order = rng.permutation(len(src))
    src = np.ascontiguousarray(src[order])
    rgb = rng.integers(0, 256, (len(src), 3)).astype(np.uint8)
    off = (xyz[::5].astype(np.int32) + rng.integers(-2, 3, (len(xyz[::5]), 3))).clip(0, 1023).astype(np.int16)
    sperm = oracle.kdtree_perm(src)[0]
    tgt = np.concatenate([src[sperm[-1:]], xyz, xyz[dup], off])
    assert np.array_equal(gpu_ctx.transfer_colors(src, rgb, tgt), oracle.transfer_colors(src, rgb, tgt))
