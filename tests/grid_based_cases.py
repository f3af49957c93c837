"""Cases and yardsticks of the grid-based segmentation (the reference's fast mode): tests/test_grid_based_segmentation_host.py,
tests/test_gpu_grid_based_segmentation.py, tests/golden/make_grid_based_segmentation_golden.py.

voxelize() restates PCCPatchSegmenter3::convertPointsToVoxels in numpy: voxel = ( coordinate + voxDim / 2 ) >> log2 voxDim -- rounding,
not floor --, the voxels in the order of their FIRST point (not key order), every point the rank of its voxel in that list.
yardstick() is yardstick (a) of the chain: the oracle's own verified stages composed -- normals, initial segmentation and grid
refinement on the voxel cloud, a numpy copy back, then the k = 16 adjacency of the FULL cloud and segment_patches.  Yardstick (b)
is the fixture tests/golden/grid_based_segmentation.npz: digests of what the unmodified reference made of the same cases."""
import os

import numpy as np

import param_cases as pc

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "grid_based_segmentation.npz")
BITS3D = 11                     # geometryBitDepth3D of the chain cases (the clouds lie in 0..1023)
REFUSED_VOXEL_DIMENSIONS = (0, 1, 3, 6, 16)


def voxelize(xyz, vox_dim):
    """-> (voxel positions int16 [V][3] in first-occurrence order, rank of every point's voxel uint32 [n])"""
    shift = {2: 1, 4: 2, 8: 3}[vox_dim]
    v = (np.asarray(xyz).astype(np.int64).reshape(-1, 3) + (vox_dim >> 1)) >> shift
    key = v[:, 0] | (v[:, 1] << 20) | (v[:, 2] << 40)
    _, first, inverse = np.unique(key, return_index=True, return_inverse=True)
    rank_of_key = np.empty(len(first), np.int64)
    rank_of_key[np.argsort(first, kind="stable")] = np.arange(len(first))      # keys ranked by their first point
    return np.ascontiguousarray(v[np.sort(first)].astype(np.int16)), rank_of_key[inverse.reshape(-1)].astype(np.uint32)


def voxelize_loop(xyz, vox_dim):
    """the same as a plain loop with a dictionary (the reference's own form): what voxelize() is checked against"""
    shift, half, seen, vox, rank = {2: 1, 4: 2, 8: 3}[vox_dim], vox_dim >> 1, {}, [], []
    for p in np.asarray(xyz).astype(int).reshape(-1, 3).tolist():
        v = tuple((c + half) >> shift for c in p)
        if v not in seen:
            seen[v] = len(vox)
            vox.append(v)
        rank.append(seen[v])
    return np.array(vox, np.int16).reshape(-1, 3), np.array(rank, np.uint32)


# ---- the voxelisation on its own: name -> (xyz int16 [n][3], voxel size, bits)
SIZES = (1, 63, 64, 65, 255, 256, 257, 4097, 65537)     # around wavefront, workgroup and scan-block boundaries


def _surface(rng, n, extent=1024):
    """n points of a thin random sheet in random order, duplicates allowed: several points per voxel, voxels in no key order"""
    a = rng.integers(0, extent, (n, 2))
    z = (a[:, 0] // 3 + a[:, 1] // 5 + rng.integers(0, 3, n)) % extent
    return np.ascontiguousarray(np.stack([a[:, 0], a[:, 1], z], 1).astype(np.int16))


def voxel_cases():
    rng, out = np.random.default_rng(5601), {}
    for n in SIZES:
        out["n=%d" % n] = (_surface(rng, n, 64 if n < 5000 else 256), 2, 10)
    out["one_voxel"] = (np.ascontiguousarray((99 + rng.integers(0, 2, (1000, 3))).astype(np.int16)), 2, 10)     # 99, 100 -> voxel 50
    g = np.stack(np.meshgrid(np.arange(12), np.arange(12), np.arange(12)), -1).reshape(-1, 3)
    out["own_voxel"] = (np.ascontiguousarray((8 * g[rng.permutation(len(g))] + 16).astype(np.int16)), 8, 10)
    dup = _surface(rng, 300, 64)
    out["duplicates"] = (np.ascontiguousarray(np.concatenate([dup, dup[::-1], dup[::3]])), 4, 10)
    pts = np.unique(_surface(rng, 3000, 128), axis=0).astype(np.int64)
    key = (pts[:, 0] >> 1) | ((pts[:, 1] >> 1) << 10) | ((pts[:, 2] >> 1) << 20)
    out["descending_keys"] = (np.ascontiguousarray(pts[np.argsort(-key, kind="stable")].astype(np.int16)), 2, 10)
    for vd in (2, 4, 8):                              # x = half - 1 | half: voxel 0 | 1; 2^k - 1 lands on 2^k / voxDim, beyond a floor rule
        h = vd >> 1
        xs = [0, h - 1, h, vd - 1, vd, vd + h - 1, vd + h, 1023 - h, 1023]
        out["rounding_%d" % vd] = (np.ascontiguousarray(np.array([(x, y, 5) for x in xs for y in (0, h, 1023)], np.int16)), vd, 10)
    for bits in (10, 11, 12):
        top = (1 << bits) - 1
        p = rng.integers(top - 40, top + 1, (500, 3))
        p[::7] = top
        p[3] = (top, 0, top - 1)
        out["top_%d" % bits] = (np.ascontiguousarray(p.astype(np.int16)), 2, bits)
    return out


# ---- the chain: (cloud, voxel size, normalOrientation)
CHAIN = [(c, 2, 1) for c in ("tiny", "small", "plane", "two_sheets", "lattice", "slope", "medium")] + [("tiny", 4, 1), ("small", 4, 1), ("tiny", 2, 0),
                                                                                                       ("tiny_top", 2, 1)]

_clouds = {}


def cloud(name):
    """param_cases.cloud, and tiny_top: the tiny cloud moved against the far faces of the 10-bit cube -- its largest coordinate is
    1023 on every axis, so its voxel cloud reaches 512 = 2^(bits - 1) INCLUSIVE, a power of two that no plain frame hands S1-S5"""
    if name != "tiny_top":
        return pc.cloud(name)
    if name not in _clouds:
        xyz, rgb = pc.cloud("tiny")
        _clouds[name] = (np.ascontiguousarray((xyz.astype(np.int64) + (1023 - xyz.max(0))).astype(np.int16)), rgb)
    return _clouds[name]


def chain_id(case):
    return "%s-vox%d%s" % (case[0], case[1], "" if case[2] == 1 else "-orientation%d" % case[2])


def fast_overrides(params, orientation=1):
    """the four defaults the reference takes with the flag (PCCEncoderParameters.cpp:64-67) on a parameter struct of either binding"""
    params.maxNNCountRefineSegmentation = 384
    params.iterationCountRefineSegmentation = 5
    params.voxelDimensionRefineSegmentation = 2
    params.searchRadiusRefineSegmentation = 128
    params.normalOrientation = orientation
    return params


def oracle_fast_params(oracle, xyz, orientation=1):
    import oracle_binding as ob
    return fast_overrides(ob.seg_params(5, BITS3D, oracle.weight_normal(xyz, BITS3D, 0.6)), orientation)


_yardstick = {}


def yardstick(oracle, case):
    """yardstick (a), computed once per case and shared: dict(voxels, rank, normals, partition, knn, seg, params)"""
    if case not in _yardstick:
        name, vox_dim, orientation = case
        xyz, rgb = cloud(name)
        sp = oracle_fast_params(oracle, xyz, orientation)
        vox, rank = voxelize(xyz, vox_dim)
        nrm = oracle.normals(vox, 16, oriented=orientation == 1)
        w = np.array([sp.weightNormal[0], sp.weightNormal[1], sp.weightNormal[2]])
        part = oracle.refine_grid(vox, nrm, oracle.initial_segmentation(nrm, w), sp.maxNNCountRefineSegmentation, sp.lambdaRefineSegmentation,
                                  sp.iterationCountRefineSegmentation, sp.voxelDimensionRefineSegmentation, sp.searchRadiusRefineSegmentation)
        knn = oracle.knn_self(xyz, 16)
        partition = np.ascontiguousarray(part[rank])
        seg = oracle.segment_patches(xyz, rgb, knn, partition, sp)
        for a in (vox, rank, nrm, knn, partition):
            a.setflags(write=False)
        _yardstick[case] = dict(voxels=vox, rank=rank, normals=np.ascontiguousarray(nrm[rank]), partition=partition, knn=knn, seg=seg, params=sp)
    return _yardstick[case]


def digests(voxel_count, partition, seg):
    """what the fixture keeps of a case"""
    d = pc.result_digests(seg)
    return dict(voxel_count=int(voxel_count), partition=pc.digest(np.ascontiguousarray(partition, np.uint32)), patch_count=d["patch_count"],
                patches=d["patches"], depth0=d["depth0"], depth1=d["depth1"], occupancy=d["occupancy"])


def input_digest(case):
    xyz, rgb = cloud(case[0])
    return pc.digest(xyz) + pc.digest(rgb)
