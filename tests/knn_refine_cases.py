"""Cases and yardsticks of the k-NN refinement of the segmentation (the reference's non-grid mode, gridBasedRefineSegmentation off):
tests/test_knn_refine_segmentation_host.py, tests/test_gpu_knn_refine_segmentation.py,
tests/golden/make_knn_refine_segmentation_golden.py.

The neighbourhood of a point is a SET: the first K points under the key (squared distance, position in the query's own depth-first
visiting order of nanoflann's tree).  Rows are therefore compared sorted; the fixture keeps a CRC32 of every sorted row, so that a
failure names its first row.  brute_force_bound() is the part of the definition that needs no tree: every row holds exactly K
different points, all points closer than its K-th distance and none farther.  host_chain() is the chain's yardstick that needs no
reference: the oracle's normals and initial segmentation, the host restatement of the refinement, the oracle's segment_patches."""
import os
import zlib

import numpy as np

import grid_based_cases as gc
import param_cases as pc

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "knn_refine_segmentation.npz")
BITS3D = 11
K, LAMBDA, ITERATIONS = 256, 3.0, 100          # the reference's defaults with the flag off


# ---- clouds: param_cases.cloud, and three made of tiny
def cloud(name):
    if name == "twice":                        # every position twice: tiny[:3000] followed by its reverse
        xyz, rgb = pc.cloud("tiny")
        return np.ascontiguousarray(np.concatenate([xyz[:3000], xyz[:3000][::-1]])), np.ascontiguousarray(np.concatenate([rgb[:3000], rgb[:3000][::-1]]))
    if name.startswith("tiny[:"):              # the first 256 / 257 points of tiny: K = n and K = n - 1
        xyz, rgb = pc.cloud("tiny")
        m = int(name[6:-1])
        return np.ascontiguousarray(xyz[:m]), np.ascontiguousarray(rgb[:m])
    return pc.cloud(name)


# ---- adjacency: (cloud, K, foreign) -- foreign: the queries are the cloud's points + 1 against the cloud's own tree
ADJACENCY = [("lattice", 256, False)] + [("tiny", k, False) for k in (1, 16, 64, 65, 100, 256, 1000, 1024)] + \
            [("plane", 256, False), ("two_sheets", 256, False), ("twice", 256, False), ("tiny[:256]", 256, False), ("tiny[:257]", 256, False),
             ("tiny", 64, True)]


def adjacency_id(case):
    return "%s-k%d%s" % (case[0], case[1], "-foreign" if case[2] else "")


def queries_of(case):
    """None for the cloud's own points"""
    return np.ascontiguousarray((cloud(case[0])[0].astype(np.int32) + 1).astype(np.int16)) if case[2] else None


# ---- rounds: (cloud, K, lambda, round counts), from the normals and the initial partition of the cloud
ROUNDS = [("lattice", 256, 3.0, (1, 2, 3, 100)), ("tiny", 256, 3.0, (1, 2, 3, 100)), ("tiny", 64, 3.0, (10,)), ("tiny", 1000, 3.0, (5,)),
          ("tiny", 256, 0.0, (2,)), ("tiny", 256, 30.0, (5,)), ("small", 256, 3.0, (100,))]


def rounds_id(case):
    return "%s-k%d-lambda%g" % case[:3]


# ---- chain: (cloud, voxelDimensionGridBasedSegmentation or 0, normalOrientation)
CHAIN = [(c, v, 1) for c in ("lattice", "tiny", "small") for v in (0, 2)] + [("tiny", 0, 0), ("medium", 0, 1)]
DIFFERS_FROM_GRID_REFINE = ("lattice", "tiny", "small", "medium")     # the generator insists: plain chain against the CTC's grid refinement
TIED_CUT = ("lattice", "tiny")                                        # ... and: >= 1000 rows whose 256th and 257th distances are equal


def chain_id(case):
    return "%s%s%s" % (case[0], "-vox%d" % case[1] if case[1] else "", "" if case[2] == 1 else "-orientation%d" % case[2])


def overrides(params, orientation=1, max_nn=K, iterations=ITERATIONS, lam=LAMBDA):
    """the flag off and the defaults the reference takes then, on a parameter struct of either binding"""
    params.gridBasedRefineSegmentation = 0
    params.maxNNCountRefineSegmentation = max_nn
    params.iterationCountRefineSegmentation = iterations
    params.lambdaRefineSegmentation = lam
    params.normalOrientation = orientation
    return params


def oracle_params(oracle, xyz, orientation=1):
    import oracle_binding as ob
    return overrides(ob.seg_params(ITERATIONS, BITS3D, oracle.weight_normal(xyz, BITS3D, 0.6)), orientation)


# ---- rows as sets
def sorted_rows(adj):
    return np.sort(np.ascontiguousarray(adj, np.uint32), axis=1)


def row_crcs(adj):
    """CRC32 of every sorted row, uint32 [n]"""
    rows = sorted_rows(adj)
    return np.array([zlib.crc32(r.tobytes()) for r in rows], np.uint32)


def first_bad_row(adj, want_crcs):
    """-1, or the first row whose set differs from the fixture's"""
    bad = np.nonzero(row_crcs(adj) != want_crcs)[0]
    return -1 if len(bad) == 0 else int(bad[0])


def kth_distances(xyz, queries, k_list):
    """squared distance of the k-th nearest point (k counted from 1) per query, int64 [len(k_list)][nq]; n + 1: beyond the cloud (-1)"""
    p, q = np.asarray(xyz).astype(np.int64), np.asarray(xyz if queries is None else queries).astype(np.int64)
    out = np.full((len(k_list), len(q)), -1, np.int64)
    for at in range(0, len(q), 512):
        d = ((q[at:at + 512, None, :] - p[None, :, :]) ** 2).sum(2)
        d.sort(axis=1)
        for j, k in enumerate(k_list):
            if k <= len(p):
                out[j, at:at + 512] = d[:, k - 1]
    return out


def brute_force_bound(xyz, queries, adj):
    """what every tie rule agrees on: K different points per row, everything closer than the K-th distance, nothing farther"""
    p, q = np.asarray(xyz).astype(np.int64), np.asarray(xyz if queries is None else queries).astype(np.int64)
    adj = np.asarray(adj).astype(np.int64)
    k = adj.shape[1]
    assert adj.shape[0] == len(q) and adj.min() >= 0 and adj.max() < len(p)
    rows = np.sort(adj, axis=1)
    assert (np.diff(rows, axis=1) > 0).all(), "a row names a point twice"
    kth = kth_distances(xyz, queries, (k,))[0]
    for at in range(0, len(q), 512):
        d = ((q[at:at + 512, None, :] - p[None, :, :]) ** 2).sum(2)
        mine = np.take_along_axis(d, adj[at:at + 512], 1)
        assert (mine <= kth[at:at + 512, None]).all(), "a row holds a point beyond its K-th distance"
        closer = (d < kth[at:at + 512, None]).sum(1)
        assert ((mine < kth[at:at + 512, None]).sum(1) == closer).all(), "a row misses a point closer than its K-th distance"


# ---- the chain without the reference
_start, _chain = {}, {}


def start(oracle, name, orientation=1, vox_dim=0):
    """(positions the front of the segmenter sees, normals, initial partition, rank of every point's voxel or None), shared and read-only"""
    key = (name, orientation, vox_dim)
    if key not in _start:
        xyz = cloud(name)[0]
        w = oracle.weight_normal(xyz, BITS3D, 0.6)
        pts, rank = (xyz, None) if vox_dim == 0 else gc.voxelize(xyz, vox_dim)
        nrm = oracle.normals(pts, 16, oriented=orientation == 1)
        part = oracle.initial_segmentation(nrm, w)
        for a in (pts, nrm, part):
            a.setflags(write=False)
        _start[key] = (pts, nrm, part, rank)
    return _start[key]


def host_chain(oracle, case):
    """dict(normals, partition, knn, seg, params) of the points, computed once per case and shared"""
    import tmc2_amd as T
    if case not in _chain:
        name, vox_dim, orientation = case
        xyz, rgb = cloud(name)
        sp = oracle_params(oracle, xyz, orientation)
        pts, nrm, part, rank = start(oracle, name, orientation, vox_dim)
        refined = T.host_refine_segmentation(pts, nrm, part, sp.maxNNCountRefineSegmentation, sp.lambdaRefineSegmentation, sp.iterationCountRefineSegmentation)
        if rank is not None:
            refined, nrm = refined[rank], nrm[rank]
        knn = oracle.knn_self(xyz, 16)
        partition = np.ascontiguousarray(refined, np.uint32)
        seg = oracle.segment_patches(xyz, rgb, knn, partition, sp)
        _chain[case] = dict(normals=np.ascontiguousarray(nrm), partition=partition, knn=knn, seg=seg, params=sp)
    return _chain[case]


def digests(partition, seg):
    """what the fixture keeps of a chain case"""
    d = pc.result_digests(seg)
    d["partition"] = pc.digest(np.ascontiguousarray(partition, np.uint32))
    return d


def input_digest(name):
    xyz, rgb = cloud(name)
    return pc.digest(xyz) + pc.digest(rgb)
