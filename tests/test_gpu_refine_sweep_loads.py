"""GPU tier: the refine sweeps (closureKernel + sweepKernel, csrc/refine.hip) after their loads were batched -- a hop reads its
record and the whole padded DEV row at once, then edge / ppi of every entry, then issues every atomicOr before it looks at an
answer, and carries the work-list append into the next hop; the sweep kernel reads everything indexed by a voxel in one batch.
Every case compares segmenter_refine_grid_based with the oracle's in-order restatement, bit for bit, at the smallest shapes at
which that change can go wrong.  A slip in the closure's ring / pending protocol shows as a hang, not as a wrong bit: run this
file under a time limit."""
import numpy as np
import pytest

import tmc2_amd as T
from tmc2_amd.synth import synth_cloud

pytestmark = pytest.mark.gpu

_CASES = {}


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def _solid_block(side):
    """the block of test_gpu_refine_solid_cloud_takes_the_larger_tier: every position of a cube, random normals"""
    g = np.arange(side, dtype=np.int16)
    xyz = np.ascontiguousarray(np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3) + np.int16(200))
    rng = np.random.default_rng(5)
    nrm = rng.normal(size=(len(xyz), 3))
    nrm /= np.linalg.norm(nrm, axis=1)[:, None]
    return xyz, nrm


def _voxel_line(count, vox_dim):
    """`count` voxels side by side on a line, the eight positions of a 2 x 2 x 2 corner of each, random normals"""
    half = vox_dim // 2
    i = np.arange(count)
    corner = np.stack([vox_dim * (4 + i) - half, np.full(count, vox_dim * 9 - half), np.full(count, vox_dim * 7 - half)], 1)
    offs = np.stack(np.meshgrid([0, 1], [0, 1], [0, 1], indexing="ij"), -1).reshape(-1, 3)
    xyz = np.ascontiguousarray((corner[:, None, :] + offs[None, :, :]).reshape(-1, 3).astype(np.int16))
    rng = np.random.default_rng(100 + count)
    nrm = rng.normal(size=(len(xyz), 3))
    nrm /= np.linalg.norm(nrm, axis=1)[:, None]
    return xyz, nrm


def _sparse_block(cells, vox_dim, at):
    """cells^3 voxels of ONE point each: full neighbourhoods of few points (a row is cut where its members reach maxNN)"""
    g = np.arange(cells, dtype=np.int64) * vox_dim + at
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3).astype(np.int16)


def _voxels(xyz, vox_dim):
    """voxel keys (sorted, unique) and their member counts, as the reference voxelises: ( p + half ) >> log2( vox_dim )"""
    shift = vox_dim.bit_length() - 1
    c = (xyz.astype(np.int64) + vox_dim // 2) >> shift
    c += 8                                                   # (room for the offsets below: no key borrows from its neighbour)
    return np.unique(c[:, 0] | (c[:, 1] << 12) | (c[:, 2] << 24), return_counts=True)


def _dev_row_lengths(xyz, vox_dim):
    """Length of every voxel's DEV row (the occupied voxels within Chebyshev distance R = 2 for voxels of 2, 1 otherwise, itself
    included) and whether that is certain: the DEV row is taken from the neighbourhood row, which is cut where its members reach
    maxNN = 1024 in order of distance -- with fewer members than that within the largest squared distance of the cube, 3 R^2,
    the cut falls behind the cube."""
    keys, counts = _voxels(xyz, vox_dim)
    R = 2 if vox_dim < 4 else 1
    length = np.zeros(len(keys), np.int64)
    members = np.zeros(len(keys), np.int64)
    reach = int(np.floor(np.sqrt(3 * R * R)))
    for dx in range(-reach, reach + 1):
        for dy in range(-reach, reach + 1):
            for dz in range(-reach, reach + 1):
                if dx * dx + dy * dy + dz * dz > 3 * R * R:
                    continue
                other = keys + dx + (dy << 12) + (dz << 24)
                at = np.searchsorted(keys, other)
                at[at == len(keys)] = 0
                hit = keys[at] == other
                members += np.where(hit, counts[at], 0)
                if max(abs(dx), abs(dy), abs(dz)) <= R:
                    length += hit
    return length, members < 1024


def _cloud(name, vox_dim):
    if name in ("tiny", "small"):
        xyz = synth_cloud(name)[0]
        return xyz, None
    if name == "chunk-classes":      # a surface (short rows) and, away from it, a block of one-point voxels (full rows inside)
        return np.ascontiguousarray(np.concatenate([synth_cloud("tiny")[0], _sparse_block(6, vox_dim, 40)])), None
    if name == "isolated":           # voxels with nobody near them (a DEV row of the voxel alone, pad entries behind it)
        lone = np.array([[30 + 40 * k, 30 + 24 * (k % 3), 900 - 56 * k] for k in range(7)], np.int16)
        return np.ascontiguousarray(np.concatenate([lone[:3], synth_cloud("tiny")[0], lone[3:]])), None
    if name.startswith("line"):
        return _voxel_line(int(name[4:]), vox_dim)
    if name.startswith("solid"):
        return _solid_block(int(name[5:]))
    raise KeyError(name)


def _case(oracle, name, vox_dim, iters):
    """(xyz, normals, initial partition, the oracle's refined partition): computed once, shared, read-only"""
    key = (name, vox_dim, iters)
    if key not in _CASES:
        base = ("cloud", name, vox_dim)
        if base not in _CASES:
            xyz, nrm = _cloud(name, vox_dim)
            if nrm is None:
                nrm = oracle.normals(xyz)
                p0 = oracle.initial_segmentation(nrm, oracle.weight_normal(xyz))
            else:
                p0 = oracle.initial_segmentation(nrm, np.ones(3))
            _CASES[base] = _frozen(xyz, nrm, p0)
        xyz, nrm, p0 = _CASES[base]
        exp, = _frozen(oracle.refine_grid(xyz, nrm, p0, iterations=iters, vox_dim=vox_dim))
        _CASES[key] = (xyz, nrm, p0, exp)
    return _CASES[key]


def _refined(ctx, xyz, nrm, p0, iters, vox_dim):
    fr = ctx.frame(xyz)
    fr.set_normals(nrm)
    fr.set_partition(p0)
    fr.segmenter_refine_grid_based(1024, 3.0, iters, vox_dim, 192)
    out = fr.get_partition()
    fr.close()
    return out


@pytest.mark.parametrize("vox_dim", [4, 2])
@pytest.mark.parametrize("name", ["tiny", "small"])
def test_gpu_sweeps_both_strides(gpu_ctx, oracle, name, vox_dim):
    """DEV rows of 32 entries (voxels of 4: one chunk a hop) and of 128 (voxels of 2: four chunks a hop, all read whatever the
    row's length)."""
    xyz, nrm, p0, exp = _case(oracle, name, vox_dim, 10)
    assert not np.array_equal(exp, p0)
    assert np.array_equal(_refined(gpu_ctx, xyz, nrm, p0, 10, vox_dim), exp)


def test_gpu_sweeps_rows_of_every_chunk_count(gpu_ctx, oracle):
    """Voxels of 2: rows that end in the first, second, third and fourth chunk of 32 -- a surface has the short ones, the inside
    of a block of voxels the full ones (one point a voxel, so that the cut at maxNN members stays behind the cube)."""
    xyz, nrm, p0, exp = _case(oracle, "chunk-classes", 2, 6)
    length, certain = _dev_row_lengths(xyz, 2)
    classes = (length[certain] - 1) // 32
    assert length.min() >= 1 and length.max() <= 125
    assert [int((classes == k).sum()) > 0 for k in range(4)] == [True] * 4, np.bincount(classes, minlength=4)
    assert np.array_equal(_refined(gpu_ctx, xyz, nrm, p0, 6, 2), exp)


@pytest.mark.parametrize("vox_dim", [4, 2])
def test_gpu_sweeps_isolated_voxels(gpu_ctx, oracle, vox_dim):
    """Voxels far from every other one, first and last in the cloud and mixed with a surface: their DEV row holds the voxel itself
    and pad entries (a row is never shorter: the voxel lies in its own ball) -- the pad entries of the row read, unconditionally,
    edge / ppi of the hopping voxel."""
    xyz, nrm, p0, exp = _case(oracle, "isolated", vox_dim, 6)
    length, certain = _dev_row_lengths(xyz, vox_dim)
    assert int((length[certain] == 1).sum()) >= 7
    assert np.array_equal(_refined(gpu_ctx, xyz, nrm, p0, 6, vox_dim), exp)


@pytest.mark.parametrize("vox_dim", [4, 2])
@pytest.mark.parametrize("count", [1, 2, 15, 17, 33])
def test_gpu_sweeps_few_voxels(gpu_ctx, oracle, count, vox_dim):
    """V = 1, 2, 15, 17, 33: the last voxel's pointStart[v + 1], the last (partly used) state word of 16 voxels, and 16-lane / 32-lane
    groups that find nothing to do."""
    xyz, nrm, p0, exp = _case(oracle, "line%d" % count, vox_dim, 5)
    assert len(_voxels(xyz, vox_dim)[0]) == count
    assert np.array_equal(_refined(gpu_ctx, xyz, nrm, p0, 5, vox_dim), exp)


@pytest.mark.parametrize("blocks,ring", [("1", None), ("3", "1")])
@pytest.mark.parametrize("vox_dim", [4, 2])
@pytest.mark.parametrize("name", ["small", "solid40"])
def test_gpu_sweeps_carried_list_append(oracle, name, vox_dim, blocks, ring):
    """What a hop is the first to mark is appended to the work list by the group's NEXT hop, or before the group goes back to
    the ring or retires.  One workgroup (long runs, long chains), and three with a ring of one slot beyond the run (nearly every
    fan-out spills; groups retire and come back): every voxel listed and processed exactly once, or the partition differs.  A
    solid block is where one seed's activations cascade."""
    xyz, nrm, p0, exp = _case(oracle, name, vox_dim, 3)
    ctx = T.Context(0)                                     # (its own: a solid block raises the context's neighbourhood tier)
    ctx.set_option("REFINE_CLOSURE_BLOCKS", blocks)
    if ring:
        ctx.set_option("REFINE_RING", ring)
    got = _refined(ctx, xyz, nrm, p0, 3, vox_dim)
    ctx.close()
    assert np.array_equal(got, exp)


@pytest.mark.parametrize("vox_dim", [4, 2])
def test_gpu_sweeps_push_as_three_words(gpu_ctx, oracle, ctx_options, vox_dim):
    ctx_options.setenv("TMC2_REFINE_PUSH", "words")
    xyz, nrm, p0, exp = _case(oracle, "small", vox_dim, 10)
    assert np.array_equal(_refined(gpu_ctx, xyz, nrm, p0, 10, vox_dim), exp)


@pytest.mark.parametrize("vox_dim", [4, 2])
@pytest.mark.parametrize("iters", [1, 2, 7])
def test_gpu_sweeps_iteration_counts(gpu_ctx, oracle, iters, vox_dim):
    """state, counters and records are double-buffered by sweep parity: a last sweep of either parity, and a single one."""
    xyz, nrm, p0, exp = _case(oracle, "tiny", vox_dim, iters)
    assert np.array_equal(_refined(gpu_ctx, xyz, nrm, p0, iters, vox_dim), exp)


@pytest.mark.parametrize("vox_dim", [4, 2])
def test_gpu_sweeps_same_frame_twice(gpu_ctx, oracle, vox_dim):
    xyz, nrm, p0, exp = _case(oracle, "small", vox_dim, 10)
    for attempt in range(2):
        assert np.array_equal(_refined(gpu_ctx, xyz, nrm, p0, 10, vox_dim), exp), attempt
