"""The k-d tree level passes fetch what a position needs in batches: 16-byte loads of eight segment ids, of record rows and of
point pairs, clamped where a position lies at or beyond n.  These clouds sit where such loads can go wrong -- a last group cut
by n, a segment that ends exactly at n, retired and live positions inside one thread's group of 8, segment boundaries that
are no multiple of 8, pool memory left over from a larger tree.  Every case compares the device build with the host builder
(and, as test_gpu_kdtree_order_matches_reference_build does, with the oracle); the unmarked test pins the host builder to the
oracle on the same inputs, so a GPU failure can only be the device's.

The level passes only run for segments above KD_HUGEMAX, so most cases set it to its minimum (4096): a few thousand points
then take one or more level passes."""
import functools

import numpy as np
import pytest

import tmc2_amd as T

# name -> (KD_HUGEMAX or None for the default, KD_DECIDE or None)
CASES = {
    "n4097": ("4096", None),          # one level pass; the last tile holds one position, the last group of 8 is cut by n
    "n6143": ("4096", None),          # one short of a tile multiple
    "n8192": ("4096", None),          # a tile multiple: the root ends at n, lvPrefix2 takes sums[tiles]
    "n8193": ("4096", None),          # one over
    "line5000": ("4096", None),       # one axis, 40 values: long equal runs, a large second sweep, lim1 / lim2 balance
    "dup12000": ("4096", None),       # 40 points x 300: everything equals the cut, count / 2, swapping lanes next to idle ones
    "dense20000": ("4096", None),     # coordinates 0..11: tiny children next to large ones, retired next to live positions
    "n40000": ("4096", None),         # four or five levels, arbitrary boundaries
    "n40000:global": ("4096", "global"),  # ... and the decide pass's other range path
    "n70000": (None, None),           # level passes, then hugeSegmentsKernel, then pieces
    "n30000:huge": ("131072", None),  # the whole tree is one huge segment
}


@functools.lru_cache(maxsize=None)
def cloud(name):
    name = name.split(":")[0]
    rng = np.random.default_rng(23)
    if name == "line5000":
        xyz = np.zeros((5000, 3), np.int16)
        xyz[:, 1] = rng.integers(0, 40, 5000)
    elif name == "dup12000":
        xyz = np.repeat(rng.integers(0, 1024, (40, 3)).astype(np.int16), 300, axis=0)
    elif name == "dense20000":
        xyz = rng.integers(0, 12, (20000, 3)).astype(np.int16)
    else:
        xyz = rng.integers(0, 1024, (int(name[1:]), 3)).astype(np.int16)
    xyz.setflags(write=False)
    return xyz


@functools.lru_cache(maxsize=None)
def host_build(name):
    perm, _, depth = T.host_kdtree_build(cloud(name))
    perm.setflags(write=False)
    return perm, depth


def check_device_tree(fr, name, oracle):
    xyz = cloud(name)
    perm, depth = fr.kdtree_order()
    hperm, hdepth = host_build(name)
    assert np.array_equal(perm, hperm) and depth == hdepth
    assert np.array_equal(perm, oracle.kdtree_perm(xyz)[0])
    q = xyz[np.random.default_rng(5).integers(0, len(xyz), 2000)]
    assert np.array_equal(fr.kdtree_search(q, 16), oracle.knn(xyz, q, 16))


@pytest.mark.parametrize("name", sorted(set(c.split(":")[0] for c in CASES)))
def test_host_builder_equals_oracle(oracle, name):
    perm, _ = host_build(name)
    assert np.array_equal(perm, oracle.kdtree_perm(cloud(name))[0])


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_gpu_level_pass_loads(gpu_ctx, oracle, ctx_options, name):
    hugemax, decide = CASES[name]
    if hugemax:
        ctx_options.setenv("KD_HUGEMAX", hugemax)
    if decide:
        ctx_options.setenv("KD_DECIDE", decide)
    check_device_tree(gpu_ctx.frame(cloud(name)), name, oracle)


@pytest.mark.gpu
def test_gpu_level_pass_loads_over_stale_pool(gpu_ctx, oracle, ctx_options):
    """A large tree, then two small ones on the same context: the small trees' arrays are cut from pool blocks that still hold
    the large tree's segment ids, prefix sums and records past their own n."""
    ctx_options.setenv("KD_HUGEMAX", "4096")
    frames = []
    for name in ("n40000", "n4097", "n8193"):
        fr = gpu_ctx.frame(cloud(name))
        fr.kdtree_order()
        frames.append((fr, name))
    for fr, name in frames:
        check_device_tree(fr, name, oracle)
