"""Every stage chain at its smallest shapes on contexts whose pool hands out POISONED blocks (option POOL_POISON).

A block from the context's caching pool holds what its last owner left, or what the driver left: usually zeros, or plausible values
of the same stage on a similar cloud.  A kernel that reads a word before any kernel of its stage has written it -- a counter never
cleared, a bitmap tail past n, the w lane of a point, a row beyond count -- therefore passes every other test.  Here each stage runs
on a context of its own per poison byte, the option set right after creation:

    0x00   what fresh memory looks like
    0xFF   the library's "no slot / no block" sentinel as a uint32, -1 as an int16, a NaN as a double
    0x5A   a plausible coordinate (23130) as an int16, a large positive index as a uint32, a huge finite double

Every product must equal the oracle (the same helpers and case modules as the stages' own tests: integer or bit-pattern equality,
no tolerance) and be byte-identical across the three bytes (the last test).  The bytes run in the order above; the context of a
byte is shared by all tests of the module, so its free lists are as dirty as the earlier stages leave them.

The probe tests prove the option itself: tmc2_selftest_pool_probe reads a block it has not written -- the whole size class is the
poison byte, for fresh and for recycled blocks, and its output differs between two bytes (the control: this harness would see an
uninitialised read).

Not covered by this module: memory that does not come from the pool (tmc2_ctx_device_alloc, page-locked staging, a buffer allocated
with no context entered) and buffers that keep their own block from one call to the next (DevBuf::alloc's early return).

To localise a mismatch that does not fault: ctx.set_option("POOL_POISON_STAGE", <stage name of ctx.stage_calls()>)."""
import hashlib
import time

import numpy as np
import pytest

import color_smoothing_cases as cs
import decoder_frame_cases as dc
import grid_based_cases as gc
import knn_refine_cases as kc
import metrics_option_cases as mc
import oracle_binding as ob
import orientation_cases as oc
import patch_round_cases as prc
import test_gpu_canvases as t_canvases
import test_gpu_color_smoothing as t_smoothing
import test_gpu_decoder_frames as t_decoder
import test_gpu_grid_based_segmentation as t_grid
import test_gpu_images as t_images
import test_gpu_kdtree_level_loads as t_levels
import test_gpu_knn_batched_loads as t_knn
import test_gpu_knn_refine_segmentation as t_refine
import test_gpu_metrics_options as t_metrics
import test_gpu_orientation as t_orient
import test_gpu_patch_border_filtering as t_pbf
import test_gpu_patch_rounds as t_rounds
import tmc2_amd as T
from canvas_cases import BY_NAME as SCENES
from test_gpu_segmenter import _assert_patches_equal, bits
from tmc2_amd.synth import synth_cloud

pytestmark = pytest.mark.gpu

BYTES = (0x00, 0xFF, 0x5A)
by_byte = pytest.mark.parametrize("byte", BYTES, ids=["0x%02X" % b for b in BYTES])
PROBE_SIZES = (1, 255, 256, 257, 4096, (1 << 20) + 1)

_products = {}   # case -> {byte: {product: (shape, dtype, sha1)}}
_seconds = {}    # stage group -> {byte: wall seconds under poison, fill-and-wait included}


def size_class(nbytes):
    c = 256
    while c < nbytes:
        c <<= 1
    return c


def record(case, byte, **arrays):
    out = {}
    for k, a in arrays.items():
        a = np.asarray(a)
        for name, part in ([(k + "." + f, a[f]) for f in a.dtype.names] if a.dtype.names else [(k, a)]):   # (records: no padding bytes)
            out[name] = (part.shape, part.dtype.str, hashlib.sha1(np.ascontiguousarray(part).tobytes()).hexdigest())
    _products.setdefault(case, {})[byte] = out


def record_state(case, byte, fr):
    """partition, normals, adjacency, patch records and pools of a segmented frame"""
    patches, d0, d1, occ = fr.get_patches()
    record(case, byte, partition=fr.get_partition(), normals=fr.get_normals(), knn=fr.get_adjacency(16), patches=patches, depth0=d0, depth1=d1,
           occupancy=occ)


class _Timed:
    def __init__(self, group, byte):
        self.group, self.byte = group, byte

    def __enter__(self):
        self.t0 = time.perf_counter()

    def __exit__(self, *exc):
        per = _seconds.setdefault(self.group, {})
        per[self.byte] = per.get(self.byte, 0.0) + time.perf_counter() - self.t0


def _token(h, v):
    if isinstance(v, np.ndarray):
        h.update(("%s%s" % (v.shape, v.dtype.str)).encode())
        h.update(np.ascontiguousarray(v).tobytes())
    elif isinstance(v, dict):
        for k in sorted(v):
            h.update(str(k).encode())
            _token(h, v[k])
    elif isinstance(v, (list, tuple)):
        h.update(b"[%d" % len(v))
        for x in v:
            _token(h, x)
    else:
        h.update(repr(v).encode())


class _Memo:
    """The oracle with every answer computed once per input and shared among the three bytes (left unchanged by the tests)."""
    _answers = {}

    def __init__(self, oracle):
        self._oracle = oracle

    def __getattr__(self, name):
        fn = getattr(self._oracle, name)

        def call(*args, **kwargs):
            h = hashlib.sha1(name.encode())
            _token(h, args)
            _token(h, kwargs)
            key = h.hexdigest()
            if key not in _Memo._answers:
                _Memo._answers[key] = fn(*args, **kwargs)
            return _Memo._answers[key]
        return call


class _Recording:
    """A context that also keeps what its own entries returned (the stages' tests assert on them and drop them)."""

    def __init__(self, ctx):
        self._ctx, self.returned, self.frames = ctx, [], []

    def __getattr__(self, name):
        fn = getattr(self._ctx, name)
        if not callable(fn):
            return fn

        def call(*args, **kwargs):
            out = fn(*args, **kwargs)
            if name in ("frame", "decoder_frame"):
                self.frames.append(out)
            parts = out if isinstance(out, (tuple, list)) else (out,)
            self.returned += [(name, a) for a in parts if isinstance(a, np.ndarray)]
            return out
        return call

    def record(self, case, byte):
        assert self.returned, "nothing came back from the context"
        record(case, byte, **{"%s_%d" % (n, i): a for i, (n, a) in enumerate(self.returned)})


@pytest.fixture(scope="module")
def poisoned():
    """byte -> the context of that byte, made on first use with the option set right after creation; all closed at the end"""
    made = {}

    def get(byte):
        if byte not in made:
            made[byte] = T.Context(0)
            made[byte].set_option("POOL_POISON", "0x%02X" % byte)
            assert int(made[byte].get_option("POOL_POISON"), 16) == byte
        return made[byte]
    get.made = made
    yield get
    for ctx in made.values():
        ctx.close()


@pytest.fixture(scope="module")
def memo(oracle):
    return _Memo(oracle)


# ---- the option itself -------------------------------------------------------------------------------------------------------------
@by_byte
def test_gpu_probe_whole_class_is_the_byte(poisoned, byte):
    ctx = poisoned(byte)
    before = ctx.selftest_pool_poisoned()
    for size in PROBE_SIZES:
        got = ctx.selftest_pool_probe(size)
        assert len(got) == size_class(size)
        wrong = np.nonzero(got != byte)[0]
        assert len(wrong) == 0, "%d of %d bytes of a block of %d are not 0x%02X, first at %d: 0x%02X" % (len(wrong), len(got), size, byte, wrong[0], got[wrong[0]])
    assert ctx.selftest_pool_poisoned() == before + len(PROBE_SIZES)


@by_byte
def test_gpu_probe_recycled_blocks_are_filled(poisoned, byte):
    """a frame built, run and destroyed leaves the free lists dirty; the next probes are served from them (no allocation) and
    still read back as the byte"""
    ctx = poisoned(byte)
    xyz, rgb = synth_cloud("tiny")
    fr = ctx.frame(xyz, rgb)
    fr.normals_compute(16, 1)
    fr.close()
    for size in PROBE_SIZES:
        ctx.selftest_pool_probe(size)                      # (every class has a free block from here on)
    calls = ctx.pool_stats()["hipmalloc_calls"]
    for size in PROBE_SIZES + (len(xyz) * 16 * 4,):
        got = ctx.selftest_pool_probe(size)
        assert (got == byte).all(), "a recycled block of %d bytes is not filled" % size
    assert ctx.pool_stats()["hipmalloc_calls"] == calls, "the probes were not served from the free lists"


def test_gpu_probe_control_differs_between_bytes(poisoned):
    """the reader of unwritten memory gives another answer under another byte: an uninitialised read cannot hide from the last test"""
    for size in PROBE_SIZES:
        a, b = poisoned(0xFF).selftest_pool_probe(size), poisoned(0x5A).selftest_pool_probe(size)
        assert a.shape == b.shape and (a != b).all()


def test_gpu_probe_unset_option_fills_nothing():
    """set, then unset, on one context: acquire stops filling (by the pool's counter; the content is unspecified then); a value
    that is no byte is refused and leaves the option as it was; POOL_POISON_STAGE narrows the fill to a stage's blocks"""
    ctx = T.Context(0)
    try:
        assert ctx.get_option("POOL_POISON") is None and ctx.selftest_pool_poisoned() == 0
        ctx.selftest_pool_probe(4096)
        assert ctx.selftest_pool_poisoned() == 0
        ctx.set_option("TMC2_POOL_POISON", 90)                        # (the prefix is accepted; decimal)
        assert ctx.get_option("POOL_POISON") == "90"
        assert (ctx.selftest_pool_probe(4096) == 0x5A).all() and ctx.selftest_pool_poisoned() == 1
        for bad in ("256", "-1", "zz"):
            with pytest.raises(T.Tmc2Error, match="error -3.*POOL_POISON"):
                ctx.set_option("POOL_POISON", bad)
            assert ctx.get_option("POOL_POISON") == "90"
        ctx.set_option("POOL_POISON_STAGE", "kdtree_build")           # no stage open around a probe or a frame's upload: not filled
        ctx.selftest_pool_probe(4096)
        fr = ctx.frame(synth_cloud("tiny")[0])
        assert ctx.selftest_pool_poisoned() == 1
        fr.kdtree_order()                                             # (the device build allocates its arrays inside the stage's span)
        inside = ctx.selftest_pool_poisoned()
        assert inside > 1 and ctx.stage_calls().get("kdtree_build", 0) == 1
        fr.close()
        ctx.set_option("POOL_POISON_STAGE", None)
        ctx.set_option("POOL_POISON", None)
        assert ctx.get_option("POOL_POISON") is None
        ctx.selftest_pool_probe(4096)
        ctx.selftest_pool_probe((1 << 20) + 1)
        assert ctx.selftest_pool_poisoned() == inside
    finally:
        ctx.close()


# ---- tree and k-NN -----------------------------------------------------------------------------------------------------------------
@by_byte
@pytest.mark.parametrize("name", ["n4097", "n8193", "dup12000"])
def test_gpu_tree_level_passes(poisoned, memo, byte, name):
    ctx = poisoned(byte)
    with _Timed("tree", byte):
        ctx.set_option("KD_HUGEMAX", "4096")
        try:
            fr = ctx.frame(t_levels.cloud(name))
            t_levels.check_device_tree(fr, name, memo)
        finally:
            ctx.set_option("KD_HUGEMAX", None)
        perm, depth = fr.kdtree_order()
        record("tree/" + name, byte, perm=perm, depth=np.array(depth))
        fr.close()


@by_byte
@pytest.mark.parametrize("name", ["duplicates", "eleven"])
def test_gpu_tree_knn_every_width(poisoned, memo, byte, name):
    ctx = poisoned(byte)
    with _Timed("tree", byte):
        xyz = t_knn.cloud(name)
        q = t_knn.queries_for(xyz, memo.kdtree_perm(xyz)[0])
        fr, got = ctx.frame(xyz), {}
        for k in (k for k in (1, 8, 16) if k <= len(xyz)):
            idx, d = fr.kdtree_search(q, k, with_dist=True)
            oi, od = memo.knn(xyz, q, k, with_dist=True)
            assert np.array_equal(idx, oi) and np.array_equal(d.astype(np.float64), od), (name, k)
            got["idx%d" % k], got["dist%d" % k] = idx, d
        record("knn/" + name, byte, **got)
        fr.close()


@by_byte
def test_gpu_tree_wide_search(poisoned, byte):
    """257 neighbours: one more than four passes of 64 lanes.  The oracle's search ends at k = 64; the rows are the host entry's, as
    test_gpu_knn_refine_segmentation.py compares the wide search above 64."""
    ctx = poisoned(byte)
    xyz = kc.cloud("tiny")[0]
    if "wide" not in _Memo._answers:
        _Memo._answers["wide"] = kc.sorted_rows(T.host_refine_segmentation(xyz, np.zeros((len(xyz), 3)), np.zeros(len(xyz), np.uint32), 257, 0.0, 0,
                                                                           with_adjacency=True)[1])
    with _Timed("tree", byte):
        fr = ctx.frame(xyz)
        rows = fr.kdtree_search_wide(257)
        assert rows.shape == (len(xyz), 257) and np.array_equal(kc.sorted_rows(rows), _Memo._answers["wide"])
        record("knn_wide/tiny257", byte, rows=kc.sorted_rows(rows))
        fr.close()


# ---- normals, orientation, weights, initial segmentation ---------------------------------------------------------------------------
@by_byte
@pytest.mark.parametrize("k", [16, 8])
def test_gpu_normals_weights_initial_segmentation(poisoned, memo, byte, k):
    ctx = poisoned(byte)
    with _Timed("normals", byte):
        xyz, rgb = synth_cloud("tiny")
        fr = ctx.frame(xyz, rgb)
        fr.normals_compute(k, 1)
        o_n = memo.normals(xyz, k, True)
        nrm = fr.get_normals()
        assert np.array_equal(bits(nrm), bits(o_n)), "normals (k = %d) differ from the oracle" % k
        w = fr.weight_normal(11, 0.6)
        assert np.array_equal(bits(w), bits(memo.weight_normal(xyz, 11, 0.6)))
        fr.segmenter_initial_segmentation(w)
        part = fr.get_partition()
        assert np.array_equal(part, memo.initial_segmentation(o_n, w))
        if k == 16:
            assert np.array_equal(fr.get_adjacency(16), memo.knn_self(xyz, 16))
        record("normals/tiny-k%d" % k, byte, normals=nrm, weight=w, partition=part)
        fr.close()


# a majority flip (20 of 37 look away), signed zeros (an all-zero field), the smallest contracted one (17 points)
@by_byte
@pytest.mark.parametrize("name", ["majority_m20_n37", "zeros", "sizes_17"])
def test_gpu_normals_orientation_case(poisoned, oracle, byte, name):
    ctx = poisoned(byte)
    c = oc.all_cases(oracle)[name]
    with _Timed("normals", byte):
        got = t_orient.orient(ctx, c, "%s under 0x%02X" % (name, byte))           # (asserts the bits against the oracle)
        t_orient.assert_path(got, c.path())
    record("orientation/" + name, byte, counters=np.array([got[k] for k in t_orient.COUNTERS]))


# ---- the three segmenter chains on tiny ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def chain_yardsticks(oracle):
    xyz, rgb = kc.cloud("tiny")
    w = oracle.weight_normal(xyz, kc.BITS3D, 0.6)
    _, nrm, initial, _ = kc.start(oracle, "tiny")
    plain = dict(partition=oracle.refine_grid(xyz, nrm, initial, iterations=3), seg=oracle.segment(xyz, rgb, ob.seg_params(3, kc.BITS3D, w)))
    return w, {"plain": plain, "grid_based-vox2": gc.yardstick(oracle, ("tiny", 2, 1)), "knn_refine": kc.host_chain(oracle, ("tiny", 0, 1))}


@by_byte
@pytest.mark.parametrize("chain", ["plain", "grid_based-vox2", "knn_refine"])
def test_gpu_chain_on_tiny(poisoned, chain_yardsticks, byte, chain):
    """segmenter_compute, segmenter_compute_grid_based and segmenter_compute_knn_refine as test_gpu_segmenter.py's chain test,
    test_gpu_grid_based_segmentation.py and test_gpu_knn_refine_segmentation.py compare them"""
    ctx = poisoned(byte)
    w, yardsticks = chain_yardsticks
    y = yardsticks[chain]
    xyz, rgb = kc.cloud("tiny")
    with _Timed("chains", byte):
        fr = ctx.frame(xyz, rgb)
        assert np.array_equal(bits(fr.weight_normal(kc.BITS3D, 0.6)), bits(w))
        if chain == "plain":
            fr.segmenter_compute(T.ctc_params(3, kc.BITS3D, w))
            assert np.array_equal(fr.get_partition(), y["partition"])
            _assert_patches_equal(fr.get_patches(), y["seg"])
        elif chain == "grid_based-vox2":
            fr.segmenter_compute(T.fast_params(bits3d=kc.BITS3D, weight=w), grid_based=2)
            t_grid.assert_is_yardstick(t_grid.state(fr), y)
        else:
            fr.segmenter_compute(kc.overrides(T.knn_refine_params(kc.ITERATIONS, kc.BITS3D, w)))
            t_refine.assert_is_chain(t_refine.state(fr), y)
        record_state("chain/" + chain, byte, fr)
        fr.close()


@by_byte
@pytest.mark.parametrize("vox_dim", [2, 4])
def test_gpu_chain_convert_points_to_voxels(poisoned, byte, vox_dim):
    ctx = poisoned(byte)
    xyz = kc.cloud("tiny")[0]
    with _Timed("chains", byte):
        vox, rank = ctx.convert_points_to_voxels(xyz, vox_dim, gc.BITS3D)
        host_vox, host_rank = T.host_convert_points_to_voxels(xyz, vox_dim, gc.BITS3D)
        want_vox, want_rank = gc.voxelize(xyz, vox_dim)
        assert np.array_equal(host_vox, want_vox) and np.array_equal(host_rank, want_rank)
        assert np.array_equal(vox, host_vox), "voxel list (positions or order)"
        assert np.array_equal(rank, host_rank), "rank of the points' voxels"
    record("voxels/tiny-vox%d" % vox_dim, byte, voxels=vox, rank=rank)


# ---- patch rounds --------------------------------------------------------------------------------------------------------------------
@by_byte
def test_gpu_rounds_slab_with_clumps(poisoned, memo, byte):
    """three sheets, a clump that becomes a patch between two that stay raw: rounds two and three run from the compacted list"""
    ctx = _Recording(poisoned(byte))
    xyz, rgb, part = prc.slab_with_clumps(0, [15, 16, 3])
    with _Timed("rounds", byte):
        exp, calls = t_rounds._segment_patches(ctx, memo, xyz, rgb, part)
        assert exp["round_raw"].tolist() == [prc.SIDE ** 2 + 18, 18] and len(exp["patches"]) == 4
        assert calls.get("patches_build", 0) == 2 and calls.get("patches_cc", 0) == 3
        patches, d0, d1, occ = ctx.frames[0].get_patches()
    record("rounds/slab-15+16+3", byte, patches=patches, depth0=d0, depth1=d1, occupancy=occ)
    ctx.frames[0].close()


# ---- canvases: the third scene after the second on the same context -- a smaller pyramid is allocated after a larger one ---------------
@by_byte
@pytest.mark.parametrize("scene", ["origin_empty_64x64", "every_mask_256x128_p4", "above_small_384x320"])
def test_gpu_canvases_scene(poisoned, byte, scene):
    ctx = poisoned(byte)
    t_canvases.answer(SCENES[scene])                                        # (the oracle's answer: once, outside the timed span)
    with _Timed("canvases", byte):
        got = t_canvases.run_scene(ctx, SCENES[scene])
    record("canvases/" + scene, byte, **got)


# ---- decoder side and tail -------------------------------------------------------------------------------------------------------------
@by_byte
@pytest.mark.parametrize("name", ["single-small", "single"])       # the smallest frame (5 points), and one patch of 1 544
def test_gpu_decoder_frame_through_the_tail(poisoned, memo, byte, name):
    """point-cloud generation, boundary identification, colouring, geometry smoothing, 16-bit colour transfer, conversion, then the
    colour smoothing on top (against the host twin: the oracle's tail has no colour smoothing)"""
    ctx = poisoned(byte)
    pair, thr = dc.PAIRS[0], (1.0, 10.0, 6.0)
    s, r = dc.scene(name), dc.scene_references(name)
    assert r["xyz"].max() < 1024
    att = t_decoder._attribute(name, "random")
    want = t_decoder._tail(memo, name, pair)
    with _Timed("decoder", byte):
        fr = t_decoder._frame(ctx, s)
        assert np.array_equal(fr.get_geometry_images()["block_to_patch"], r["block_to_patch"])
        fr.codec_generate_point_cloud()
        xyz, _, p2p = fr.get_reconstruction(colors=False)
        assert np.array_equal(xyz, r["xyz"]) and np.array_equal(p2p, r["point_to_pixel"])
        fr.codec_identify_boundary_points()
        assert np.array_equal(fr.get_post_reconstruction(colors16=False, rgb=False)["boundary"], r["boundary"])
        fr.codec_color_point_cloud(att)
        assert np.array_equal(fr.get_post_reconstruction(rgb=False)["colors16"], memo.color_point_cloud(r["point_to_pixel"], att))
        fr.codec_smooth_point_cloud_postprocess(*pair)
        fr.codec_transfer_colors_16bit_bp()
        fr.codec_convert_yuv16_to_rgb8()
        t_decoder._assert_post(fr, want, (pair, "stages"))
        post = fr.get_post_reconstruction()
        fr.set_geometry_bit_depth_3d(10)
        fr.codec_color_smoothing(4, *thr)
        smoothed = fr.get_post_reconstruction(rgb=False)
        host = T.host_color_smoothing(post["xyz"], post["colors16"], post["boundary"], t_smoothing.patch_of_points(fr), 4, 10, *thr)
        assert np.array_equal(smoothed["colors16"], host)
        assert np.array_equal(smoothed["xyz"], post["xyz"]) and np.array_equal(smoothed["boundary"], post["boundary"])
    record("decoder/" + name, byte, recon=xyz, p2p=p2p, smoothed=smoothed["colors16"], **post)
    fr.close()


@by_byte
def test_gpu_decoder_patch_border_filtering(poisoned, byte):
    ctx = poisoned(byte)
    name = "plane_m0_o0"                                                   # a tilted, noisy plane of 48 x 48 pixels
    with _Timed("decoder", byte):
        occ = t_pbf.check_case_against_fixture(ctx, np.load(t_pbf.pc.FIXTURE), "hand_" + name, t_pbf.HAND[name])
    record("pbf/" + name, byte, occupancy=occ)


@by_byte
def test_gpu_decoder_color_smoothing_case(poisoned, byte):
    ctx = poisoned(byte)
    golden = np.load(cs.FIXTURE)
    xyz, c16, bt, part, grid, nbits, thr = cs.random_case(0)
    assert cs.input_digest(xyz, c16, bt, part) == str(golden["arb_rand0_input_md5"])
    with _Timed("decoder", byte):
        got = ctx.color_smoothing(xyz, c16, bt, part, grid, nbits, *thr)
    assert np.array_equal(got, t_smoothing.expected(c16, golden, "arb_rand0"))
    record("color_smoothing/rand0", byte, colors16=got)


# ---- colour ----------------------------------------------------------------------------------------------------------------------------
@by_byte
@pytest.mark.parametrize("name", ["tiny:3:0:33", "small:0:0:1001"])
def test_gpu_colour_transfer_identical_points_and_duplicates(poisoned, memo, byte, name):
    """targets that are source points, duplicate source positions with different colours, targets off the cloud: the split-path
    clouds of test_gpu_knn_batched_loads.py (the input of the same name in test_gpu_images.py takes 22 s on any context)"""
    ctx = _Recording(poisoned(byte))
    xyz = t_knn.cloud(name)
    with _Timed("colour", byte):
        t_knn.test_gpu_split_path(ctx, memo, {name: (xyz, memo.kdtree_perm(xyz)[0], None)}, name)
    ctx.record("colour/transfer-" + name, byte)


@by_byte
def test_gpu_colour_conversion_66x70(poisoned, memo, byte):
    """RGB444 -> YUV420 and YUV420 -> YUV444 with the filters the library builds (the reference's defaults; it refuses any other)"""
    ctx = _Recording(poisoned(byte))
    with _Timed("colour", byte):
        t_images.test_gpu_color_conversion_matches_oracle(ctx, memo, "noise", 66, 70)
    ctx.record("colour/conversion-66x70", byte)


# ---- metrics ---------------------------------------------------------------------------------------------------------------------------
@by_byte
@pytest.mark.parametrize("set_name", ["default", "dd0", "hausdorff", "combined"])
def test_gpu_metrics_ordinary(poisoned, byte, set_name):
    ctx = _Recording(poisoned(byte))
    with _Timed("metrics", byte):
        t_metrics.test_gpu_metrics_options_match_reference(ctx, np.load(mc.FIXTURE), "ordinary", set_name)
    ctx.record("metrics/ordinary-" + set_name, byte)


# ---- one GOF ---------------------------------------------------------------------------------------------------------------------------
@by_byte
def test_gpu_gof_two_tiny_frames_two_workers(memo, byte):
    frames = [synth_cloud("tiny", f) for f in range(2)]
    exp_a = memo.phase_a(frames, 10, 11, 4)
    exp_b = memo.phase_b(frames, exp_a, 4)
    with _Timed("gof", byte):
        enc = T.GofEncoder(0, workers=2, iterations=10)
        try:
            enc.set_option("POOL_POISON", "0x%02X" % byte)              # every worker context
            frs = enc.upload(frames)
            W, H = enc.phase_a(frs)
            enc.phase_b(frs)
            for i, (fr, ea, eb) in enumerate(zip(frs, exp_a, exp_b)):
                img = fr.get_geometry_images()
                assert (W, H) == (ea["width"], ea["height"])
                for k in t_canvases.GEOMETRY:
                    assert np.array_equal(img[k], ea[k]), (i, k)
                att = fr.get_attribute_images()
                assert np.array_equal(att, eb["attribute"]), i
                record("gof/frame%d" % i, byte, attribute=att, **{k: img[k] for k in t_canvases.GEOMETRY})
            assert all(c.selftest_pool_poisoned() > 0 for c in enc.ctxs)
            for fr in frs:
                fr.close()
        finally:
            enc.close(join=True)


# ---- across the bytes --------------------------------------------------------------------------------------------------------------------
def test_gpu_products_identical_across_bytes(poisoned):
    """every product recorded above, byte for byte the same under the three poison bytes (the tests above must have run), on
    contexts that still carry the option and have filled blocks"""
    for group, per in sorted(_seconds.items()):
        print("POOL_POISON %-9s %s" % (group, "  ".join("0x%02X: %6.2f s" % (b, per[b]) for b in BYTES if b in per)))
    assert _products, "no product was recorded: this test closes the module and does not run on its own"
    for case, per in sorted(_products.items()):
        assert sorted(per) == sorted(BYTES), "%s ran under %s only" % (case, ["0x%02X" % b for b in sorted(per)])
        for b in BYTES[1:]:
            assert sorted(per[b]) == sorted(per[BYTES[0]]), case
            differ = [k for k in per[b] if per[b][k] != per[BYTES[0]][k]]
            assert not differ, "%s: %s under 0x%02X differ from those under 0x%02X" % (case, differ, b, BYTES[0])
    for b, ctx in poisoned.made.items():
        assert int(ctx.get_option("POOL_POISON"), 16) == b and ctx.selftest_pool_poisoned() > 0
