"""GPU tier (-m gpu): the metric over the switches PccAppMetrics takes (tmc2_metrics_compute_ex and its frame forms) against what the
UNMODIFIED reference made of the same clouds (tests/golden/metrics_options.npz) -- every double bit-equal, the runs the host form
declines included -- and against the host form on clouds no fixture covers."""
import ctypes as C

import numpy as np
import pytest

import metrics_option_cases as mc
import tmc2_amd as T
from tmc2_amd.synth import synth_cloud

pytestmark = pytest.mark.gpu

NON_DEFAULT = (T.MetricsParams(compute_hausdorff=True, neighbors_proc=4), T.MetricsParams(drop_duplicates=0, neighbors_proc=0, compute_hausdorff=True))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def golden():
    return np.load(mc.FIXTURE)


@pytest.mark.parametrize("name,set_name", mc.runs())
def test_gpu_metrics_options_match_reference(gpu_ctx, golden, name, set_name):
    src, sc, rec, rc, nrm = mc.case(name)
    assert mc.digest(src, sc, rec, rc, nrm) == str(golden[name + "__input_md5"]), "generated input differs from the fixture's"
    params = mc.PARAM_SETS[set_name]
    got, counts = gpu_ctx.metrics_compute(src, sc, rec, rc, mc.normals_for(name, params, nrm), params=params)
    k = mc.key(name, set_name)
    assert got.shape == (3, 14) and np.array_equal(counts, golden[k + "__counts"])
    assert np.array_equal(bits(got), bits(golden[k + "__q"])), (got, golden[k + "__q"])


def test_gpu_wide_groups_are_reached_on_duplicates(gpu_ctx):
    """dropDuplicates 0 on the cloud with a position that is there 40 times: the 32-wide search runs (the first 30 count)."""
    src, sc, rec, rc, nrm = mc.case("duplicates")
    gpu_ctx.stage_reset()
    gpu_ctx.metrics_compute(src, sc, rec, rc, nrm, params=mc.PARAM_SETS["dd0"])
    assert gpu_ctx.stage_ms().get("metrics_wide_search", 0) == 1.0


@pytest.mark.parametrize("name", ["ordinary", "duplicates"])
def test_gpu_default_params_are_the_old_entry(gpu_ctx, name):
    src, sc, rec, rc, nrm = mc.case(name)
    normals = mc.normals_for(name, T.MetricsParams(), nrm)
    old, oc = gpu_ctx.metrics_compute(src, sc, rec, rc, normals)
    new, nc = gpu_ctx.metrics_compute(src, sc, rec, rc, normals, params=T.MetricsParams())
    assert old.shape == (3, 8) and np.array_equal(oc, nc) and np.array_equal(bits(old), bits(new[:, :8]))


@pytest.mark.parametrize("set_name", ["hausdorff", "dd1", "np3", "np4", "no_c2p", "combined"])
def test_gpu_metrics_options_match_host_form(gpu_ctx, set_name):
    """A cloud no fixture holds (another seed, 4 500 points: five blocks of the ordered sums), against the host form."""
    rng = np.random.default_rng(5)
    xyz, rgb = mc._tiny(rng, 4500)
    rec = xyz.copy()
    move = rng.random(len(xyz)) < 0.5
    rec[move] += rng.integers(-2, 3, (int(move.sum()), 3)).astype(np.int16)
    col = rng.integers(0, 256, rgb.shape).astype(np.uint8)
    nrm = mc._unit(rng, len(xyz))
    params = mc.PARAM_SETS[set_name]
    got, gc = gpu_ctx.metrics_compute(xyz, rgb, rec[::-1], col, nrm, params=params)
    exp, ec = T.host_metrics_compute(xyz, rgb, rec[::-1], col, nrm, params=params)
    assert np.array_equal(gc, ec) and np.array_equal(bits(got), bits(exp)), (got, exp)


def test_gpu_frame_entries_match_the_host_array_entry(gpu_ctx):
    """tmc2_metrics_compute_frame_ex (which 0 and 1) and tmc2_metrics_compute_frame_source_ex on the tiny pipeline state = the
    host-array entry on the same clouds fetched to the host, for two non-default sets."""
    xyz, rgb = synth_cloud("tiny")
    fr = gpu_ctx.frame(xyz, rgb)
    w = fr.weight_normal(11, 0.6)
    fr.segmenter_compute(T.ctc_params(10, 11, w))
    h = fr.encoder_pack_flexible(1280, 2, 1.0)
    W, H = T.encoder_canvas_size([h], 1280, 1280, 1280)
    fr.encoder_generate_geometry_images(W, H, 4)
    fr.encoder_generate_attribute_images()
    rx, rc, _ = fr.get_reconstruction()
    nrm = fr.get_normals()
    for params in NON_DEFAULT:
        for use_normals in (False, True):
            got, gc = fr.metrics_compute(0, use_normals, params=params)
            exp, ec = gpu_ctx.metrics_compute(xyz, rgb, rx, rc, nrm if use_normals else None, params=params)
            assert got.shape == (3, 14) and np.array_equal(gc, ec) and np.array_equal(bits(got), bits(exp)), (got, exp)
    fr.codec_set_decoded_attribute_yuv420(fr.encoder_attribute_to_yuv420(4), 0)
    fr.codec_post_reconstruct(None)
    post = fr.get_post_reconstruction()
    for params in NON_DEFAULT:
        exp, ec = gpu_ctx.metrics_compute(xyz, rgb, post["xyz"], post["rgb"], nrm, params=params)
        got, gc = fr.metrics_compute(1, True, params=params)
        assert np.array_equal(gc, ec) and np.array_equal(bits(got), bits(exp)), (got, exp)
        got, gc = fr.metrics_compute_source(xyz, rgb, nrm, which=1, params=params)
        assert np.array_equal(gc, ec) and np.array_equal(bits(got), bits(exp)), (got, exp)
    assert (exp[:, 10] >= 1).all() and (exp[:2, 12] > 0).all()


def test_gpu_sequential_sums_give_the_same_bits(gpu_ctx, golden, ctx_options):
    ctx_options.setenv("TMC2_METRICS_SUMS", "sequential")
    src, sc, rec, rc, nrm = mc.case("ordinary")
    got, _ = gpu_ctx.metrics_compute(src, sc, rec, rc, nrm, params=mc.PARAM_SETS["combined"])
    assert np.array_equal(bits(got), bits(golden[mc.key("ordinary", "combined") + "__q"]))


def test_gpu_refusals_by_name_leave_no_state(gpu_ctx, golden):
    """Each refusal comes back by name (TMC2_E_UNSUPPORTED; TMC2_E_INVALID without params), and a default call after it returns
    the bits it returned before."""
    src, sc, rec, rc, nrm = mc.case("ordinary")
    L = gpu_ctx.L
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    before, _ = gpu_ctx.metrics_compute(src, sc, rec, rc, nrm, params=T.MetricsParams())
    assert np.array_equal(bits(before), bits(golden[mc.key("ordinary", "default") + "__q"]))
    fr = gpu_ctx.frame(src, sc)
    out, counts = np.full((3, 14), -1.0), np.zeros(2, np.int64)
    unsupported, invalid = -4, -3
    refusals = [(dict(drop_duplicates=3), "dropDuplicates = 3"), (dict(drop_duplicates=-1), "dropDuplicates = -1"),
                (dict(neighbors_proc=5), "neighborsProc = 5"), (dict(neighbors_proc=-1), "neighborsProc = -1"),
                (dict(compute_c2c=2), "computeC2c = 2"), (dict(compute_c2p=-1), "computeC2p = -1"), (dict(compute_color=7), "computeColor = 7"),
                (dict(compute_hausdorff=2), "computeHausdorff = 2"), (None, "params is NULL")]
    for bad, message in refusals:
        st = None if bad is None else C.byref(T.MetricsParams(**bad).struct())
        want = invalid if bad is None else unsupported
        gpu_ctx.stage_reset()
        assert L.tmc2_metrics_compute_ex(gpu_ctx.h, p(src), p(sc), len(src), p(rec), p(rc), len(rec), p(nrm), 1023.0, st, p(out), p(counts)) == want
        assert message in L.tmc2_last_error().decode(), (message, L.tmc2_last_error().decode())
        assert L.tmc2_metrics_compute_frame_ex(fr.h, 0, 0, 1023.0, st, p(out), p(counts)) == want
        assert L.tmc2_metrics_compute_frame_source_ex(fr.h, 1, p(src), p(sc), len(src), None, 1023.0, st, p(out), p(counts)) == want
        assert not any(gpu_ctx.stage_calls().values()), "a refused call ran a stage"
        assert (out == -1.0).all()
        after, _ = gpu_ctx.metrics_compute(src, sc, rec, rc, nrm, params=T.MetricsParams())
        assert np.array_equal(bits(after), bits(before)), bad
