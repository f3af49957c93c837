"""GPU tier of the colour smoothing (T6 of the post-reconstruction tail, csrc/color_smoothing.hip) against what the UNMODIFIED
reference's PCCCodec::colorSmoothing made of the same states (tests/golden/color_smoothing.npz) and against the host
restatement (tmc2_host_color_smoothing) on states no fixture covers.  Bit equality throughout."""
import os

import numpy as np
import pytest

import color_smoothing_cases as cs
import tmc2_amd as T
from tmc2_amd.configs import FULL_SIZE_CASES, constrained_pack
from tmc2_amd.synth import synth_cloud, synth_decoded_attribute

pytestmark = pytest.mark.gpu
GOLD = os.path.dirname(cs.FIXTURE)


@pytest.fixture(scope="module")
def golden():
    return np.load(cs.FIXTURE)


def expected(before, g, key):
    out = before.copy()
    out[g[key + "_idx"]] = g[key + "_colors16"]
    return out


def patch_of_points(fr):
    """the patch of every reconstructed point as the tail takes it: blockToPatch through pointToPixel"""
    b2p = fr.get_geometry_images()["block_to_patch"]
    _, _, p2p = fr.get_reconstruction(colors=False)
    return (b2p[p2p[:, 1] // 16, p2p[:, 0] // 16] - 1).astype(np.uint32)


def test_gpu_color_smoothing_tiny_gof_matches_reference(golden):
    """The 2-frame tiny GOF through GofEncoder.phase_c( color_smoothing = ... ): 16-bit colours, RGB and boundary types equal the
    reference's for the three threshold sets; the stage moves no point."""
    post = np.load(os.path.join(GOLD, "gof_tiny2_post.npz"))
    frames = [synth_cloud("tiny", f) for f in range(2)]
    enc = T.GofEncoder(0, workers=2, iterations=10)
    try:
        frs = enc.upload(frames)
        enc.phase_a(frs)
        enc.phase_b(frs)
        dec = [synth_decoded_attribute(fr.get_attribute_images()) for fr in frs]
        assert "".join(cs.digest(d) for d in dec) == str(post["decoded_md5"])
        enc.phase_c(frs, dec)
        plain = [fr.get_post_reconstruction() for fr in frs]
        for i, (fr, pc) in enumerate(zip(frs, plain)):
            assert cs.input_digest(pc["xyz"], pc["colors16"], pc["boundary"], patch_of_points(fr)) == str(golden["pipe_f%d_input_md5" % i])
        for t, thr in enumerate(cs.PIPELINE_THRESHOLDS):
            enc.phase_c(frs, dec, color_smoothing=(4,) + thr)
            for i, fr in enumerate(frs):
                got, key = fr.get_post_reconstruction(), "pipe_f%d_t%d" % (i, t)
                assert np.array_equal(got["colors16"], expected(plain[i]["colors16"], golden, key)), key
                assert cs.digest(got["rgb"]) == str(golden[key + "_rgb_md5"]), key
                assert np.array_equal(got["xyz"], plain[i]["xyz"]) and np.array_equal(got["boundary"], plain[i]["boundary"])
                assert cs.digest(got["boundary"]) == str(post["f%d_boundary_md5" % i]) and cs.digest(got["xyz"]) == str(post["f%d_xyz_md5" % i])
        enc.phase_c(frs, dec)                                    # None again: today's sequence of calls, today's bytes
        for fr, pc in zip(frs, plain):
            again = fr.get_post_reconstruction()
            assert all(np.array_equal(again[k], pc[k]) for k in pc)
        for fr in frs:
            fr.close()
    finally:
        enc.close(join=True)


@pytest.mark.parametrize("name", list(cs.arbitrary_cases()))
def test_gpu_color_smoothing_arbitrary_clouds_match_reference(gpu_ctx, golden, name):
    """Context.color_smoothing on arbitrary clouds (grids 2 / 4 / 8 / 16; the dense ones hold cells whose float colour sums pass
    2^24: the ordered path; segments beyond 64 points: the histogram median)."""
    xyz, c16, bt, part, grid, bits, thr = cs.arbitrary_cases()[name]
    assert cs.input_digest(xyz, c16, bt, part) == str(golden["arb_%s_input_md5" % name])
    got = gpu_ctx.color_smoothing(xyz, c16, bt, part, grid, bits, *thr)
    assert np.array_equal(got, expected(c16, golden, "arb_" + name))
    assert np.array_equal(got, T.host_color_smoothing(xyz, c16, bt, part, grid, bits, *thr))


def test_gpu_color_smoothing_refusals(gpu_ctx):
    xyz, c16, bt, part, grid, bits, thr = cs.random_case(1)
    for bad in (1, 3, 32):
        with pytest.raises(T.Tmc2Error, match="gridSize %d .*unsupported" % bad):
            gpu_ctx.color_smoothing(xyz, c16, bt, part, bad, bits, *thr)
    n = 65536
    at = np.full((n, 3), 100, np.int16)
    with pytest.raises(T.Tmc2Error, match="65536 points"):
        gpu_ctx.color_smoothing(at, np.full((n, 3), 1000, np.uint16), np.ones(n, np.uint16), (np.arange(n) % 2).astype(np.uint32), 4, 10)
    far = xyz.copy()
    far[0, 1] = 1024
    with pytest.raises(T.Tmc2Error, match="outside the cube"):
        gpu_ctx.color_smoothing(far, c16, bt, part, grid, bits, *thr)
    assert np.array_equal(gpu_ctx.color_smoothing(xyz, c16, bt, part, grid, bits, *thr), T.host_color_smoothing(xyz, c16, bt, part, grid, bits, *thr))


def test_gpu_color_smoothing_full_size_frame(golden):
    """Frame 0 of the longdress case at BASELINE size, in the decoder-side state full_size.npz pins as f0_post_*: MD5 of the smoothed
    colours and of the RGB against the reference, the host restatement on the GPU's own state, and the resident metric
    (which = 1) on the smoothed colours against tmc2_metrics_compute on the downloaded cloud."""
    name = str(golden["full_case"])
    c = FULL_SIZE_CASES[name]
    xyz, rgb = synth_cloud(c["workload"], 0)
    gof = T.GofEncoder(0, workers=1, iterations=c["iterations"], bits3d=c["bits3d"], occ_precision=c["precision"], min_w=c["min_w"],
                       min_h=c["min_h"], vox_dim=c["vox_dim"])
    try:
        fr = gof.upload([(xyz, rgb)])[0]
        gof.phase_a([fr], constrained_pack=constrained_pack(c))
        gof.phase_b([fr])
        fr.codec_set_decoded_attribute_yuv420(fr.encoder_attribute_to_yuv420(4), 0)
        fr.codec_post_reconstruct(None)
        plain, part = fr.get_post_reconstruction(), patch_of_points(fr)
        assert cs.input_digest(plain["xyz"], plain["colors16"], plain["boundary"], part) == str(golden["full_f0_input_md5"])
        counts = golden["full_f0_counts"].tolist()
        assert counts[0] == len(plain["xyz"]) and counts[3] > 0
        res = float((1 << (c["bits3d"] - 1)) - 1)
        for t, thr in reversed(list(enumerate(cs.PIPELINE_THRESHOLDS))):
            fr.codec_post_reconstruct(None, color_smoothing=(c["precision"],) + thr)
            got = fr.get_post_reconstruction()
            assert cs.digest(got["colors16"]) == str(golden["full_f0_t%d_colors16_md5" % t]), t
            assert cs.digest(got["rgb"]) == str(golden["full_f0_t%d_rgb_md5" % t]), t
            assert int((got["colors16"] != plain["colors16"]).any(1).sum()) == counts[3 + t]
            assert np.array_equal(got["xyz"], plain["xyz"]) and np.array_equal(got["boundary"], plain["boundary"])
        # (the last set run is the reference's default one)
        host = T.host_color_smoothing(plain["xyz"], plain["colors16"], plain["boundary"], part, c["precision"], c["bits3d"], *cs.PIPELINE_THRESHOLDS[0])
        assert np.array_equal(got["colors16"], host)
        resident, counts_r = fr.metrics_compute(1, True, res)
        via_host, counts_h = gof.ctxs[0].metrics_compute(xyz, rgb, got["xyz"], got["rgb"], fr.get_normals(), res)
        assert np.array_equal(resident.view(np.uint64), via_host.view(np.uint64)) and np.array_equal(counts_r, counts_h)
        before, _ = gof.ctxs[0].metrics_compute(xyz, rgb, plain["xyz"], plain["rgb"], None, res)
        assert not np.array_equal(before[:, 4:], via_host[:, 4:])          # the colour metric sees the smoothed colours
        print("color_smoothing stage ms (3 runs):", {k: round(v, 3) for k, v in gof.ctxs[0].stage_ms().items() if k in ("color_smoothing", "geometry_smoothing")})
        fr.close()
    finally:
        gof.close(join=True)


def test_gpu_color_smoothing_decoder_side_and_call_order(gpu_ctx):
    """A decoder-side frame (tmc2_decoder_frame_create: no source cloud, no segmenter) gives the same as the encoder-side frame it
    was cut from; the call out of order, or without the bit depth, returns TMC2_E_STATE."""
    xyz, rgb = synth_cloud("small", 2)
    enc = gpu_ctx.frame(xyz, rgb)
    enc.segmenter_compute(T.ctc_params(10, 11, enc.weight_normal(11, 0.6)))
    h = enc.encoder_pack_flexible(1280, 2, 1.0)
    W, H = T.encoder_canvas_size([h], 1280, 1280, 1280)
    enc.encoder_generate_geometry_images(W, H, 4)
    enc.encoder_generate_attribute_images()
    with pytest.raises(T.Tmc2Error, match="error -5") as e:          # TMC2_E_STATE: no 16-bit colours yet
        enc.codec_color_smoothing(4)
    assert "16-bit colours" in str(e.value)
    img = enc.get_geometry_images()
    i420 = enc.encoder_attribute_to_yuv420(4)
    patches = enc.get_patches()[0][enc.get_patch_order()]
    sent = np.zeros(len(patches), patches.dtype)
    for k in ("u0", "v0", "sizeU0", "sizeV0", "patchOrientation", "u1", "v1", "d1", "normalAxis", "tangentAxis", "bitangentAxis",
              "projectionMode"):
        sent[k] = patches[k]
    sent["sizeU"], sent["sizeV"] = sent["sizeU0"] * 16, sent["sizeV0"] * 16
    dec = gpu_ctx.decoder_frame(sent, W, H, 4, img["occ_video"], np.stack([img["geo0"], img["geo1"]]))
    dec.codec_generate_point_cloud()
    thr = (1.0, 10.0, 6.0)
    dec.codec_set_decoded_attribute_yuv420(i420, 0)
    with pytest.raises(T.Tmc2Error, match="geometryBitDepth3D is unknown"):
        dec.codec_post_reconstruct(None, color_smoothing=(4,) + thr)
    dec.set_geometry_bit_depth_3d(11)
    dec.codec_post_reconstruct(None, color_smoothing=(4,) + thr)
    got = dec.get_post_reconstruction()
    enc.codec_set_decoded_attribute_yuv420(i420, 0)
    enc.codec_post_reconstruct(None)
    plain = enc.get_post_reconstruction()
    enc.codec_post_reconstruct(None, color_smoothing=(4,) + thr)
    same = enc.get_post_reconstruction()
    for k in ("xyz", "colors16", "rgb", "boundary"):
        assert np.array_equal(got[k], same[k]), k
    host = T.host_color_smoothing(plain["xyz"], plain["colors16"], plain["boundary"], patch_of_points(enc), 4, 11, *thr)
    assert np.array_equal(same["colors16"], host) and (host != plain["colors16"]).any()
    dec.close(), enc.close()


def test_gpu_color_smoothing_sixteen_contexts_in_flight():
    """The 8-frame tiny / small mix twice over, sixteen contexts in flight, with the stage on: the same bytes as one context."""
    mix = [synth_cloud("tiny" if f % 2 == 0 else "small", f) for f in range(8)]
    thr = (4, 1.0, 10.0, 6.0)

    def run(frames, workers):
        enc = T.GofEncoder(0, workers=workers, iterations=10)
        try:
            frs = enc.upload(frames)
            enc.phase_a(frs)
            enc.phase_b(frs)
            out = []
            for rep in range(2):
                enc.phase_c(frs, color_smoothing=thr)
                out.append(enc.per_frame(frs, lambda fr, i: fr.get_post_reconstruction()))
            for fr in frs:
                fr.close()
            return out
        finally:
            enc.close(join=True)
    # (the canvas of a GOF is the tallest frame's: both runs hold the same eight frames)
    one = run(mix, 1)[0]
    many = run(mix + mix, 16)
    assert any((pc["boundary"] == 1).sum() > 100 for pc in one)
    for rep in many:
        for i, pc in enumerate(rep):
            for k in ("xyz", "colors16", "rgb", "boundary"):
                assert np.array_equal(pc[k], one[i % 8][k]), (i, k)
