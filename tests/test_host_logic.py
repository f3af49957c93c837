"""CPU tier: the product's host-side logic (k-d tree builder, spanning-tree orientation) and the C-ABI
surface.  No compute kernels run here -- there is no GPU in this tier."""
import ctypes
import os
import re

import numpy as np
import pytest

import tmc2_amd as T
from tmc2_amd.synth import synth_cloud

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def test_library_exports_every_declared_symbol():
    hdr = open(os.path.join(ROOT, "include", "tmc2hip.h")).read()
    names = sorted(set(re.findall(r"\b(tmc2_[a-z0-9_]+)\s*\(", hdr)))
    assert len(names) > 25
    lib = T.load_library()
    missing = [n for n in names if not hasattr(lib, n)]
    assert not missing, "declared in tmc2hip.h but not exported: %s" % missing


def test_native_gof_host_exports_its_header_and_refuses_bad_arguments():
    """libtmc2gof.so (include/tmc2gof.h): every declared entry is exported; argument errors come back as TMC2_E_INVALID before
    any device work (no GPU here)."""
    import ctypes as C
    from tmc2_amd import native_gof
    hdr = open(os.path.join(ROOT, "include", "tmc2gof.h")).read()
    names = sorted(set(re.findall(r"\b(tmc2_gof_[a-z0-9_]+)\s*\(", hdr)))
    assert names == ["tmc2_gof_comm_create", "tmc2_gof_comm_destroy", "tmc2_gof_encode", "tmc2_gof_encode_resume", "tmc2_gof_encode_sharded",
                     "tmc2_gof_encode_sharded_resume", "tmc2_gof_last_error", "tmc2_gof_slot_core"]
    G = native_gof.load_library()
    assert not [n for n in names if not hasattr(G, n)]
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert not [n for n in names if n not in doc], "not in INTEGRATION.md"
    cfg = native_gof.GofConfig(10, 4, 11, 4, 1280, 1280, 0, 0)
    W, H = C.c_int32(0), C.c_int32(0)
    invalid = int(re.search(r"#define TMC2_E_INVALID (-?\d+)", open(os.path.join(ROOT, "include", "tmc2hip.h")).read()).group(1))
    none = None
    assert G.tmc2_gof_encode(none, none, 0, 1, C.byref(cfg), none, none, none, none, none, none, 1280, 1280, C.byref(W), C.byref(H)) == invalid
    handles, slot = (C.c_void_p * 1)(None), (C.c_int32 * 1)(0)
    assert G.tmc2_gof_encode(handles, slot, 1, 1, C.byref(cfg), none, none, none, none, none, none, 1280, 1280, C.byref(W), C.byref(H)) == invalid
    handles, slot = (C.c_void_p * 1)(1), (C.c_int32 * 1)(3)   # slot out of range: refused before the handle is touched
    assert G.tmc2_gof_encode(handles, slot, 1, 2, C.byref(cfg), none, none, none, none, none, none, 1280, 1280, C.byref(W), C.byref(H)) == invalid


def test_native_gof_host_names_the_core_of_a_slot():
    """tmc2_gof_slot_core: the core a pass pins a slot's thread to -- one of the CPUs this process may run on, or -1 where the cache
    topology cannot be read -- and the same answer every time (the list is kept)."""
    from tmc2_amd import native_gof
    G = native_gof.load_library()
    allowed = os.sched_getaffinity(0)
    first = [G.tmc2_gof_slot_core(s) for s in range(40)]
    assert all(c == -1 or c in allowed for c in first), (first, sorted(allowed))
    assert len({c == -1 for c in first}) == 1                                     # (readable for every slot or for none)
    assert [G.tmc2_gof_slot_core(s) for s in range(40)] == first
    assert G.tmc2_gof_slot_core(-1) == -1


def test_every_declared_symbol_is_bound_and_documented():
    """Each entry of include/tmc2hip.h has its ctypes binding (tmc2_amd/lib.py) and its reference counterpart in
    INTEGRATION.md -- the drop-in boundary stays in step with its documentation."""
    hdr = open(os.path.join(ROOT, "include", "tmc2hip.h")).read()
    names = sorted(set(re.findall(r"\b(tmc2_[a-z0-9_]+)\s*\(", hdr)))
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    binding = open(os.path.join(ROOT, "mpeg-pcc-tmc2_amd", "tmc2_amd", "lib.py")).read()
    assert not [n for n in names if n not in doc], "not in INTEGRATION.md"
    assert not [n for n in names if n not in binding], "not bound in lib.py"


def _header(name):
    """include/<name> without its comments and preprocessor lines"""
    text = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)
    return re.sub(r"^\s*#.*$", "", text, flags=re.M)


def _c_type(declarator):
    """'const int16_t* xyz' -> 'const int16_t*', 'double weight[3]' -> 'double[3]': a parameter's type without its name"""
    base, dim = re.fullmatch(r"(.*?)\s*\b\w+\s*(\[\d+\])?", " ".join(declarator.split())).groups()
    return re.sub(r"\s*\*", "*", base) + (dim or "")


def _declared_prototypes(name):
    """{function: 'ret function(type, ...)'} of a header, spelled as the rows of tmc2_amd/lib.py are"""
    out = {}
    for ret, fn, params in re.findall(r"([\w\s*]+?)\b(tmc2_\w+)\s*\(([^)]*)\)\s*;", _header(name)):
        types = "void" if params.strip() == "void" else ", ".join(_c_type(p) for p in params.split(","))
        assert fn not in out, "%s is declared twice" % fn
        out[fn] = "%s %s(%s)" % (re.sub(r"\s*\*", "*", " ".join(ret.split())), fn, types)
    return out


# The rule of tmc2_amd/lib.py, restated: scalars by their exact width; `const char*` is c_char_p; every other pointer (handles,
# out-parameters, arrays, struct pointers, a returned void*) is c_void_p; a function that returns void has restype None.
_C_SCALARS = {"void": None, "int": ctypes.c_int, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "uint64_t": ctypes.c_uint64,
              "size_t": ctypes.c_size_t, "long": ctypes.c_long, "double": ctypes.c_double}


def _expected_ctype(c_type):
    if c_type == "const char*":
        return ctypes.c_char_p
    return ctypes.c_void_p if c_type[-1] in "*]" else _C_SCALARS[c_type]


def test_installed_prototypes_match_the_headers():
    """Types, not only names: the table of tmc2_amd/lib.py has exactly the functions the two headers declare, with the header's
    return and parameter types, and what load_library() installed on each function is what the mapping rule gives for them."""
    from tmc2_amd import lib as binding, native_gof
    for header, rows, lib in (("tmc2hip.h", binding.TMC2HIP, T.load_library()), ("tmc2gof.h", native_gof.TMC2GOF, native_gof.load_library())):
        declared = _declared_prototypes(header)
        assert set(declared) == set(re.findall(r"\b(tmc2_[a-z0-9_]+)\s*\(", _header(header))), "a declaration the parser missed"
        table = {re.search(r"\b(tmc2_\w+)\(", row).group(1): row for row in rows}
        assert len(table) == len(rows), "a function has two rows"
        assert table == declared, "%s and its table in tmc2_amd/lib.py disagree" % header
        for fn, row in declared.items():
            ret, params = re.fullmatch(r"(.+?) %s\((.*)\)" % fn, row).groups()
            want = [] if params == "void" else [_expected_ctype(t) for t in params.split(", ")]
            got = getattr(lib, fn)
            assert got.restype is _expected_ctype(ret) and got.argtypes == want, \
                "%s: installed %s %s, the header says %s" % (fn, got.restype, got.argtypes, row)


def test_struct_mirrors_match_the_headers():
    """SegmenterParams, Patch and GofConfig have the fields of the header's structs -- names, order, types -- and PATCH_DTYPE lays a
    record out as Patch does."""
    from tmc2_amd import lib, native_gof
    scalar = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "double": ctypes.c_double}
    for header, struct, mirror in (("tmc2hip.h", "tmc2_segmenter_params", T.SegmenterParams), ("tmc2hip.h", "tmc2_patch", T.Patch),
                                   ("tmc2gof.h", "tmc2_gof_config", native_gof.GofConfig)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), _header(header), flags=re.S).group(1)
        fields = []
        for decl in filter(None, (" ".join(d.split()) for d in body.split(";"))):
            c_type, names = decl.split(" ", 1)
            for name, dim in re.findall(r"(\w+)(?:\[(\d+)\])?", names):
                fields.append((name, scalar[c_type] * int(dim) if dim else scalar[c_type]))
        assert len(fields) >= 8 and mirror._fields_ == fields, "%s and %s disagree" % (struct, mirror.__name__)
    dt = lib.PATCH_DTYPE
    assert dt.names == tuple(n for n, _ in T.Patch._fields_) and dt.itemsize == ctypes.sizeof(T.Patch)
    for n, t in T.Patch._fields_:
        assert dt.fields[n] == (np.dtype(t), getattr(T.Patch, n).offset), n


def test_pool_poison_option_values():
    """POOL_POISON takes a byte, decimal or 0x..; tmc2_option_check is tmc2_ctx_set_option's own check without a context (a context
    needs a device: the set / get round trip on one is tests/test_gpu_pool_poison.py::test_gpu_probe_unset_option_fills_nothing)"""
    from tmc2_amd import lib
    for good in ("0", "255", "0x5A", "90", "0xff", "0X00", 7):
        lib.option_check("POOL_POISON", good)
        lib.option_check("TMC2_POOL_POISON", good)
    for bad in ("256", "-1", "zz", "", "0x", "0x100", " 5", "5 ", "1e2", "0x5G", "+3", "99999999999999999999"):
        with pytest.raises(T.Tmc2Error, match=r"error -3: option POOL_POISON"):          # TMC2_E_INVALID
            lib.option_check("POOL_POISON", bad)
    lib.option_check("POOL_POISON", None)                    # unsetting is always accepted
    lib.option_check("KD_HUGEMAX", "zz")                     # the options read where they are used keep taking any text
    lib.option_check("POOL_POISON_STAGE", "kdtree_build")
    with pytest.raises(T.Tmc2Error, match="error -3"):
        lib.option_check("", "1")


def test_no_cpu_fallback_without_device():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible")
    with pytest.raises(T.Tmc2Error, match="no HIP device"):
        T.Context(0)


@pytest.mark.parametrize("name", ["tiny", "small"])
def test_host_kdtree_matches_oracle(oracle, name):
    xyz, _ = synth_cloud(name)
    perm, nodes, depth = T.host_kdtree_build(xyz)
    operm, onodes = oracle.kdtree_perm(xyz)
    assert np.array_equal(perm, operm) and nodes == onodes and 1 < depth <= 64


def test_host_kdtree_degenerate_inputs(oracle):
    rng = np.random.default_rng(5)
    # coplanar, collinear, heavy ties on the cut plane, fewer points than one leaf
    cases = [np.stack([rng.integers(0, 40, 500), np.full(500, 7), rng.integers(0, 40, 500)], 1),
             np.stack([np.arange(300), np.zeros(300), np.zeros(300)], 1),
             np.stack([rng.integers(0, 3, 800), rng.integers(0, 200, 800), rng.integers(0, 3, 800)], 1),
             rng.integers(0, 1024, (7, 3))]
    for c in cases:
        c = np.unique(c.astype(np.int16), axis=0)
        perm, nodes, _ = T.host_kdtree_build(c)
        operm, onodes = oracle.kdtree_perm(c)
        assert np.array_equal(perm, operm) and nodes == onodes


@pytest.mark.parametrize("name", ["tiny", "small", "small_noisy"])      # (_noisy: a rough shell -- inconsistent cycles of strong edges)
def test_host_orientation_matches_oracle(oracle, name):
    xyz, _ = synth_cloud(name)
    knn = oracle.knn_self(xyz, 16)
    raw = oracle.compute_normals(xyz, knn)
    assert np.array_equal(bits(T.host_orient_normals(xyz, knn, raw)), bits(oracle.orient_normals(xyz, knn, raw)))


def test_host_orientation_disconnected_components(oracle):
    xyz, _ = synth_cloud("tiny")
    two = np.concatenate([xyz, xyz + np.array([300, 0, 0], np.int16)])
    knn = oracle.knn_self(two, 16)
    raw = oracle.compute_normals(two, knn)
    assert np.array_equal(bits(T.host_orient_normals(two, knn, raw)), bits(oracle.orient_normals(two, knn, raw)))


def test_host_orientation_compact_and_per_point_walks_agree(oracle):
    """The walk over the compact contracted graph (clusters numbered by first member, per pair of clusters the light edges of
    largest |n_u . n_v| + one strong edge per sign: what the device hands to the host) gives the reference's normals on a
    180 K-point cloud with several components.  (The walk over the full cross-edge list with per-point arrays it was once
    compared with has been removed.)"""
    xyz, _ = synth_cloud("medium")
    two = np.unique(np.concatenate([xyz, (xyz[::3] // 2 + np.array([700, 20, 40])).astype(np.int16)]), axis=0)
    knn = oracle.knn_self(two, 16)
    raw = oracle.compute_normals(two, knn)
    exp = oracle.orient_normals(two, knn, raw)
    assert np.array_equal(bits(T.host_orient_normals(two, knn, raw)), bits(exp))


@pytest.mark.parametrize("tau", ["0.0", "0.5", "0.9", "0.98", "0.9999", "4"])
def test_host_orientation_strong_edge_thresholds(oracle, tau, tmp_path):
    """The strong-edge shortcut of the orientation (breadth-first absorption of >= tau edges, verified for sign
    consistency, repeated with a tighter threshold / the plain growth on disagreement) must give the reference's
    result for ANY threshold: 0 makes every edge strong (fails the check at once on real clouds and falls back),
    4 disables it.  The threshold is read once per process, hence the subprocess."""
    import subprocess, sys, os
    xyz, _ = synth_cloud("small")
    knn = oracle.knn_self(xyz, 16)
    raw = oracle.compute_normals(xyz, knn)
    exp = oracle.orient_normals(xyz, knn, raw)
    np.savez(tmp_path / "in.npz", xyz=xyz, knn=knn, raw=raw)
    code = ("import sys, numpy as np; sys.path.insert(0, %r); import tmc2_amd as T; z = np.load(%r);"
            "np.save(%r, T.host_orient_normals(z['xyz'], z['knn'], z['raw']))"
            % (os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mpeg-pcc-tmc2_amd"),
               str(tmp_path / "in.npz"), str(tmp_path / "out.npy")))
    subprocess.run([sys.executable, "-c", code], check=True, env=dict(os.environ, TMC2_ORIENT_TAU=tau))
    assert np.array_equal(bits(np.load(tmp_path / "out.npy")), bits(exp))


@pytest.mark.parametrize("name,nframes", [("tiny", 4), ("small", 3)])
def test_host_spatial_consistency_packing_matches_oracle(oracle, name, nframes):
    """S10' (low-delay condition): the product's placement logic on plain records against the oracle's restatement of
    spatialConsistencyPackFlexible, frame after frame (each frame is packed against the product's own previous result)."""
    frames = [synth_cloud(name, f) for f in range(nframes)]
    w = oracle.weight_normal(frames[0][0], 11, 0.6)
    import oracle_binding as ob
    sp = ob.seg_params(10, 11, w)
    prev_list = None
    for f, (xyz, rgb) in enumerate(frames):
        seg = oracle.segment(xyz, rgb, sp)
        if prev_list is None:
            placed, order, _ = oracle.pack_flexible(seg["patches"], seg["occupancy"], 1280)
        else:
            placed, order, match, h = T.host_pack_spatial_consistency(seg["patches"], seg["occupancy"], prev_list, 1280)
            ep, eo, em, eh = oracle.pack_spatial_consistency(seg["patches"], seg["occupancy"], prev_list, 1280)
            assert h == eh and np.array_equal(order, eo) and np.array_equal(match, em) and (em >= 0).sum() >= 2
            for k in ("u0", "v0", "patchOrientation"):
                assert np.array_equal(placed[k], ep[k]), (f, k)
        prev_list = placed[order]


@pytest.mark.parametrize("case", ["accept", "mixed", "bad_packing", "bad_height", "bad_count", "single"])
def test_host_global_patch_allocation_matches_oracle(oracle, case):
    """S10' (random-access condition): the product's global patch allocation on plain records against the oracle's
    restatement of performDataAdaptiveGPAMethod, on GOFs / canvases that drive it through each of its outcomes."""
    import oracle_binding as ob
    from tmc2_amd.synth import two_body_gof
    from test_oracle_golden import _jumping
    frames, min_w, min_h = {
        "accept": (two_body_gof("tiny", 5, seed=1), 256, 128),
        "mixed": (two_body_gof("tiny", 6), 128, 192),
        "bad_packing": (two_body_gof("tiny", 6), 192, 160),
        "bad_height": (two_body_gof("tiny", 6), 160, 160),
        "bad_count": (_jumping([synth_cloud("tiny", f) for f in range(5)]), 512, 512),
        "single": ([synth_cloud("tiny", 0)], 256, 256),
    }[case]
    sp = ob.seg_params(10, 11, oracle.weight_normal(frames[0][0], 11, 0.6))
    per = []
    for xyz, rgb in frames:
        seg = oracle.segment(xyz, rgb, sp)
        if per:
            _, pplaced, porder, _ = per[-1]
            placed, order, match, h = oracle.pack_spatial_consistency(seg["patches"], seg["occupancy"], pplaced[porder], min_w)
            seg["matches"] = match
        else:
            placed, order, h = oracle.pack_flexible(seg["patches"], seg["occupancy"], min_w)
            seg["matches"] = np.full(len(order), -1, np.int32)
        per.append((seg, placed, order, h))
    exp = oracle.global_patch_allocation(per, min_w, min_h)
    tw, th = oracle.tile_size(per, min_w, min_h)
    got = T.host_global_patch_allocation([placed[order] for _, placed, order, _ in per], [seg["occupancy"] for seg, _, _, _ in per],
                                         [seg["matches"] for seg, _, _, _ in per], tw, th, min_w, min_h)
    assert len(got) == len(exp)
    grew = False
    for f, ((gl, go, gm, gw, gh), (el, eo, em, ew, eh)) in enumerate(zip(got, exp)):
        assert (gw, gh) == (ew, eh), f
        assert np.array_equal(gm, em), f
        for n in el.dtype.names:
            assert np.array_equal(gl[n], el[n]), (f, n)
        assert np.array_equal(go, eo[:len(go)]) and len(go) == int((el["sizeU0"] * el["sizeV0"]).sum()), f
        grew |= bool((np.sort(gl["sizeU0"] * gl["sizeV0"]) != np.sort(per[f][1]["sizeU0"] * per[f][1]["sizeV0"])).any())
    if case in ("accept", "mixed"):
        assert any((gm >= 0).any() for _, _, gm, _, _ in got)             # some sub-context spans several frames
    if case == "accept":
        assert grew                                                        # tracked patches took their union's box


def _ply_inputs():
    xyz, rgb = synth_cloud("tiny", 0)
    return xyz[:1500].copy(), rgb[:1500].copy()


@pytest.mark.parametrize("case", ["ascii_float", "ascii_mixed", "ascii_short", "binary_float_normals", "binary_mixed",
                                  "binary_int32_named", "binary_short"])
@pytest.mark.parametrize("read_normals", [False, True])
def test_host_ply_read_matches_oracle_and_reference(tmp_path, case, read_normals):
    """PCCPointSet3::read: the product's reader against the numpy restatement (oracle/port_io.py) and, where it is present,
    the compiled reference, on every header / body variant the reference distinguishes."""
    import importlib.util
    from ply_cases import cases
    spec = importlib.util.spec_from_file_location("port_io", os.path.join(os.path.dirname(__file__), "..", "oracle", "port_io.py"))
    port_io = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(port_io)
    xyz, rgb = _ply_inputs()
    path = tmp_path / (case + ".ply")
    path.write_bytes(cases(xyz, rgb)[case])
    exp = port_io.ply_read(str(path), read_normals)
    for threads in (1, 3, 8):
        got = T.ply_read(str(path), read_normals, threads)
        for g, e in zip(got, exp):
            assert (g is None) == (e is None)
            assert g is None or np.array_equal(g, e)
    n, has_rgb, has_nrm = T.ply_info(str(path), read_normals)
    assert n == len(exp[0]) and has_rgb == (exp[1] is not None) and has_nrm == (exp[2] is not None)
    if case == "ascii_float":
        assert np.array_equal(exp[0], xyz) and np.array_equal(exp[1], rgb)          # and it is the cloud that was written
    import oracle_binding as ob
    if os.path.exists(ob.REF_PATH):
        ref = ob.Reference().ply_read(str(path), read_normals)
        for k, (g, e) in enumerate(zip(got, ref)):
            assert (g is None) == (e is None)
            if g is not None and case == "binary_short" and k == 2:
                cut = int(np.flatnonzero(g.any(1))[-1]) + 1      # the property the file ends in is an uninitialised local there
                g, e = g[:cut], e[:cut]
            assert g is None or np.array_equal(g, e)


def test_host_ply_read_refuses_what_the_reference_misreads(tmp_path):
    from ply_cases import cases
    xyz, rgb = _ply_inputs()
    files = cases(xyz, rgb)
    bad = {"big_endian": files["binary_float_normals"].replace(b"binary_little_endian", b"binary_big_endian"),
           "not_ply": b"plx\n" + files["ascii_float"][4:],
           "no_coordinates": files["ascii_float"].replace(b"property float z", b"property float w"),
           "unknown_type": files["ascii_float"].replace(b"property float x", b"property half x"),
           "too_few_columns": files["ascii_float"].replace(b"end_header\n", b"end_header\n1 2\n", 1)}
    for name, data in bad.items():
        p = tmp_path / (name + ".ply")
        p.write_bytes(data)
        with pytest.raises(T.Tmc2Error):
            T.ply_read(str(p))
    with pytest.raises(T.Tmc2Error):
        T.ply_read(str(tmp_path / "missing.ply"))


@pytest.mark.parametrize("reorder", [False, True])
@pytest.mark.parametrize("colors", [True, False])
def test_host_checksum_matches_oracle_and_reference(reorder, colors):
    """PCCPointSet3::computeChecksum: MD5 (own implementation) over positions and colours, with and without the reordering
    that merges duplicate positions; against hashlib / numpy and, where present, the compiled reference."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("port_io", os.path.join(os.path.dirname(__file__), "..", "oracle", "port_io.py"))
    port_io = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(port_io)
    import oracle_binding as ob
    xyz, rgb = synth_cloud("tiny", 1)
    rng = np.random.default_rng(5)
    dup = rng.choice(len(xyz), 400)
    xyz = np.concatenate([xyz, xyz[dup], xyz[dup[:100]]])                     # duplicate positions with other colours
    rgb = np.concatenate([rgb, rng.integers(0, 256, (500, 3), dtype=np.uint8)])
    perm = rng.permutation(len(xyz))
    xyz, rgb = xyz[perm], rgb[perm]
    for n in (0, 1, 9, 10, 11, 21, 22, len(xyz)):                             # lengths around the 64-byte MD5 block boundaries
        c = rgb[:n] if colors else None
        exp = port_io.checksum(xyz[:n], c, reorder)
        assert T.point_set_checksum(xyz[:n], c, reorder) == exp, n
        if os.path.exists(ob.REF_PATH) and n:
            assert ob.Reference().checksum(xyz[:n], c, reorder) == exp, n
    # the position order is a counting sort per coordinate: negative coordinates, a constant axis, one occupied position
    for cloud in (rng.integers(-300, 300, (5000, 3)), rng.integers(0, 40, (5000, 3)) * [1, 0, 1] + [0, -7, 0], np.full((64, 3), 11)):
        cloud = cloud.astype(np.int16)
        c = rng.integers(0, 256, (len(cloud), 3), dtype=np.uint8) if colors else None
        exp = port_io.checksum(cloud, c, reorder)
        assert T.point_set_checksum(cloud, c, reorder) == exp
        if os.path.exists(ob.REF_PATH):
            assert ob.Reference().checksum(cloud, c, reorder) == exp


def test_host_ply_read_and_checksum_match_golden_fixture(tmp_path):
    """The same, against the fixture the unmodified reference produced (tests/golden/io_golden.npz)."""
    import hashlib
    from ply_cases import cases
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "io_golden.npz"))
    digest = lambda a: hashlib.md5(np.ascontiguousarray(a).tobytes()).hexdigest()
    xyz, rgb = _ply_inputs()
    assert str(g["input_md5"]) == digest(xyz) + digest(rgb)
    for name, data in cases(xyz, rgb).items():
        assert hashlib.md5(data).hexdigest() == str(g[name + "_file_md5"]), "tests/ply_cases.py drifted from the fixture"
        path = tmp_path / (name + ".ply")
        path.write_bytes(data)
        for rn in (0, 1):
            got = T.ply_read(str(path), bool(rn))
            if name == "binary_short" and got[2] is not None:
                got = (got[0], got[1], got[2][:int(np.flatnonzero(got[0].any(1))[-1])])
            assert ["" if a is None else digest(a) for a in got] == g["%s_n%d" % (name, rn)].tolist(), (name, rn)
    big = np.concatenate([xyz, xyz[:300]]), np.concatenate([rgb, rgb[300:600]])
    for reorder in (0, 1):
        assert T.point_set_checksum(big[0], big[1], bool(reorder)) == g["checksum_r%d" % reorder].tobytes()
        assert T.point_set_checksum(big[0], None, bool(reorder)) == g["checksum_nocolor_r%d" % reorder].tobytes()


def _random_patch_gof(rng, frames, patches, drift, churn):
    """Random patch records (no point cloud behind them): boxes in the (u1, v1) plane of six views that drift from frame to
    frame, some vanish, some appear; block occupancies with holes.  -> per frame (records by index, occupancy pool)."""
    import oracle_binding as ob
    base = [dict(view=int(rng.integers(0, 6)), u1=int(rng.integers(0, 600)), v1=int(rng.integers(0, 600)),
                 su=int(rng.integers(4, 150)), sv=int(rng.integers(4, 150))) for _ in range(patches)]
    out = []
    for f in range(frames):
        cur = []
        for b in base:
            if rng.random() < churn:
                continue
            cur.append(dict(b, u1=max(0, b["u1"] + int(rng.integers(-drift, drift + 1))), v1=max(0, b["v1"] + int(rng.integers(-drift, drift + 1))),
                            su=max(2, b["su"] + int(rng.integers(-drift, drift + 1))), sv=max(2, b["sv"] + int(rng.integers(-drift, drift + 1)))))
        for _ in range(int(rng.integers(0, 1 + int(patches * churn * 2)))):
            cur.append(dict(view=int(rng.integers(0, 6)), u1=int(rng.integers(0, 600)), v1=int(rng.integers(0, 600)),
                            su=int(rng.integers(4, 150)), sv=int(rng.integers(4, 150))))
        rng.shuffle(cur)
        rec = np.zeros(len(cur), ob.PATCH_DTYPE)
        pool = []
        for i, c in enumerate(cur):
            u0, v0 = (c["su"] + 15) // 16, (c["sv"] + 15) // 16
            occ = (rng.random((v0, u0)) < 0.8).astype(np.uint8)
            occ[0, 0] = 1
            rec[i]["index"], rec[i]["viewId"] = i, c["view"]
            rec[i]["u1"], rec[i]["v1"], rec[i]["sizeU"], rec[i]["sizeV"] = c["u1"], c["v1"], c["su"], c["sv"]
            rec[i]["sizeU0"], rec[i]["sizeV0"] = u0, v0
            rec[i]["occOffset"] = sum(len(p) for p in pool)
            pool.append(occ.reshape(-1))
        out.append((rec, np.concatenate(pool) if pool else np.zeros(0, np.uint8)))
    return out


# (1574, 1727, 2141: GOFs whose FIRST frame has no patches -- the global patch allocation is then left out, PCCEncoder.cpp:4812)
@pytest.mark.parametrize("seed", list(range(60)) + [1574, 1727, 2141])
def test_host_interframe_packers_random_patch_sets(oracle, seed):
    """S10' on synthetic patch records: the spatial-consistency chain and the global patch allocation of the product against
    the oracle on random GOFs -- drifting, vanishing and appearing patches on canvases from roomy to far too small, so that
    every restart branch and the canvas doubling are hit many times."""
    import oracle_binding as ob
    rng = np.random.default_rng(1000 + seed)
    frames = int(rng.integers(2, 7))
    gof = _random_patch_gof(rng, frames, int(rng.integers(3, 40)), drift=int(rng.integers(0, 30)), churn=float(rng.choice([0.0, 0.1, 0.4])))
    min_w = int(rng.choice([128, 256, 512, 1280]))
    min_h = int(rng.choice([64, 128, 256, 512, 1280]))
    per = []
    for rec, occ in gof:
        if per:
            _, pplaced, porder, _ = per[-1]
            exp_sc = oracle.pack_spatial_consistency(rec, occ, pplaced[porder], min_w)
            if exp_sc is None:         # an inherited orientation makes a patch wider than the canvas: the reference spins
                with pytest.raises(T.Tmc2Error):
                    T.host_pack_spatial_consistency(rec, occ, pplaced[porder], min_w)
                return
            placed, order, match, h = T.host_pack_spatial_consistency(rec, occ, pplaced[porder], min_w)
            ep, eo, em, eh = exp_sc
            assert h == eh and np.array_equal(order, eo) and np.array_equal(match, em)
            for k in ("u0", "v0", "patchOrientation"):
                assert np.array_equal(placed[k], ep[k]), k
        else:
            placed, order, h = T.host_pack_flexible(rec, occ, min_w)
            ep, eo, eh = oracle.pack_flexible(rec, occ, min_w)
            assert h == eh and np.array_equal(order, eo)
            for k in ("u0", "v0", "patchOrientation"):
                assert np.array_equal(placed[k], ep[k]), k
            match = np.full(len(order), -1, np.int32)
        per.append((dict(occupancy=occ, matches=match), placed, order, h))
    for rec, occ in gof[1:]:        # S10 on every frame on its own (the all-intra condition)
        placed, order, h = T.host_pack_flexible(rec, occ, min_w)
        ep, eo, eh = oracle.pack_flexible(rec, occ, min_w)
        assert h == eh and np.array_equal(order, eo)
        for k in ("u0", "v0", "patchOrientation"):
            assert np.array_equal(placed[k], ep[k]), k
    exp = oracle.global_patch_allocation(per, min_w, min_h)
    tw, th = oracle.tile_size(per, min_w, min_h)
    args = ([placed[order] for _, placed, order, _ in per], [seg["occupancy"] for seg, _, _, _ in per],
            [seg["matches"] for seg, _, _, _ in per], tw, th, min_w, min_h)
    if exp is None:            # undefined in the reference: the product must refuse, not guess
        with pytest.raises(T.Tmc2Error):
            T.host_global_patch_allocation(*args)
        return
    got = T.host_global_patch_allocation(*args)
    for f, ((gl, go, gm, gw, gh), (el, eo, em, ew, eh)) in enumerate(zip(got, exp)):
        assert (gw, gh) == (ew, eh) and np.array_equal(gm, em), f
        for n in el.dtype.names:
            assert np.array_equal(gl[n], el[n]), (f, n)
        assert np.array_equal(go, eo[:len(go)]), f


@pytest.mark.parametrize("seed", range(30))
def test_host_tree_and_orientation_on_degenerate_clouds(oracle, seed):
    """The host-resident pieces of S1 / S3 on degenerate clouds (planes, lines, lattices, dust): tree permutation against
    the oracle's nanoflann restatement, orientation against the oracle's spanning-tree walk (bit patterns)."""
    from test_oracle_golden import degenerate_cloud
    rng = np.random.default_rng(9000 + seed)
    xyz = degenerate_cloud(rng)
    if len(xyz) < 20:
        pytest.skip("too few distinct points")
    assert np.array_equal(T.host_kdtree_build(xyz)[0], oracle.kdtree_perm(xyz)[0])
    if len(xyz) >= 16:
        knn = oracle.knn_self(xyz, 16)
        raw = oracle.compute_normals(xyz, knn)
        assert np.array_equal(bits(T.host_orient_normals(xyz, knn, raw)), bits(oracle.orient_normals(xyz, knn, raw)))


@pytest.mark.parametrize("ascii_", [True, False])
@pytest.mark.parametrize("with_rgb,with_normals", [(True, False), (True, True), (False, False)])
def test_host_ply_write_is_byte_identical_to_the_reference(tmp_path, ascii_, with_rgb, with_normals):
    """PCCPointSet3::write: the files the reference writes for reconstructed frames, byte for byte (where the compiled
    reference is present), and the product's own reader gets the cloud back from them."""
    import oracle_binding as ob
    xyz, rgb = _ply_inputs()
    rng = np.random.default_rng(2)
    nrm = rng.normal(size=(len(xyz), 3)) if with_normals else None
    mine = tmp_path / "mine.ply"
    T.ply_write(str(mine), xyz, rgb if with_rgb else None, nrm, ascii_)
    got = T.ply_read(str(mine), read_normals=True)
    assert np.array_equal(got[0], xyz) and (not with_rgb or np.array_equal(got[1], rgb))
    if with_normals and not ascii_:
        assert np.array_equal(got[2], nrm.astype(np.float32).astype(np.float64))
    if os.path.exists(ob.REF_PATH):
        import ctypes as C
        theirs = tmp_path / "theirs.ply"
        L = ob.Reference().L
        x = np.ascontiguousarray(xyz, np.int16)
        c = np.ascontiguousarray(rgb, np.uint8) if with_rgb else None
        n64 = None if nrm is None else np.ascontiguousarray(nrm, np.float64)
        p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
        assert L.ref_ply_write(str(theirs).encode(), p(x), p(c), p(n64), C.c_size_t(len(x)), int(ascii_)) == 0
        assert mine.read_bytes() == theirs.read_bytes()


def test_host_orientation_one_way_strong_edge_inside_a_cluster(oracle):
    """Round 4, found by the 32-frame redandblack fixture: frame 26 of that GOF has ONE strong edge (|n_u . n_v| >= 0.98) that
    is not mutual, lies inside a cluster of mutual strong edges and disagrees with the cluster's parities -- the reference's
    growth happens to take it first and orients two points against their cluster.  The contraction must notice (every strong
    edge inside a cluster is checked, not only the mutual ones) and grow with the tighter threshold; the result is the
    reference's (its digest in tests/golden/full_size.npz)."""
    import hashlib
    xyz, _ = synth_cloud("redandblack_vox10", 26)
    knn = oracle.knn_self(xyz, 16)
    raw = oracle.compute_normals(xyz, knn)
    got = T.host_orient_normals(xyz, knn, raw)
    g = np.load(os.path.join(ROOT, "tests", "golden", "full_size.npz"))
    assert hashlib.md5(np.ascontiguousarray(got).tobytes()).hexdigest() == str(g["redandblack_vox10_ai_r3_gof32/f26_src_normals_md5"])


def test_every_bench_configuration_has_its_reference_fixture():
    """`bench.py --config <name>` verifies what it timed against the digests of the unmodified reference: every configuration of
    tmc2_amd/configs.py BENCH_CONFIGS (and every soak case) must be in tests/golden/full_size.npz with ALL its frames --
    encoder side (10 digests a frame) and decoder side (I420, 4 post-reconstruction digests, source normals, metric doubles)."""
    from tmc2_amd.configs import BENCH_CONFIGS, FULL_SIZE_CASES
    g = np.load(os.path.join(ROOT, "tests", "golden", "full_size.npz"))
    names = set(g.files)
    for short, case in BENCH_CONFIGS.items():
        c = FULL_SIZE_CASES[case]
        assert c["frames"] == (8 if short == "rough" else 32), (short, case)   # BASELINE.json: 32-frame GOFs (+ the rough shell: 8)
        for f in range(c["frames"]):
            for k in ("counts", "patches_md5", "occupancy_md5", "occ_video_md5", "block_to_patch_md5", "geo0_md5", "geo1_md5",
                      "recon_xyz_md5", "recon_rgb_md5", "point_to_pixel_md5", "attribute_md5", "i420_md5", "dec444_md5",
                      "post_xyz_md5", "post_colors16_md5", "post_rgb_md5", "post_boundary_md5", "src_normals_md5"):
                assert "%s/f%d_%s" % (case, f, k) in names, (case, f, k)
            assert g["%s/f%d_post_metrics" % (case, f)].shape == (3, 8)
    for case, c in FULL_SIZE_CASES.items():
        assert case + "/canvas" in names and case + "/input_md5" in names, case
        assert len(str(g[case + "/input_md5"])) == 64 * c["frames"]


def test_native_front_end_builds_and_fails_loudly_without_a_gpu(tmp_path):
    """integration/tmc2_encode_gof.cpp (a C++ host front end over the C-ABI, the whole GOF path) compiles against
    include/tmc2hip.h and include/tmc2gof.h -- its pass is libtmc2gof.so's -- and, on a machine without an MI355X, stops with
    the library's "no device" error instead of computing anything on the CPU."""
    import shutil
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if shutil.which("g++") is None or shutil.which("make") is None:
        pytest.skip("no host toolchain")
    subprocess.run(["make", "-C", os.path.join(root, "integration")], check=True, capture_output=True)
    exe = os.path.join(root, "integration", "tmc2_encode_gof")
    assert subprocess.run([exe, "--help"], capture_output=True).returncode == 1
    metrics_exe = os.path.join(root, "integration", "tmc2_metrics")
    xyz, rgb = synth_cloud("tiny", 0)
    T.ply_write(str(tmp_path / "fr_0000.ply"), xyz, rgb)
    r = subprocess.run([exe, "--in", str(tmp_path / "fr_%04d.ply"), "--frames", "1", "--out", str(tmp_path / "gof")],
                       capture_output=True, text=True)
    try:
        import torch
        gpu = torch.cuda.is_available()
    except ImportError:
        gpu = False
    m = subprocess.run([metrics_exe, "--uncompressedDataPath", str(tmp_path / "fr_%04d.ply"), "--reconstructedDataPath",
                        str(tmp_path / "fr_%04d.ply")], capture_output=True, text=True)
    if gpu:
        assert r.returncode == 0 and (tmp_path / "gof_checksums.txt").exists()
        assert m.returncode == 0 and "mseF,PSNR (p2point): inf" in m.stdout          # a cloud against itself
    else:
        assert r.returncode == 2 and "no HIP device" in r.stderr and not list(tmp_path.glob("gof_*"))
        assert m.returncode == 2 and "no HIP device" in m.stderr and not m.stdout


@pytest.mark.parametrize("with_normals", [True, False])
def test_host_metrics_display_text_matches_the_reference(oracle, with_normals):
    """PCCMetrics::display(): the log lines the CTC parsers read, rebuilt from the numbers the metric entry returns (here the
    oracle's, bit-identical to tmc2_metrics_compute) -- against the reference's own stdout at the applications' precision."""
    import ctypes as C
    import oracle_binding as ob
    if not os.path.exists(ob.REF_PATH):
        pytest.skip("compiled reference not present")
    xyz, rgb = synth_cloud("tiny", 0)
    rng = np.random.default_rng(4)
    rec = np.concatenate([xyz[:5000] + rng.integers(-1, 2, (5000, 3)).astype(np.int16), xyz[:300]])    # noise + duplicates
    rec_rgb = rng.integers(0, 256, (len(rec), 3), dtype=np.uint8)
    nrm = oracle.normals(xyz, 16, True) if with_normals else None
    q, counts = oracle.metrics(xyz, rgb, rec, rec_rgb, nrm, 1023.0)
    text = T.metrics_display(q, len(xyz), len(rec), counts, 1023, with_normals, 9)
    L = ob.Reference().L
    L.ref_metrics_display.restype = C.c_int64
    p = lambda a: None if a is None else np.ascontiguousarray(a).ctypes.data_as(C.c_void_p)
    buf = C.create_string_buffer(1 << 16)
    x, c, rx, rc = (np.ascontiguousarray(a) for a in (xyz, rgb, rec, rec_rgb))
    n64 = None if nrm is None else np.ascontiguousarray(nrm, np.float64)
    size = L.ref_metrics_display(p(x), p(c), C.c_size_t(len(x)), p(rx), p(rc), C.c_size_t(len(rx)), p(n64), C.c_double(1023.0), buf,
                                 C.c_int64(len(buf)))
    assert 0 < size < len(buf)
    assert text == buf.value.decode()
    assert "mseF,PSNR (p2point): " in text and ("mse1      (p2plane)" in text) == with_normals


def test_host_checksum_file_is_byte_identical_to_the_reference(tmp_path):
    """PCCChecksum::write: the .checksum file next to the bitstream (frame count, checksum size, one hex line per frame), and reading it back."""
    import ctypes as C
    import oracle_binding as ob
    clouds = [synth_cloud("tiny", f) for f in range(3)]
    digests = [T.point_set_checksum(x, c, False) for x, c in clouds]
    mine = tmp_path / "mine.checksum"
    T.checksum_file_write(str(mine), digests)
    assert T.checksum_file_read(str(mine)) == digests
    assert mine.read_text().split("\n")[:2] == ["3", "16"]
    if os.path.exists(ob.REF_PATH):
        L = ob.Reference().L
        xyz = np.ascontiguousarray(np.concatenate([x for x, _ in clouds]), np.int16)
        rgb = np.ascontiguousarray(np.concatenate([c for _, c in clouds]), np.uint8)
        counts = np.array([len(x) for x, _ in clouds], np.int64)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        L.ref_checksum_file_write(str(tmp_path / "theirs.bin").encode(), p(xyz), p(rgb), p(counts), 3)
        assert mine.read_bytes() == (tmp_path / "theirs.checksum").read_bytes()


def test_segmenter_params_check_accepts_ctc_and_names_what_it_refuses():
    """tmc2_segmenter_params_check: the CTC lossy parameter sets pass; options the path does not implement are refused
    with a message instead of being computed differently from the reference."""
    for it, bits in ((50, 10), (20, 11), (10, 11)):
        T.segmenter_params_check(T.ctc_params(it, bits))
    for field, value in (("nnNormalEstimation", 12), ("maxNNCountPatchSegmentation", 8), ("normalOrientation", 2),
                         ("gridBasedRefineSegmentation", 0), ("occupancyResolution", 8), ("mapCountMinus1", 0)):
        p = T.ctc_params()
        setattr(p, field, value)
        with pytest.raises(T.Tmc2Error) as e:
            T.segmenter_params_check(p)
        assert "params" in str(e.value)
    # values no stage can compute (a division by minLevel, negative sizes and counts, thresholds cast to unsigned, a ball the
    # LDS tile does not hold), and the range in which the reference's own patch loop never ends: refused by name, before a launch
    for field, value in (("minLevel", 0), ("minLevel", -64), ("minLevel", 512), ("surfaceThickness", -1), ("maxPatchSize", 0),
                         ("maxPatchSize", -1024), ("minPointCountPerCCPatchSegmentation", -1), ("quantizerSizeX", -16),
                         ("quantizerSizeY", -1), ("maxAllowedDist2RawPointsDetection", -1.0), ("maxAllowedDist2RawPointsSelection", -0.5),
                         ("maxAllowedDist2RawPointsDetection", 28.0), ("maxAllowedDist2RawPointsSelection", float("nan")),
                         ("maxAllowedDepth", 66), ("maxAllowedDepth", 63), ("maxAllowedDepth", -1), ("surfaceThickness", 193),
                         ("geometryBitDepth2D", 0), ("geometryBitDepth3D", 17), ("maxNNCountRefineSegmentation", 0),
                         ("lambdaRefineSegmentation", -1.0), ("voxelDimensionRefineSegmentation", 3),
                         ("voxelDimensionRefineSegmentation", 1), ("voxelDimensionRefineSegmentation", 0),
                         ("searchRadiusRefineSegmentation", 392), ("searchRadiusRefineSegmentation", 3),
                         ("searchRadiusRefineSegmentation", -192)):
        p = T.ctc_params()
        setattr(p, field, value)
        with pytest.raises(T.Tmc2Error) as e:
            T.segmenter_params_check(p)
        assert "params: " in str(e.value) and field in str(e.value), (field, value, str(e.value))
    for field, value in (("maxAllowedDepth", 67), ("searchRadiusRefineSegmentation", 391), ("minLevel", 128),
                         ("maxAllowedDist2RawPointsDetection", 27.9), ("surfaceThickness", 192)):
        p = T.ctc_params()
        setattr(p, field, value)
        T.segmenter_params_check(p)                 # the last value on the accepted side of each bound


def test_segmenter_params_check_accepts_the_parameter_table_and_refuses_what_never_ends():
    """Every point of tests/param_cases.py passes the check; of the points on which the reference does not return, those whose
    cause lies in the parameters alone (the depth filter) are refused -- the others depend on the cloud, and the patch loop ends
    the call when it meets them."""
    import param_cases as pc
    for p in pc.POINTS:
        T.segmenter_params_check(pc.apply(T.ctc_params(), p))
    for p in pc.OUTSIDE:
        if pc.OUTSIDE_STALL[p["name"]] == 2:
            with pytest.raises(T.Tmc2Error) as e:
                T.segmenter_params_check(pc.apply(T.ctc_params(), p))
            assert "params: maxAllowedDepth" in str(e.value)


@pytest.mark.parametrize("seed", list(range(30)) + [1574])
def test_host_pack_gof_records_matches_the_oracle_chain(oracle, seed):
    """placeSegments over the patch records of a GOF (what rank 0 runs when the frames live on several ranks): the low-delay
    chain and the random-access condition, lists / matches / pools / tile sizes against the oracle's packers."""
    rng = np.random.default_rng(1000 + seed)
    frames = int(rng.integers(2, 7))
    gof = _random_patch_gof(rng, frames, int(rng.integers(3, 40)), drift=int(rng.integers(0, 30)), churn=float(rng.choice([0.0, 0.1, 0.4])))
    min_w = int(rng.choice([128, 256, 512, 1280]))
    min_h = int(rng.choice([64, 128, 256, 512, 1280]))
    per = []
    for rec, occ in gof:
        if per:
            step = oracle.pack_spatial_consistency(rec, occ, per[-1][1][per[-1][2]], min_w)
            if step is None:
                with pytest.raises(T.Tmc2Error):
                    T.host_pack_gof_records(gof, 1, min_w, min_h)
                return
            placed, order, match, h = step
        else:
            placed, order, h = oracle.pack_flexible(rec, occ, min_w)
            match = np.full(len(order), -1, np.int32)
        per.append((dict(occupancy=occ, matches=match), placed, order, h))
    got = T.host_pack_gof_records(gof, 1, min_w, min_h)
    for (seg, placed, order, h), (gl, gpool, gm, gw, gh) in zip(per, got):
        el = placed[order]
        assert gh == h and np.array_equal(gm, seg["matches"])
        assert all(np.array_equal(gl[n], el[n]) for n in el.dtype.names)
        assert np.array_equal(gpool, seg["occupancy"])
    assert max([min_w] + [g[3] for g in got]) == oracle.tile_size(per, min_w, min_h)[0]
    exp = oracle.global_patch_allocation(per, min_w, min_h)
    if exp is None:                                            # undefined / never returning in the reference: refused
        with pytest.raises(T.Tmc2Error):
            T.host_pack_gof_records(gof, 2, min_w, min_h)
        return
    got = T.host_pack_gof_records(gof, 2, min_w, min_h)
    for (el, eo, em, ew, eh), (gl, go, gm, gw, gh) in zip(exp, got):
        assert (gw, gh) == (ew, eh) and np.array_equal(gm, em)
        assert all(np.array_equal(gl[n], el[n]) for n in el.dtype.names)
        assert np.array_equal(go, eo[:len(go)])


def test_bench_cpu_baseline_leg_reports_one_core_and_all_cores():
    """bench.py's cpu_baseline leg (the checker timed as the reported baseline, never part of the product path): the
    one-thread figure and, flat next to it, the figure of a GOF through the reference's own TBB path (its ENABLE_TBB build)
    on the physical cores, on the smallest workload."""
    import importlib.util
    import oracle_binding as ob
    spec = importlib.util.spec_from_file_location("bench_module", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    from tmc2_amd.synth import synth_cloud
    from tmc2_amd.configs import FULL_SIZE_CASES
    case = dict(FULL_SIZE_CASES["longdress_vox10_ai_r3_gof32"], name="longdress_vox10_ai_r3_gof32")
    res = bench.cpu_baseline("tiny", 2, [synth_cloud("tiny", f) for f in range(4)], case)
    assert res["unit"] == "frames/s" and res["cores"] == 1 and res["value"] > 0 and res["kind"] in ("reference", "port")
    if os.path.exists(ob.REF_TBB_PATH):
        assert "all_cores_error" not in res, res
        assert res["all_cores_value"] > 0 and res["all_cores"] == bench.physical_cores() and "TBB" in res["all_cores_sample"]
    assert "frame_processes_error" not in res, res
    assert res["frame_processes_value"] > 0 and 1 <= res["frame_processes"] <= 32
    if os.path.exists(os.path.join(ROOT, "oracle", "_ref", "PccAppEncoder")):
        # the reference's CLI end to end on one frame, from the flattened CTC options alone (no cfg folder at run time)
        assert "error" not in res["cli"], res["cli"]
        assert res["cli"]["wall_s"] > 0 and 0 < res["cli"]["path_share"]


def test_reference_tbb_build_gives_the_serial_results(reference):
    """oracle/_ref/libtmc2ref_tbb.so (ENABLE_TBB + the vendored TBB, what bench.py times as the all-core baseline) against the
    serial build on a small GOF: frames in parallel, points / voxels in parallel inside a frame, same bytes."""
    import oracle_binding as ob
    if not os.path.exists(ob.REF_TBB_PATH):
        pytest.skip("oracle/_ref/libtmc2ref_tbb.so not built")
    from tmc2_amd.synth import synth_cloud
    frames = [synth_cloud("tiny", f) for f in range(3)]
    par = ob.Reference(tbb=True, nb_thread=4)
    a1, a4 = reference.phase_a(frames, 4, 11, 4), None
    b1 = reference.phase_b(frames, a1, 4)
    a4 = par.phase_a(frames, 4, 11, 4)
    b4 = par.phase_b(frames, a4, 4)
    for x, y in zip(a1, a4):
        assert all(np.array_equal(x[k], y[k]) for k in ("occupancy", "occ_video", "block_to_patch", "geo0", "geo1"))
    for x, y in zip(b1, b4):
        assert all(np.array_equal(x[k], y[k]) for k in ("recon_xyz", "recon_rgb", "point_to_pixel", "attribute"))


def test_gof_encoder_without_a_device_fails_instead_of_waiting():
    """A worker whose context cannot be created (here: no HIP device) hands the error to the constructor; before round 4's
    end the thread died with it and `GofEncoder( .. )` -- and `python bench.py` on a box without a GPU -- waited for ever."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible")
    import threading
    result = []

    def make():
        try:
            T.GofEncoder(0, 2, 3, 11, 4, 256, 256)
            result.append("made")
        except T.Tmc2Error as e:
            result.append(str(e))
    w = threading.Thread(target=make, daemon=True)
    w.start()
    w.join(60)
    assert not w.is_alive(), "GofEncoder() is still waiting for a worker that died"
    assert result and "no HIP device" in result[0]


def test_host_gate_is_an_object_of_the_caller():
    """tmc2_host_gate_create / tmc2_host_gate_destroy / tmc2_ctx_set_host_gate (round 6: an encoder's own budget of host-resident
    steps instead of one process-wide count): argument errors without a device."""
    import ctypes as C
    L = T.load_library()
    g = C.c_void_p()
    assert L.tmc2_host_gate_create(4, C.byref(g)) == 0 and g.value
    assert L.tmc2_host_gate_create(-1, C.byref(g)) != 0
    assert L.tmc2_host_gate_create(0, None) != 0
    assert L.tmc2_ctx_set_host_gate(None, g) != 0 and b"invalid argument" in L.tmc2_last_error()
    L.tmc2_host_gate_destroy(g)
    L.tmc2_host_gate_destroy(g)                                # (twice: harmless)
    L.tmc2_host_gate_destroy(None)
