"""ctypes binding of libtmc2hip.so (include/tmc2hip.h).  Class/method names mirror the reference's
seams: Frame.normals_compute <-> PCCNormalsGenerator3::compute, Frame.segmenter_* <-> PCCPatchSegmenter3::*,
Frame.kdtree_search <-> PCCKdTree::search."""
import ctypes as C
import dataclasses
import os as _os

# One HIP stream per in-flight frame (32 per GPU in a GOF run): the runtime multiplexes streams onto 4 hardware queues by
# default, and a queue is held by whatever kernel is at its head (e.g. a 140 us single-workgroup closure tail).  Must be
# set before the HIP runtime initialises; an explicit setting of the user wins.
_os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")
import os
import re
import threading
import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None


def library_path():
    return os.path.normpath(os.path.join(_HERE, "..", "libtmc2hip.so"))


class Tmc2Error(RuntimeError):
    pass


class SegmenterParams(C.Structure):
    """Mirror of tmc2_segmenter_params (PCCPatchSegmenter3Parameters, PCCPatchSegmenter.h:48-100)."""
    _fields_ = [(n, C.c_int32) for n in (
        "nnNormalEstimation", "normalOrientation", "gridBasedRefineSegmentation", "maxNNCountRefineSegmentation",
        "iterationCountRefineSegmentation", "voxelDimensionRefineSegmentation", "searchRadiusRefineSegmentation",
        "occupancyResolution", "enablePatchSplitting", "maxPatchSize", "quantizerSizeX", "quantizerSizeY",
        "minPointCountPerCCPatchSegmentation", "maxNNCountPatchSegmentation", "surfaceThickness", "mapCountMinus1",
        "minLevel", "maxAllowedDepth", "geometryBitDepth2D", "geometryBitDepth3D")] + [
        ("maxAllowedDist2RawPointsDetection", C.c_double), ("maxAllowedDist2RawPointsSelection", C.c_double),
        ("lambdaRefineSegmentation", C.c_double), ("weightNormal", C.c_double * 3)]


class Patch(C.Structure):
    """Mirror of tmc2_patch (PCCPatch fields produced by the hot path)."""
    _fields_ = [(n, C.c_int32) for n in (
        "index", "viewId", "normalAxis", "tangentAxis", "bitangentAxis", "projectionMode", "u1", "v1", "d1", "sizeU",
        "sizeV", "sizeD", "sizeDPixel", "sizeU0", "sizeV0", "size2DXInPixel", "size2DYInPixel", "d0Count",
        "eomAndD1Count", "u0", "v0", "patchOrientation")] + [("depthOffset", C.c_int64), ("occOffset", C.c_int64)]


PATCH_DTYPE = np.dtype(Patch._fields_)


class _MetricsParamsStruct(C.Structure):
    """Mirror of tmc2_metrics_params."""
    _fields_ = [(n, C.c_int32) for n in ("computeC2c", "computeC2p", "computeColor", "computeHausdorff", "dropDuplicates", "neighborsProc")]


@dataclasses.dataclass(frozen=True)
class MetricsParams:
    """The switches of PCCMetricsParameters that PccAppMetrics takes (tmc2_metrics_params; the defaults are the reference's):
    drop_duplicates 0 keep / 1 first colour / 2 mean colour; neighbors_proc 0 first result / 1, 2 mean / 3, 4 "min" / "max" as the
    reference is written (include/tmc2hip.h)."""
    compute_c2c: bool = True
    compute_c2p: bool = True
    compute_color: bool = True
    compute_hausdorff: bool = False
    drop_duplicates: int = 2
    neighbors_proc: int = 1

    def struct(self):
        return _MetricsParamsStruct(int(self.compute_c2c), int(self.compute_c2p), int(self.compute_color), int(self.compute_hausdorff),
                                    int(self.drop_duplicates), int(self.neighbors_proc))


class _ColorTransferParamsStruct(C.Structure):
    """Mirror of tmc2_color_transfer_params."""
    _fields_ = [(n, C.c_int32) for n in (
        "searchRange", "losslessAttribute", "numNeighborsColorTransferFwd", "numNeighborsColorTransferBwd", "useDistWeightedAverageFwd",
        "useDistWeightedAverageBwd", "skipAvgIfIdenticalSourcePointPresentFwd", "skipAvgIfIdenticalSourcePointPresentBwd")] + [
        (n, C.c_double) for n in ("distOffsetFwd", "distOffsetBwd", "maxGeometryDist2Fwd", "maxGeometryDist2Bwd", "maxColorDist2Fwd",
                                  "maxColorDist2Bwd")] + [("excludeColorOutlier", C.c_int32), ("thresholdColorOutlierDist", C.c_double)]


@dataclasses.dataclass(frozen=True)
class ColorTransferParams:
    """The arguments of PCCPointSet3::transferColors in its order (tmc2_color_transfer_params).  The defaults are the CTC point, what
    the entries without a parameter set compute; PCCEncoderParameters' own defaults differ (1 forward neighbour, no skip flags, offsets
    0.0001, thresholds 10000)."""
    search_range: int = 0
    lossless_attribute: bool = False
    num_neighbors_fwd: int = 8
    num_neighbors_bwd: int = 1
    use_dist_weighted_average_fwd: bool = True
    use_dist_weighted_average_bwd: bool = True
    skip_avg_if_identical_source_point_present_fwd: bool = True
    skip_avg_if_identical_source_point_present_bwd: bool = True
    dist_offset_fwd: float = 4.0
    dist_offset_bwd: float = 4.0
    max_geometry_dist2_fwd: float = 1000.0
    max_geometry_dist2_bwd: float = 1000.0
    max_color_dist2_fwd: float = 1000.0
    max_color_dist2_bwd: float = 1000.0
    exclude_color_outlier: bool = False
    threshold_color_outlier_dist: float = 10.0

    def struct(self):
        v = dataclasses.astuple(self)
        return _ColorTransferParamsStruct(*([int(x) for x in v[:8]] + [float(x) for x in v[8:14]] + [int(v[14]), float(v[15])]))


def color_transfer_params_check(params):
    """tmc2_color_transfer_params_check: raises Tmc2Error naming the field the transfer refuses (no device needed)."""
    _check(load_library().tmc2_color_transfer_params_check(C.byref(params.struct())))


def host_transfer_colors(src_xyz, src_rgb, tgt_xyz, params=None):
    """tmc2_host_transfer_colors: PCCPointSet3::transferColors restated on the host (no device) -> the target's colours [m][3]."""
    a = np.ascontiguousarray(src_xyz, np.int16).reshape(-1, 3)
    b = np.ascontiguousarray(src_rgb, np.uint8).reshape(-1, 3)
    c = np.ascontiguousarray(tgt_xyz, np.int16).reshape(-1, 3)
    if a.shape != b.shape:
        raise Tmc2Error("host_transfer_colors: %d source points, %d source colours" % (len(a), len(b)))
    out = np.zeros((len(c), 3), np.uint8)
    st = (params or ColorTransferParams()).struct()
    _check(load_library().tmc2_host_transfer_colors(_ptr(a), _ptr(b), len(a), _ptr(c), len(c), C.byref(st), _ptr(out)))
    return out


def ctc_params(iterations=10, bits3d=11, weight=(1.0, 1.0, 1.0), vox_dim=4):
    """CTC lossy settings (cfg/common/ctc-common.cfg + sequence cfg).  Per sequence: iterations 50
    (longdress), 20 (basketball_player), 10 (the others); vox_dim = voxelDimensionRefineSegmentation: 4, but 2 for loot,
    redandblack and soldier."""
    p = SegmenterParams()
    p.nnNormalEstimation = 16
    p.normalOrientation = 1
    p.gridBasedRefineSegmentation = 1
    p.maxNNCountRefineSegmentation = 1024
    p.iterationCountRefineSegmentation = iterations
    p.voxelDimensionRefineSegmentation = vox_dim
    p.searchRadiusRefineSegmentation = 192
    p.occupancyResolution = 16
    p.enablePatchSplitting = 1
    p.maxPatchSize = 1024
    p.quantizerSizeX = 16
    p.quantizerSizeY = 16
    p.minPointCountPerCCPatchSegmentation = 16
    p.maxNNCountPatchSegmentation = 16
    p.surfaceThickness = 4
    p.mapCountMinus1 = 1
    p.minLevel = 64
    p.maxAllowedDepth = 255
    p.geometryBitDepth2D = 8
    p.geometryBitDepth3D = bits3d
    p.maxAllowedDist2RawPointsDetection = 9.0
    p.maxAllowedDist2RawPointsSelection = 1.0
    p.lambdaRefineSegmentation = 3.0
    p.weightNormal[0], p.weightNormal[1], p.weightNormal[2] = weight
    return p


def fast_params(iterations=5, bits3d=11, weight=(1.0, 1.0, 1.0)):
    """The CTC settings with the defaults the reference takes when gridBasedSegmentation is set (PCCEncoderParameters.cpp:64-67):
    maxNNCountRefineSegmentation 384, iterationCountRefineSegmentation 5, voxelDimensionRefineSegmentation 2,
    searchRadiusRefineSegmentation 128 -- for Frame.segmenter_compute( params, grid_based = voxDim )."""
    p = ctc_params(iterations, bits3d, weight, vox_dim=2)
    p.maxNNCountRefineSegmentation = 384
    p.searchRadiusRefineSegmentation = 128
    return p


def knn_refine_params(iterations=100, bits3d=11, weight=(1.0, 1.0, 1.0)):
    """The CTC settings with gridBasedRefineSegmentation off and the defaults the reference takes then: maxNNCountRefineSegmentation
    256, iterationCountRefineSegmentation 100 -- for Frame.segmenter_compute( params[, grid_based = voxDim] ), which goes to the k-NN
    refinement (PCCPatchSegmenter3::refineSegmentation).  The refinement's voxel size and search radius are not read."""
    p = ctc_params(iterations, bits3d, weight)
    p.gridBasedRefineSegmentation = 0
    p.maxNNCountRefineSegmentation = 256
    return p


# TMC2_GUARD=1 (tests, bench.py --guard): every array handed to the C-ABI travels in a copy with a red zone of _GUARD bytes on
# both sides, filled with a pattern; after the call (_check) the zones are verified -- the library wrote outside a buffer of the
# caller's iff they changed -- and the payload is copied back.  Calls are synchronous on host buffers (the getters end with a
# stream synchronisation), so the copy-back sees the final bytes.  Costs a copy per argument: a debugging aid, not a mode to time.
_GUARD = 4096
_guard_on = os.environ.get("TMC2_GUARD", "0") == "1"
_guard_tls = threading.local()


def set_guard(on):
    global _guard_on
    _guard_on = bool(on)


def _ptr(a):
    if not _guard_on or a.nbytes == 0:
        return a.ctypes.data_as(C.c_void_p)
    if not a.flags["C_CONTIGUOUS"]:
        raise Tmc2Error("guard mode: array handed to the C-ABI is not contiguous")
    g = np.full(a.nbytes + 2 * _GUARD, 0xA5, np.uint8)
    g[_GUARD:_GUARD + a.nbytes] = a.reshape(-1).view(np.uint8)
    if not hasattr(_guard_tls, "pending"):
        _guard_tls.pending = []
    _guard_tls.pending.append((a, g))
    return C.c_void_p(g.ctypes.data + _GUARD)


def _guard_finish():
    pending, _guard_tls.pending = getattr(_guard_tls, "pending", []), []
    for a, g in pending:
        n = a.nbytes
        lo, hi = g[:_GUARD], g[_GUARD + n:]
        if (lo != 0xA5).any() or (hi != 0xA5).any():
            before, after = int((lo != 0xA5).sum()), int((hi != 0xA5).sum())
            first = int(np.argmax(hi != 0xA5)) if after else -1
            raise Tmc2Error("guard mode: the library wrote outside a caller's buffer (%s %s, %d bytes): %d bytes changed before it, "
                            "%d after it (first at +%d)" % (a.dtype, a.shape, n, before, after, first))
        if a.flags["WRITEABLE"]:
            a.reshape(-1).view(np.uint8)[:] = g[_GUARD:_GUARD + n]


# The C-ABI as ctypes has to be told it: TMC2HIP (at the end of this file) has one row per function of include/tmc2hip.h, in the
# header's order and spelling, parameter names dropped (native_gof.TMC2GOF: include/tmc2gof.h).  Without a prototype every Python int
# travels as a 32-bit C int and every return value is read as one: wrong for each uint64_t / int64_t / size_t / double.  A new entry
# point gets a row; tests/test_host_logic.py compares the rows, and what declare() installed, with the headers -- which a copy of
# the package away from the repository cannot read: hence a table.
# The one mapping rule: scalars by their exact width; `const char*` is c_char_p; every other pointer -- handles, out-parameters,
# arrays such as `double[3]`, struct pointers, a returned `void*` -- is c_void_p, which takes None, byref(x), a ctypes array, a
# c_void_p, a plain address and bytes; a function that returns void has restype None.
_SCALARS = {"void": None, "int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "uint64_t": C.c_uint64, "size_t": C.c_size_t,
            "long": C.c_long, "double": C.c_double}


def _ctype(c_type):
    if c_type == "const char*":
        return C.c_char_p
    return C.c_void_p if c_type[-1] in "*]" else _SCALARS[c_type]


def declare(handle, rows):
    """Install the prototypes of `rows` on a CDLL handle (a function the library does not export is an AttributeError)."""
    for row in rows:
        ret, name, params = re.fullmatch(r"(.+?) (tmc2_\w+)\((.*)\)", row).groups()
        fn = getattr(handle, name)
        fn.restype = _ctype(ret)
        fn.argtypes = [] if params == "void" else [_ctype(t) for t in params.split(", ")]
    return handle


def load_library():
    """Load libtmc2hip.so; raises if it has not been built (no silent fallback)."""
    global _LIB
    if _LIB is not None:
        return _LIB
    path = library_path()
    if not os.path.exists(path):
        raise Tmc2Error("libtmc2hip.so not built: run `python __graft_entry__.py build` (hipcc, gfx950)")
    _LIB = declare(C.CDLL(path), TMC2HIP)
    return _LIB


def _check(rc):
    if _guard_on:
        _guard_finish()
    if rc != 0:
        raise Tmc2Error("tmc2hip error %d: %s" % (rc, load_library().tmc2_last_error().decode()))


class HostGate:
    """One encoder's budget of concurrently running host-resident steps (tmc2_host_gate_create): shared by the contexts it is set
    on (Context.set_host_gate) and by nobody else -- two encoders of one process do not draw on one process-wide count."""

    def __init__(self, limit):
        self.L = load_library()
        self.h = C.c_void_p()
        _check(self.L.tmc2_host_gate_create(int(limit), C.byref(self.h)))

    def close(self):
        if self.h:
            self.L.tmc2_host_gate_destroy(self.h)       # (contexts that still hold the gate keep it alive)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Context:
    def __init__(self, device=0):
        self.L = load_library()
        self.h = C.c_void_p()
        _check(self.L.tmc2_ctx_create(int(device), C.byref(self.h)))

    def close(self):
        if self.h:
            self.L.tmc2_ctx_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def synchronize(self):
        _check(self.L.tmc2_ctx_synchronize(self.h))

    def set_option(self, key, value):
        """Per-context option (include/tmc2hip.h: tmc2_ctx_set_option); value None unsets it.  A context starts with the TMC2_*
        variables of the environment it was created in."""
        _check(self.L.tmc2_ctx_set_option(self.h, key.encode(), None if value is None else str(value).encode()))

    def get_option(self, key):
        v = self.L.tmc2_ctx_get_option(self.h, key.encode())
        return None if v is None else v.decode()

    def set_host_gate(self, gate):
        """This context's host-resident steps wait at `gate` (a HostGate; None: the process' default gate again)."""
        _check(self.L.tmc2_ctx_set_host_gate(self.h, None if gate is None else gate.h))

    def reserve(self, max_points, vox_dim, bits3d, max_w, max_h):
        """tmc2_ctx_reserve: the device memory of the sequence's largest frame, allocated now (no first-use hipMalloc later)."""
        _check(self.L.tmc2_ctx_reserve(self.h, int(max_points), int(vox_dim), int(bits3d), int(max_w), int(max_h)))

    # device staging (what libtmc2gof.so's RCCL mode uses between its collectives): raw device memory of this context's device,
    # copies ordered on its stream
    def device_alloc(self, nbytes):
        p = C.c_void_p()
        _check(self.L.tmc2_ctx_device_alloc(self.h, int(nbytes), C.byref(p)))
        return p

    def device_free(self, p):
        _check(self.L.tmc2_ctx_device_free(self.h, p))

    def upload(self, device_ptr, array):
        a = np.ascontiguousarray(array)
        _check(self.L.tmc2_ctx_upload(self.h, device_ptr, _ptr(a), a.nbytes))

    def download(self, array, device_ptr):
        _check(self.L.tmc2_ctx_download(self.h, _ptr(array), device_ptr, array.nbytes))
        return array


    # The shared device primitives on their own (include/tmc2hip.h: tmc2_selftest_*; csrc/selftest.hip).  Device pointers in
    # (device_alloc / upload / download), queued on the context's stream, not waited for.
    def selftest_scan(self, d_in, d_out, n, d_total=None, host_answer=None, d_carry=None, carry_words=0, epoch=0):
        _check(self.L.tmc2_selftest_scan(self.h, d_in, d_out, int(n), d_total, host_answer, d_carry, int(carry_words), int(epoch)))

    def selftest_fill(self, regions):
        """regions: (device address, bytes, byte value) each"""
        r = np.ascontiguousarray([[int(getattr(p, "value", p) or 0), int(b), int(v)] for p, b, v in regions], dtype=np.uint64).reshape(-1, 3)
        _check(self.L.tmc2_selftest_fill(self.h, _ptr(r) if len(r) else None, len(r)))

    def selftest_work_map(self, grid_blocks, block_threads, n, live_blocks, d_hits, d_logical):
        _check(self.L.tmc2_selftest_work_map(self.h, int(grid_blocks), int(block_threads), int(n), int(live_blocks), d_hits, d_logical))

    def selftest_components(self, d_knn, d_partition, d_raw, d_perm, n, d_root, d_bad):
        _check(self.L.tmc2_selftest_components(self.h, d_knn, d_partition, d_raw, d_perm, int(n), d_root, d_bad))

    def selftest_union_find(self, parity, d_word, n, d_edges, m, precheck, agent, d_root, d_root_parity, d_bad):
        _check(self.L.tmc2_selftest_union_find(self.h, int(parity), d_word, int(n), d_edges, int(m), int(precheck), int(agent), d_root,
                                               d_root_parity, d_bad))

    def selftest_cand_sort(self, d_lists, d_offsets, lists, d_ok):
        _check(self.L.tmc2_selftest_cand_sort(self.h, d_lists, d_offsets, int(lists), d_ok))

    def selftest_marked_cells(self, d_xyz4, d_boundary_type, m, grid_size, bits=0, max_coord=0, d_bits=None, d_rank=None, d_keys=None,
                              keys=0, d_slots=None):
        """the number of marked cells (this one waits for it); bits != 0: the cube of 2^bits, else the grid over [0, max_coord]"""
        cells = C.c_uint32(0)
        _check(self.L.tmc2_selftest_marked_cells(self.h, d_xyz4, d_boundary_type, int(m), int(grid_size), int(bits), int(max_coord),
                                                 C.byref(cells), d_bits, d_rank, d_keys, int(keys), d_slots))
        return cells.value

    def selftest_wave(self, op, param, d_in, d_out, n, d_aux=None):
        """one idiom of csrc/wave.h per call (include/tmc2hip.h: the op codes)"""
        _check(self.L.tmc2_selftest_wave(self.h, int(op), int(param), d_in, d_out, d_aux, int(n)))

    def selftest_pool_probe(self, nbytes):
        """the whole size class of a pool block of nbytes as the pool hands it out, unwritten (option POOL_POISON); this one waits"""
        cls = C.c_uint64(0)
        _check(self.L.tmc2_selftest_pool_probe(self.h, int(nbytes), None, C.byref(cls)))
        out = np.empty(cls.value, np.uint8)
        _check(self.L.tmc2_selftest_pool_probe(self.h, int(nbytes), _ptr(out), C.byref(cls)))
        return out

    def selftest_pool_poisoned(self):
        """blocks this context's pool has filled with the poison byte so far"""
        blocks = C.c_uint64(0)
        _check(self.L.tmc2_selftest_pool_poisoned(self.h, C.byref(blocks)))
        return blocks.value

    def stream(self):
        return self.L.tmc2_ctx_stream(self.h)

    def device(self):
        return int(self.L.tmc2_ctx_device(self.h))

    def make_current(self):
        _check(self.L.tmc2_ctx_make_current(self.h))

    def pool_stats(self):
        held, calls, carved, ms = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_double()
        _check(self.L.tmc2_ctx_pool_stats(self.h, C.byref(held), C.byref(calls), C.byref(ms), C.byref(carved)))
        return {"bytes_held": held.value, "hipmalloc_calls": calls.value, "hipmalloc_ms": ms.value, "carved_blocks": carved.value}

    def stage_ms(self):
        return {self.L.tmc2_ctx_stage_name(self.h, i).decode(): self.L.tmc2_ctx_stage_ms(self.h, i)
                for i in range(self.L.tmc2_ctx_stage_count(self.h))}

    def stage_calls(self):
        return {self.L.tmc2_ctx_stage_name(self.h, i).decode(): self.L.tmc2_ctx_stage_calls(self.h, i)
                for i in range(self.L.tmc2_ctx_stage_count(self.h))}

    def stage_reset(self):
        self.L.tmc2_ctx_stage_reset(self.h)

    def set_timing(self, enabled):
        self.L.tmc2_ctx_set_timing(self.h, 1 if enabled else 0)

    def frame(self, xyz, rgb=None):
        return Frame(self, xyz, rgb)

    # PCCPointSet3::transferColors
    def transfer_colors(self, src_xyz, src_rgb, tgt_xyz, params=None):
        """params = ColorTransferParams: tmc2_transfer_colors_ex; None: the CTC point (tmc2_transfer_colors)."""
        a = np.ascontiguousarray(src_xyz, np.int16)
        b = np.ascontiguousarray(src_rgb, np.uint8)
        c = np.ascontiguousarray(tgt_xyz, np.int16)
        if a.shape != b.shape:                                    # (the C entry takes ONE count for both: a short colour array is read past its end)
            raise Tmc2Error("transfer_colors: %d source points, %d source colours" % (len(a), len(b)))
        out = np.zeros((len(c), 3), np.uint8)
        if params is None:
            _check(self.L.tmc2_transfer_colors(self.h, _ptr(a), _ptr(b), len(a), _ptr(c), len(c), _ptr(out)))
        else:
            _check(self.L.tmc2_transfer_colors_ex(self.h, _ptr(a), _ptr(b), len(a), _ptr(c), len(c), C.byref(params.struct()), _ptr(out)))
        return out

    # PCCPatchSegmenter3::convertPointsToVoxels
    def convert_points_to_voxels(self, xyz, vox_dim, bits3d):
        """tmc2_segmenter_convert_points_to_voxels on a host cloud -> (voxel positions [V][3] in first-occurrence order, the rank of
        every point's voxel [n])."""
        a = np.ascontiguousarray(xyz, np.int16).reshape(-1, 3)
        vox, rank, count = np.zeros((len(a), 3), np.int16), np.zeros(len(a), np.uint32), C.c_uint64()
        _check(self.L.tmc2_segmenter_convert_points_to_voxels(self.h, _ptr(a), len(a), int(vox_dim), int(bits3d), _ptr(vox), C.byref(count),
                                                              _ptr(rank)))
        return vox[:count.value].copy(), rank

    # PCCCodec::colorSmoothing
    def color_smoothing(self, xyz, colors16, boundary, patch_index, grid_size, bits3d, thr_smoothing=10.0, thr_difference=10.0,
                        thr_variation=6.0):
        """tmc2_color_smoothing on host arrays: the smoothed 16-bit colours (a copy)."""
        a = _color_smoothing_arrays(xyz, colors16, boundary, patch_index)
        _check(self.L.tmc2_color_smoothing(self.h, _ptr(a[0]), _ptr(a[1]), _ptr(a[2]), _ptr(a[3]), len(a[0]), int(grid_size),
                                          int(bits3d), thr_smoothing, thr_difference, thr_variation))
        return a[1]

    # PCCMetrics::compute (one frame)
    def decoder_frame(self, patches, width, height, occ_precision, occ_video, geometry):
        """A frame without a source cloud: decoded patch records (list order), occupancy video, geometry maps [2][H][W]."""
        pt = np.ascontiguousarray(patches, dtype=PATCH_DTYPE)
        ov = np.ascontiguousarray(occ_video, dtype=np.uint8)
        geo = np.ascontiguousarray(geometry, dtype=np.uint16)
        if ov.shape != (height // occ_precision, width // occ_precision) or geo.shape != (2, height, width):
            raise ValueError("decoded canvases do not match %dx%d at precision %d" % (width, height, occ_precision))
        fr = Frame.__new__(Frame)
        fr.L, fr.ctx, fr.h = self.L, self, C.c_void_p()
        fr._xyz, fr._rgb, fr.n = None, None, 0
        _check(self.L.tmc2_decoder_frame_create(self.h, _ptr(pt), len(pt), int(width), int(height), int(occ_precision), _ptr(ov),
                                               _ptr(geo), C.byref(fr.h)))
        fr._canvas = (int(width), int(height), int(occ_precision))
        return fr

    # PCCInternalColorConverter (the attribute video's colour-space conversion)
    def color_convert_rgb444_to_yuv420(self, rgb, downsampling_filter=4):
        """rgb uint8 [3][H][W] -> (y [H][W], u, v [H/2][W/2])"""
        rgb = np.ascontiguousarray(rgb, dtype=np.uint8)
        _, H, W = rgb.shape
        out = np.zeros(W * H * 3 // 2, np.uint8)
        _check(self.L.tmc2_color_convert_rgb444_to_yuv420(self.h, _ptr(rgb), int(W), int(H), int(downsampling_filter), _ptr(out)))
        a = W * H
        return out[:a].reshape(H, W), out[a:a + a // 4].reshape(H // 2, W // 2), out[a + a // 4:].reshape(H // 2, W // 2)

    def color_convert_yuv420_to_yuv444(self, y, u, v, upsampling_filter=0):
        """-> uint16 [3][H][W]"""
        H, W = y.shape
        src = np.concatenate([np.ascontiguousarray(a, dtype=np.uint8).reshape(-1) for a in (y, u, v)])
        out = np.zeros((3, H, W), np.uint16)
        _check(self.L.tmc2_color_convert_yuv420_to_yuv444(self.h, _ptr(src), int(W), int(H), int(upsampling_filter), _ptr(out)))
        return out

    def metrics_compute(self, src_xyz, src_rgb, rec_xyz, rec_rgb, normals=None, resolution=1023.0, params=None):
        """(q[3][8], counts[2]) with the defaults of PCCMetricsParameters; params = MetricsParams: q[3][14] (tmc2_metrics_compute_ex)."""
        a = np.ascontiguousarray(src_xyz, np.int16)
        b = np.ascontiguousarray(src_rgb, np.uint8)
        c = np.ascontiguousarray(rec_xyz, np.int16)
        d = np.ascontiguousarray(rec_rgb, np.uint8)
        nm = None if normals is None else np.ascontiguousarray(normals, np.float64)
        out = np.zeros((3, 8 if params is None else 14), np.float64)
        counts = np.zeros(2, np.int64)
        if params is None:
            _check(self.L.tmc2_metrics_compute(self.h, _ptr(a), _ptr(b), len(a), _ptr(c), _ptr(d), len(c),
                                               None if nm is None else _ptr(nm), resolution, _ptr(out), _ptr(counts)))
        else:
            _check(self.L.tmc2_metrics_compute_ex(self.h, _ptr(a), _ptr(b), len(a), _ptr(c), _ptr(d), len(c),
                                                  None if nm is None else _ptr(nm), resolution, C.byref(params.struct()), _ptr(out), _ptr(counts)))
        return out, counts

    def metrics_ordered_sums(self, terms_a, terms_b):
        """The ordered sums of per-point terms [n][5] (tmc2_metrics_ordered_sums): out[10], five per direction."""
        a = np.ascontiguousarray(terms_a, np.float64).reshape(-1, 5)
        b = np.ascontiguousarray(terms_b, np.float64).reshape(-1, 5)
        out = np.zeros(10, np.float64)
        _check(self.L.tmc2_metrics_ordered_sums(self.h, _ptr(a) if len(a) else None, len(a), _ptr(b) if len(b) else None, len(b), _ptr(out)))
        return out


class Frame:
    """Device-resident state of one point-cloud frame (tmc2_frame)."""

    def __init__(self, ctx, xyz, rgb=None):
        self.ctx, self.L = ctx, ctx.L
        xyz = np.ascontiguousarray(xyz, dtype=np.int16)
        assert xyz.ndim == 2 and xyz.shape[1] == 3
        self.n = len(xyz)
        self._xyz = xyz
        self._rgb = None if rgb is None else np.ascontiguousarray(rgb, dtype=np.uint8)
        self.h = C.c_void_p()
        _check(self.L.tmc2_frame_create(ctx.h, _ptr(xyz), None if rgb is None else _ptr(self._rgb), self.n, C.byref(self.h)))

    def close(self):
        if self.h:
            self.L.tmc2_frame_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset(self):
        _check(self.L.tmc2_frame_reset(self.h))

    def metrics_compute(self, which=0, use_normals=True, resolution=1023.0, params=None):
        """S23 on the frame's resident clouds (nothing is uploaded): source = the frame, reconstruction = which 0: the cloud of
        the attribute-image step, 1: the finished cloud of the post-reconstruction tail.  Returns (q[3][8], counts[2]); with
        params = MetricsParams (q[3][14], counts[2]) (tmc2_metrics_compute_frame_ex)."""
        out = np.zeros((3, 8 if params is None else 14), np.float64)
        counts = np.zeros(2, np.int64)
        if params is None:
            _check(self.L.tmc2_metrics_compute_frame(self.h, which, 1 if use_normals else 0, resolution, _ptr(out), _ptr(counts)))
        else:
            _check(self.L.tmc2_metrics_compute_frame_ex(self.h, which, 1 if use_normals else 0, resolution, C.byref(params.struct()), _ptr(out),
                                                        _ptr(counts)))
        return out, counts

    def metrics_compute_source(self, src_xyz, src_rgb, normals=None, which=1, resolution=1023.0, params=None):
        """S23 of a source cloud held on the host against this frame's resident reconstruction (the decoder side); params as above."""
        a = np.ascontiguousarray(src_xyz, np.int16)
        b = np.ascontiguousarray(src_rgb, np.uint8)
        nm = None if normals is None else np.ascontiguousarray(normals, np.float64)
        out = np.zeros((3, 8 if params is None else 14), np.float64)
        counts = np.zeros(2, np.int64)
        if params is None:
            _check(self.L.tmc2_metrics_compute_frame_source(self.h, which, _ptr(a), _ptr(b), len(a),
                                                            None if nm is None else _ptr(nm), resolution, _ptr(out), _ptr(counts)))
        else:
            _check(self.L.tmc2_metrics_compute_frame_source_ex(self.h, which, _ptr(a), _ptr(b), len(a), None if nm is None else _ptr(nm),
                                                               resolution, C.byref(params.struct()), _ptr(out), _ptr(counts)))
        return out, counts

    def kdtree_build(self):
        _check(self.L.tmc2_kdtree_build(self.h))

    def kdtree_order(self):
        """(perm, depth): the permutation the tree build leaves behind (tree order -> point index) and the levels."""
        perm = np.empty(self.n, np.uint32)
        depth = C.c_int32()
        _check(self.L.tmc2_frame_get_kdtree_order(self.h, _ptr(perm), C.byref(depth)))
        return perm, depth.value

    def device_images(self):
        """Device addresses + shapes of the canvases (for RCCL hand-off): dict name -> (ptr, shape, typestr)."""
        W, H, p = self._canvas
        ptrs = [C.c_void_p() for _ in range(4)]
        _check(self.L.tmc2_frame_device_images(self.h, *[C.byref(x) for x in ptrs]))
        out = dict(occupancy=(ptrs[0].value, (H, W), "|u1"), occ_video=(ptrs[1].value, (H // p, W // p), "|u1"),
                   block_to_patch=(ptrs[2].value, (H // 16, W // 16), "<u4"), geometry=(ptrs[3].value, (2, H, W), "<u2"))
        a = C.c_void_p()
        if self.L.tmc2_frame_device_attribute(self.h, C.byref(a)) == 0:
            out["attribute"] = (a.value, (2, 3, H, W), "|u1")
        return out

    # PCCKdTree::search
    def kdtree_search(self, queries, k, with_dist=False):
        q = np.ascontiguousarray(queries, dtype=np.int16)
        idx = np.empty((len(q), k), np.uint32)
        d = np.empty((len(q), k), np.uint32) if with_dist else None
        _check(self.L.tmc2_kdtree_search(self.h, _ptr(q), len(q), int(k), _ptr(idx), None if d is None else _ptr(d)))
        return (idx, d) if with_dist else idx

    def kdtree_search_wide(self, k, queries=None):
        """tmc2_kdtree_search_wide: the k (1..1024) results of nanoflann's search per query as a SET (the order inside a row is
        unspecified), by the wave-per-query kernel; queries None: the frame's own points, row i = point i."""
        q = None if queries is None else np.ascontiguousarray(queries, dtype=np.int16).reshape(-1, 3)
        nq = self.n if q is None else len(q)
        idx = np.empty((nq, max(int(k), 0) if int(k) <= 1024 else 0), np.uint32)
        _check(self.L.tmc2_kdtree_search_wide(self.h, None if q is None else _ptr(q), nq, int(k), _ptr(idx)))
        return idx

    # PCCNormalsGenerator3
    def normals_compute_normals(self, k=16):
        _check(self.L.tmc2_normals_compute_normals(self.h, int(k)))

    def normals_orient(self):
        _check(self.L.tmc2_normals_orient(self.h))

    def normals_compute(self, k=16, orientation=1):
        _check(self.L.tmc2_normals_compute(self.h, int(k), int(orientation)))

    def get_normals(self):
        out = np.empty((self.n, 3), np.float64)
        _check(self.L.tmc2_frame_get_normals(self.h, _ptr(out)))
        return out

    def set_normals(self, normals):
        a = np.ascontiguousarray(normals, dtype=np.float64)
        _check(self.L.tmc2_frame_set_normals(self.h, _ptr(a)))

    def get_adjacency(self, k=16):
        out = np.empty((self.n, k), np.uint32)
        _check(self.L.tmc2_frame_get_adjacency(self.h, _ptr(out)))
        return out

    # PCCEncoder::calculateWeightNormal
    def weight_normal(self, bits3d=11, min_weight_epp=0.6):
        w = (C.c_double * 3)()
        _check(self.L.tmc2_weight_normal(self.h, int(bits3d), min_weight_epp, w))
        return np.array([w[0], w[1], w[2]])

    # PCCPatchSegmenter3
    def segmenter_initial_segmentation(self, weight):
        w = (C.c_double * 3)(*[float(x) for x in weight])
        _check(self.L.tmc2_segmenter_initial_segmentation(self.h, w))

    def segmenter_refine_grid_based(self, max_nn=1024, lam=3.0, iterations=10, vox_dim=4, radius=192):
        _check(self.L.tmc2_segmenter_refine_grid_based(self.h, int(max_nn), lam, int(iterations), int(vox_dim), int(radius)))

    def segmenter_refine(self, max_nn=256, lam=3.0, iterations=100):
        """PCCPatchSegmenter3::refineSegmentation on the frame's normals and partition: max_nn nearest neighbours, Jacobi rounds."""
        _check(self.L.tmc2_segmenter_refine(self.h, int(max_nn), lam, int(iterations)))

    def get_partition(self):
        out = np.empty(self.n, np.uint32)
        _check(self.L.tmc2_frame_get_partition(self.h, _ptr(out)))
        return out

    def set_partition(self, partition):
        a = np.ascontiguousarray(partition, dtype=np.uint32)
        _check(self.L.tmc2_frame_set_partition(self.h, _ptr(a)))

    def segmenter_segment_patches(self, params):
        _check(self.L.tmc2_segmenter_segment_patches(self.h, C.byref(params)))

    def segmenter_compute(self, params, grid_based=None):
        """PCCPatchSegmenter3::compute; grid_based = voxelDimensionGridBasedSegmentation (2, 4 or 8): the reference's fast mode --
        S1-S5 on the voxel cloud, partition and normals copied back, tree / adjacency / patches on the full cloud.
        params.gridBasedRefineSegmentation == 0 (knn_refine_params): the refinement over k-NN neighbourhoods, on the cloud or, with
        grid_based, on the voxel cloud (tmc2_segmenter_compute_knn_refine)."""
        if not params.gridBasedRefineSegmentation:
            _check(self.L.tmc2_segmenter_compute_knn_refine(self.h, C.byref(params), 0 if grid_based is None else int(grid_based)))
        elif grid_based is None:
            _check(self.L.tmc2_segmenter_compute(self.h, C.byref(params)))
        else:
            _check(self.L.tmc2_segmenter_compute_grid_based(self.h, C.byref(params), int(grid_based)))

    def get_patches(self):
        cnt = self.L.tmc2_frame_patch_count(self.h)
        dc, oc = C.c_int64(), C.c_int64()
        _check(self.L.tmc2_frame_patch_pool_sizes(self.h, C.byref(dc), C.byref(oc)))
        patches = np.zeros(cnt, PATCH_DTYPE)
        d0 = np.zeros(dc.value, np.int16)
        d1 = np.zeros(dc.value, np.int16)
        occ = np.zeros(oc.value, np.uint8)
        _check(self.L.tmc2_frame_get_patches(self.h, _ptr(patches), _ptr(d0), _ptr(d1), _ptr(occ)))
        return patches, d0, d1, occ


    def get_patch_records(self):
        """(patch records, block-occupancy pool) without the depth pools: what the inter-frame packers work on."""
        cnt = self.L.tmc2_frame_patch_count(self.h)
        dc, oc = C.c_int64(), C.c_int64()
        _check(self.L.tmc2_frame_patch_pool_sizes(self.h, C.byref(dc), C.byref(oc)))
        patches, occ = np.zeros(cnt, PATCH_DTYPE), np.zeros(oc.value, np.uint8)
        _check(self.L.tmc2_frame_get_patches(self.h, _ptr(patches), None, None, _ptr(occ)))
        return patches, occ

    def set_packing(self, patch_list, matches, occupancy, packed_width, packed_height):
        """Install a packed patch list (list order) computed elsewhere -- on the rank that runs the inter-frame chain."""
        p = np.ascontiguousarray(patch_list, dtype=PATCH_DTYPE)
        occ = np.ascontiguousarray(occupancy, dtype=np.uint8)
        m = None if matches is None else np.ascontiguousarray(matches, dtype=np.int32)
        _check(self.L.tmc2_frame_set_packing(self.h, _ptr(p), len(p), None if m is None else _ptr(m), _ptr(occ), len(occ),
                                             int(packed_width), int(packed_height)))

    # PCCEncoder image generation, phase A
    def encoder_pack_flexible(self, preset_width=1280, tiles_hor=2, ratio=1.0):
        h = C.c_int32()
        _check(self.L.tmc2_encoder_pack_flexible(self.h, int(preset_width), int(tiles_hor), ratio, C.byref(h)))
        return h.value

    def encoder_pack_spatial_consistency(self, previous, preset_width=1280, tiles_hor=2, ratio=1.0):
        """S10' (constrainedPack): pack against the previous frame of the GOF (which must be packed already)."""
        h = C.c_int32()
        _check(self.L.tmc2_encoder_pack_spatial_consistency(self.h, previous.h, int(preset_width), int(tiles_hor), ratio, C.byref(h)))
        return h.value

    def get_packed_size(self):
        """(width, height) of the tile as the packers left it."""
        w, h = C.c_int32(), C.c_int32()
        _check(self.L.tmc2_frame_get_packed_size(self.h, C.byref(w), C.byref(h)))
        return w.value, h.value

    def get_patch_matches(self):
        m = np.zeros(self.L.tmc2_frame_patch_count(self.h), np.int32)
        _check(self.L.tmc2_frame_get_patch_matches(self.h, _ptr(m)))
        return m

    def get_patch_order(self):
        order = np.zeros(self.L.tmc2_frame_patch_count(self.h), np.int32)
        _check(self.L.tmc2_frame_get_patch_order(self.h, _ptr(order)))
        return order

    def encoder_generate_geometry_images(self, width, height, occ_precision=4):
        _check(self.L.tmc2_encoder_generate_geometry_images(self.h, int(width), int(height), int(occ_precision)))
        self._canvas = (int(width), int(height), int(occ_precision))

    def get_geometry_images(self, out=None):
        W, H, p = self._canvas
        if out is None:
            out = dict(occupancy=np.zeros((H, W), np.uint8), occ_video=np.zeros((H // p, W // p), np.uint8),
                       block_to_patch=np.zeros((H // 16, W // 16), np.uint32), geo0=np.zeros((H, W), np.uint16),
                       geo1=np.zeros((H, W), np.uint16))
        _check(self.L.tmc2_frame_get_geometry_images(self.h, _ptr(out["occupancy"]), _ptr(out["occ_video"]),
                                                     _ptr(out["block_to_patch"]), _ptr(out["geo0"]), _ptr(out["geo1"])))
        return out


    # PCCEncoder image generation, phase B
    def encoder_generate_attribute_images(self, color_transfer=None):
        """color_transfer = ColorTransferParams: the transfer under that set (tmc2_encoder_generate_attribute_images_ex); None: the CTC point."""
        if color_transfer is None:
            self._pbf = False
            _check(self.L.tmc2_encoder_generate_attribute_images(self.h))
            return
        color_transfer_params_check(color_transfer)                # (a refused set leaves the frame, and what is known of it here, as it was)
        self._pbf = False
        _check(self.L.tmc2_encoder_generate_attribute_images_ex(self.h, C.byref(color_transfer.struct())))

    def recon_count(self):
        """Points of the reconstructed cloud (0 before the reconstruction)."""
        return self.L.tmc2_frame_recon_count(self.h)

    def get_reconstruction(self, colors=True):
        M = self.L.tmc2_frame_recon_count(self.h)
        xyz, rgb, p2p = np.zeros((M, 3), np.int16), (np.zeros((M, 3), np.uint8) if colors else None), np.zeros((M, 3), np.uint32)
        _check(self.L.tmc2_frame_get_reconstruction(self.h, _ptr(xyz), None if rgb is None else _ptr(rgb), _ptr(p2p)))
        return xyz, rgb, p2p

    def codec_generate_point_cloud(self, pbf=None):
        """PCCCodec::generatePointCloud alone (no colour transfer, no attribute images).  pbf: None, or occupancy synthesis (patch
        border filtering) first, as (passesCount, filterSize, log2Threshold[, thresholdLossyOM]): the occupancy is then the filtered
        one and the frame has its boundary types from the filter."""
        self._pbf = pbf is not None
        if pbf is None:
            _check(self.L.tmc2_codec_generate_point_cloud(self.h))
            return
        passes, filter_size, log2_threshold, threshold_om = (tuple(pbf) + (0,))[:4]
        _check(self.L.tmc2_codec_generate_point_cloud_pbf(self.h, int(threshold_om), int(passes), int(filter_size), int(log2_threshold)))

    def get_patch_border_filtering(self):
        """What the filter of codec_generate_point_cloud(pbf=...) left: (occupancy, border), uint8, the interior sizeU0*16 x sizeV0*16
        of every patch in list order, back to back."""
        n = C.c_int64()
        _check(self.L.tmc2_frame_patch_border_filtering_size(self.h, C.byref(n)))
        occ, border = np.zeros(n.value, np.uint8), np.zeros(n.value, np.uint8)
        _check(self.L.tmc2_frame_get_patch_border_filtering(self.h, _ptr(occ), _ptr(border)))
        return occ, border

    # post-reconstruction tail (PCCEncoder::encode :571-719 / PCCDecoder::decode :330-470)
    def codec_identify_boundary_points(self):
        _check(self.L.tmc2_codec_identify_boundary_points(self.h))

    def encoder_attribute_to_yuv420(self, downsampling_filter=4, out=None):
        """The two attribute canvases as the I420 frames the video encoder reads: uint8 [2][H*W*3/2]."""
        W, H, _ = self._canvas
        if out is None:
            out = np.zeros((2, W * H * 3 // 2), np.uint8)
        _check(self.L.tmc2_encoder_attribute_to_yuv420(self.h, int(downsampling_filter), _ptr(out)))
        return out

    def codec_set_decoded_attribute_yuv420(self, yuv420, upsampling_filter=0):
        """The two decoded I420 attribute frames (uint8 [2][H*W*3/2]) -> 16-bit 4:4:4 planes kept on the device."""
        W, H, _ = self._canvas
        src = np.ascontiguousarray(yuv420, dtype=np.uint8)
        if src.size != 2 * (W * H * 3 // 2):
            raise ValueError("decoded I420 frames must hold 2 x %d bytes" % (W * H * 3 // 2))
        _check(self.L.tmc2_codec_set_decoded_attribute_yuv420(self.h, _ptr(src), int(upsampling_filter)))

    def get_decoded_attribute(self):
        W, H, _ = self._canvas
        out = np.zeros((2, 3, H, W), np.uint16)
        _check(self.L.tmc2_frame_get_decoded_attribute(self.h, _ptr(out)))
        return out

    def codec_color_point_cloud(self, attribute16=None):
        """attribute16: the decoded attribute frames of this frame, uint16 [2][3][H][W]; None: those already on the device
        (codec_set_decoded_attribute_yuv420)."""
        if attribute16 is None:
            _check(self.L.tmc2_codec_color_point_cloud(self.h, None))
            return
        W, H, _ = self._canvas
        att = np.ascontiguousarray(attribute16, dtype=np.uint16)
        if att.shape != (2, 3, H, W):
            raise ValueError("decoded attribute frames must be uint16 [2][3][%d][%d]" % (H, W))
        _check(self.L.tmc2_codec_color_point_cloud(self.h, _ptr(att)))

    def codec_smooth_point_cloud_postprocess(self, grid_size=8, threshold=64.0):
        _check(self.L.tmc2_codec_smooth_point_cloud_postprocess(self.h, int(grid_size), threshold))

    def codec_transfer_colors_16bit_bp(self):
        _check(self.L.tmc2_codec_transfer_colors_16bit_bp(self.h))

    def codec_convert_yuv16_to_rgb8(self):
        _check(self.L.tmc2_codec_convert_yuv16_to_rgb8(self.h))

    def set_geometry_bit_depth_3d(self, bits3d):
        """The cube of the colour smoothing's grid, for a frame that did not run segmenter_compute (a decoder-side frame)."""
        _check(self.L.tmc2_frame_set_geometry_bit_depth_3d(self.h, int(bits3d)))

    def codec_color_smoothing(self, grid_size, thr_smoothing=10.0, thr_difference=10.0, thr_variation=6.0):
        """PCCCodec::colorSmoothing on the finished cloud (after codec_transfer_colors_16bit_bp, before codec_convert_yuv16_to_rgb8);
        grid_size = occupancyPrecision; the thresholds default as PCCEncoderParameters does."""
        _check(self.L.tmc2_codec_color_smoothing(self.h, int(grid_size), thr_smoothing, thr_difference, thr_variation))

    def codec_post_reconstruct(self, attribute16=None, grid_size=8, threshold=64.0, color_smoothing=None, pbf=None):
        """The whole tail in the reference's order: boundary points, 16-bit colours from the decoded attribute frames, grid
        geometry smoothing, colour transfer onto the moved points, [colour smoothing,] YUV -> RGB.  color_smoothing: None (the
        CTC: flagColorSmoothing off) or the arguments of codec_color_smoothing as a tuple, (grid_size[, thresholds ...]).
        pbf: None, or the arguments of codec_generate_point_cloud(pbf=...) for a stream with occupancy synthesis: the frame is
        reconstructed again with the filter, the boundary points are the filter's, and the colour transfer onto the moved points
        is not run (PCCEncoder.cpp:653, PCCDecoder.cpp:412)."""
        if pbf is not None:
            self.codec_generate_point_cloud(pbf)
        else:
            if getattr(self, "_pbf", False):   # (an earlier call left the filtered reconstruction: back to the plain rule)
                self.codec_generate_point_cloud()
            self.codec_identify_boundary_points()
        self.codec_color_point_cloud(attribute16)
        self.codec_smooth_point_cloud_postprocess(grid_size, threshold)
        if pbf is None:
            self.codec_transfer_colors_16bit_bp()
        if color_smoothing is not None:
            self.codec_color_smoothing(*color_smoothing)
        self.codec_convert_yuv16_to_rgb8()

    def get_post_reconstruction(self, xyz=True, colors16=True, rgb=True, boundary=True):
        M = self.L.tmc2_frame_recon_count(self.h)
        out = dict(xyz=np.zeros((M, 3), np.int16) if xyz else None, colors16=np.zeros((M, 3), np.uint16) if colors16 else None,
                   rgb=np.zeros((M, 3), np.uint8) if rgb else None, boundary=np.zeros(M, np.uint16) if boundary else None)
        _check(self.L.tmc2_frame_get_post_reconstruction(self.h, *[None if out[k] is None else _ptr(out[k])
                                                                    for k in ("xyz", "colors16", "rgb", "boundary")]))
        return {k: v for k, v in out.items() if v is not None}

    def get_attribute_images(self, out=None):
        W, H, _ = self._canvas
        if out is None:
            out = np.zeros((2, 3, H, W), np.uint8)
        _check(self.L.tmc2_frame_get_attribute_images(self.h, _ptr(out)))
        return out

    def set_decoded_geometry(self, occ_video=None, geometry=None):
        ov = None if occ_video is None else np.ascontiguousarray(occ_video, dtype=np.uint8)
        g = None if geometry is None else np.ascontiguousarray(geometry, dtype=np.uint16)
        _check(self.L.tmc2_frame_set_decoded_geometry(self.h, None if ov is None else _ptr(ov), None if g is None else _ptr(g)))


class _Pinned:
    """tmc2_host_alloc / tmc2_host_free: page-locked host memory every device of the node can DMA into."""

    def __init__(self, nbytes):
        self.L, self.p, self.nbytes = load_library(), C.c_void_p(), int(nbytes)
        _check(self.L.tmc2_host_alloc(self.nbytes, C.byref(self.p)))
        self.__array_interface__ = dict(shape=(self.nbytes,), typestr="|u1", data=(self.p.value, False), version=3)

    def __del__(self):
        try:
            if self.p:
                self.L.tmc2_host_free(self.p)
                self.p = C.c_void_p()
        except Exception:
            pass


class SharedHostArray:
    """A named shared-memory segment (/dev/shm) mapped by several processes of the node, page-locked in the process that writes
    it from a GPU (tmc2_host_register).  create=True makes (and on close removes) the segment; every opener gets a numpy view."""

    def __init__(self, name, nbytes, create, register=True):
        import mmap
        self.path, self.nbytes, self.created, self.registered = os.path.join("/dev/shm", name), int(nbytes), bool(create), False
        fd = os.open(self.path, (os.O_CREAT | os.O_RDWR) if create else os.O_RDWR, 0o600)
        try:
            if create:
                os.ftruncate(fd, self.nbytes)
            self.map = mmap.mmap(fd, self.nbytes)
        finally:
            os.close(fd)
        self.array = np.frombuffer(self.map, dtype=np.uint8)
        if register:
            # (the mapping's own address, never a red-zone copy of the guard mode: the call page-locks the memory, it moves no payload)
            _check(load_library().tmc2_host_register(C.c_void_p(self.array.ctypes.data), self.nbytes))
            self.registered = True

    def close(self):
        if self.registered:
            rc = load_library().tmc2_host_unregister(C.c_void_p(self.array.ctypes.data))
            self.registered = False
            if rc != 0:
                raise Tmc2Error("tmc2_host_unregister(%s) failed: %d" % (self.path, rc))
        if self.created:
            try:
                os.unlink(self.path)
            except OSError:
                pass
            self.created = False


def host_array(shape, dtype=np.uint8):
    """A numpy array in page-locked host memory (the array keeps the allocation alive): destination of the canvas getters,
    so that the copies out of HBM are plain DMA."""
    dtype = np.dtype(dtype)
    n = int(np.prod(shape)) * dtype.itemsize
    return np.asarray(_Pinned(max(n, 1)))[:n].view(dtype).reshape(shape)


def encoder_canvas_size(heights, tile_width=1280, min_w=1280, min_h=1280):
    """resizeTileGeometryVideo + resizeGeometryVideo: common canvas of a GOF."""
    L = load_library()
    hs = np.ascontiguousarray(heights, dtype=np.int32)
    W, H = C.c_int32(), C.c_int32()
    _check(L.tmc2_encoder_canvas_size(_ptr(hs), len(hs), int(tile_width), int(min_w), int(min_h), C.byref(W), C.byref(H)))
    return W.value, H.value


# ---- host-only pieces (no device needed) -----------------------------------------------------------
def host_kdtree_build(xyz):
    L = load_library()
    xyz = np.ascontiguousarray(xyz, dtype=np.int16)
    perm = np.empty(len(xyz), np.uint32)
    nodes, depth = C.c_uint64(), C.c_int32()
    _check(L.tmc2_host_kdtree_build(_ptr(xyz), len(xyz), _ptr(perm), C.byref(nodes), C.byref(depth)))
    return perm, nodes.value, depth.value


def host_pack_flexible(patches, occupancy, preset_width=1280, tiles_hor=2, ratio=1.0):
    """(placed patches by index, order, height) -- the S10 placement on plain records."""
    L = load_library()
    p = np.array(patches, dtype=PATCH_DTYPE, order="C", copy=True)
    occ = np.ascontiguousarray(occupancy, dtype=np.uint8)
    order, h = np.zeros(len(p), np.int32), C.c_int32()
    _check(L.tmc2_host_pack_flexible(_ptr(p), len(p), _ptr(occ), int(preset_width), int(tiles_hor), ratio, _ptr(order),
                                     C.byref(h)))
    return p, order, h.value


def host_pack_spatial_consistency(patches, occupancy, previous_list, preset_width=1280, tiles_hor=2, ratio=1.0):
    """(placed patches by index, order, matches per list position, height) -- the S10' placement on plain records."""
    L = load_library()
    p = np.array(patches, dtype=PATCH_DTYPE, order="C", copy=True)
    prev = np.ascontiguousarray(previous_list, dtype=PATCH_DTYPE)
    occ = np.ascontiguousarray(occupancy, dtype=np.uint8)
    order, match, h = np.zeros(len(p), np.int32), np.zeros(len(p), np.int32), C.c_int32()
    _check(L.tmc2_host_pack_spatial_consistency(_ptr(p), len(p), _ptr(occ), _ptr(prev), len(prev), int(preset_width),
                                                int(tiles_hor), ratio, _ptr(order), _ptr(match), C.byref(h)))
    return p, order, match, h.value


def encoder_global_patch_allocation(frames, min_w=1280, min_h=1280):
    """S10' second half (random-access condition) over the packed frames of a GOF, in order; returns the tile
    (widths, heights) per frame.  Afterwards every frame's patch records are in list order."""
    L = load_library()
    n = len(frames)
    handles = (C.c_void_p * n)(*[fr.h for fr in frames])
    w, h = np.zeros(n, np.int32), np.zeros(n, np.int32)
    _check(L.tmc2_encoder_global_patch_allocation(handles, n, int(min_w), int(min_h), _ptr(w), _ptr(h)))
    return w, h


def host_global_patch_allocation(lists, pools, matches, tile_w, tile_h, min_w=1280, min_h=1280):
    """The allocation on plain records: per frame the patches in list order, their block-occupancy pool and matches.
    Returns per frame (list, pool, matches, tile width, tile height)."""
    L = load_library()
    n = len(lists)
    counts = np.array([len(x) for x in lists], np.int32)
    patches = np.ascontiguousarray(np.concatenate([np.asarray(x, dtype=PATCH_DTYPE) for x in lists]), dtype=PATCH_DTYPE)
    m = np.ascontiguousarray(np.concatenate([np.asarray(x, dtype=np.int32) for x in matches]), dtype=np.int32)
    pools = [np.ascontiguousarray(x, dtype=np.uint8) for x in pools]
    base = np.zeros(n, np.int64)
    base[1:] = np.cumsum([len(x) for x in pools])[:-1]
    occ = np.ascontiguousarray(np.concatenate(pools)) if n else np.zeros(0, np.uint8)
    # a patch can grow to the box of its track's union: never beyond the largest box of the GOF in either direction
    cap = int(len(patches) * max(1, int(patches["sizeU0"].max(initial=1))) * max(1, int(patches["sizeV0"].max(initial=1))))
    out, out_base = np.zeros(max(cap, 1), np.uint8), np.zeros(n + 1, np.int64)
    w, h = np.zeros(n, np.int32), np.zeros(n, np.int32)
    _check(L.tmc2_host_global_patch_allocation(n, _ptr(counts), _ptr(patches), _ptr(occ), _ptr(base), _ptr(m), int(tile_w),
                                               int(tile_h), int(min_w), int(min_h), _ptr(out), cap, _ptr(out_base),
                                               _ptr(w), _ptr(h)))
    res, at = [], 0
    for f in range(n):
        c = int(counts[f])
        res.append((patches[at:at + c].copy(), out[out_base[f]:out_base[f + 1] if f + 1 < n else out_base[n]].copy(),
                    m[at:at + c].copy(), int(w[f]), int(h[f])))
        at += c
    return res


def host_pack_gof_records(records, mode, min_w=1280, min_h=1280, tiles_hor=2, ratio=1.0):
    """PCCEncoder::placeSegments over the patch RECORDS of a GOF (tmc2_host_place_segments; no device): records[f] =
    (patches by index, occupancy pool) of frame f.  mode 0: every frame on its own (packFlexible); 1: the low-delay chain
    (frame f against frame f-1); 2: the chain followed by the global patch allocation (random access).
    Returns per frame (patch list in list order, pool the list's occOffsets point into, matches, tile width, tile height)."""
    L = load_library()
    n = len(records)
    if n == 0:
        return []
    counts = np.array([len(r) for r, _ in records], np.int32)
    patches = np.ascontiguousarray(np.concatenate([np.asarray(r, dtype=PATCH_DTYPE) for r, _ in records]), dtype=PATCH_DTYPE)
    pools = [np.ascontiguousarray(o, dtype=np.uint8) for _, o in records]
    base = np.zeros(n, np.int64)
    base[1:] = np.cumsum([len(x) for x in pools])[:-1]
    occ = np.ascontiguousarray(np.concatenate(pools))
    # (random access) a patch can grow to the box of its track's union: never beyond the largest box of the GOF in either direction
    cap = int(len(patches) * max(1, int(patches["sizeU0"].max(initial=1))) * max(1, int(patches["sizeV0"].max(initial=1)))) if mode == 2 else len(occ)
    out, out_base = np.zeros(max(cap, 1), np.uint8), np.zeros(n + 1, np.int64)
    m = np.zeros(max(len(patches), 1), np.int32)
    w, h = np.zeros(n, np.int32), np.zeros(n, np.int32)
    _check(L.tmc2_host_place_segments(n, _ptr(counts), _ptr(patches), _ptr(occ), _ptr(base), int(mode), int(min_w), int(min_h),
                                      int(tiles_hor), ratio, _ptr(m), _ptr(out), cap, _ptr(out_base), _ptr(w), _ptr(h)))
    res, at = [], 0
    for f in range(n):
        c = int(counts[f])
        res.append((patches[at:at + c].copy(), out[out_base[f]:out_base[f + 1]].copy(), m[at:at + c].copy(), int(w[f]), int(h[f])))
        at += c
    return res


def segmenter_params_check(params):
    """Raises Tmc2Error for a parameter set outside what the path implements (the CTC lossy conditions are inside)."""
    _check(load_library().tmc2_segmenter_params_check(C.byref(params)))


def metrics_display(out, source_points, reconstruct_points, counts, resolution=1023, with_c2p=True, precision=9, params=None):
    """The text PCCMetrics::display() prints for one frame (what the CTC log parsers read); params = MetricsParams: from the
    q[3][14] of the entries that take them (tmc2_metrics_display_ex)."""
    L = load_library()
    q = np.ascontiguousarray(out, dtype=np.float64)
    c = np.ascontiguousarray(counts, dtype=np.int64)
    need = C.c_uint64()
    if params is not None:
        if q.shape != (3, 14):
            raise Tmc2Error("metrics_display: q[3][14] expected with params")
        st = params.struct()
        _check(L.tmc2_metrics_display_ex(_ptr(q), C.byref(st), int(source_points), int(reconstruct_points), _ptr(c), int(resolution),
                                         int(bool(with_c2p)), int(precision), None, 0, C.byref(need)))
        buf = C.create_string_buffer(need.value)
        _check(L.tmc2_metrics_display_ex(_ptr(q), C.byref(st), int(source_points), int(reconstruct_points), _ptr(c), int(resolution),
                                         int(bool(with_c2p)), int(precision), buf, need.value, None))
        return buf.value.decode()
    _check(L.tmc2_metrics_display(_ptr(q), int(source_points), int(reconstruct_points), _ptr(c), int(resolution), int(bool(with_c2p)),
                                  int(precision), None, 0, C.byref(need)))
    buf = C.create_string_buffer(need.value)
    _check(L.tmc2_metrics_display(_ptr(q), int(source_points), int(reconstruct_points), _ptr(c), int(resolution), int(bool(with_c2p)),
                                  int(precision), buf, need.value, None))
    return buf.value.decode()


def checksum_file_write(path, digests):
    """PCCChecksum::write: digests = list of 16-byte MD5s, one per frame."""
    L = load_library()
    d = np.frombuffer(b"".join(digests), np.uint8).copy() if len(digests) else np.zeros(0, np.uint8)
    _check(L.tmc2_checksum_file_write(str(path).encode(), _ptr(d) if len(d) else None, len(digests)))


def checksum_file_read(path):
    L = load_library()
    n = C.c_uint64()
    _check(L.tmc2_checksum_file_read(str(path).encode(), None, 0, C.byref(n)))
    d = np.zeros(16 * max(1, n.value), np.uint8)
    _check(L.tmc2_checksum_file_read(str(path).encode(), _ptr(d), n.value, C.byref(n)))
    return [d[16 * f:16 * f + 16].tobytes() for f in range(n.value)]


def ply_info(path, read_normals=False):
    """(point count, has colours, has float normals) from the header of a PLY file."""
    L = load_library()
    n, c, m = C.c_uint64(), C.c_int(), C.c_int()
    _check(L.tmc2_ply_info(str(path).encode(), int(bool(read_normals)), C.byref(n), C.byref(c), C.byref(m)))
    return n.value, bool(c.value), bool(m.value)


def ply_read(path, read_normals=False, threads=0, out=None):
    """PCCPointSet3::read: (xyz int16[n][3], rgb uint8[n][3] or None, normals float64[n][3] or None).
    out = (xyz, rgb) preallocated arrays (e.g. views of page-locked memory) to land the cloud in."""
    L = load_library()
    n, has_rgb, has_nrm = ply_info(path, read_normals)
    if out is not None:
        xyz, rgb = out
        if len(xyz) < n or (rgb is not None and len(rgb) < n):
            raise ValueError("buffers too small for %d points" % n)
    else:
        xyz, rgb = np.zeros((n, 3), np.int16), (np.zeros((n, 3), np.uint8) if has_rgb else None)
    nrm = np.zeros((n, 3), np.float64) if has_nrm else None
    cnt = C.c_uint64()
    _check(L.tmc2_ply_read(str(path).encode(), _ptr(xyz), None if rgb is None or not has_rgb else _ptr(rgb),
                           None if nrm is None else _ptr(nrm), len(xyz), int(threads), C.byref(cnt)))
    return xyz[:n], (rgb[:n] if rgb is not None and has_rgb else None), nrm


def ply_write(path, xyz, rgb=None, normals=None, ascii=True):
    """PCCPointSet3::write, byte for byte."""
    L = load_library()
    xyz = np.ascontiguousarray(xyz, dtype=np.int16)
    rgb = None if rgb is None else np.ascontiguousarray(rgb, dtype=np.uint8)
    nrm = None if normals is None else np.ascontiguousarray(normals, dtype=np.float64)
    _check(L.tmc2_ply_write(str(path).encode(), _ptr(xyz), None if rgb is None else _ptr(rgb), None if nrm is None else _ptr(nrm),
                            len(xyz), int(bool(ascii))))


def point_set_checksum(xyz, rgb=None, reorder=False):
    """PCCPointSet3::computeChecksum: the 16 MD5 bytes."""
    L = load_library()
    xyz = np.ascontiguousarray(xyz, dtype=np.int16)
    rgb = None if rgb is None else np.ascontiguousarray(rgb, dtype=np.uint8)
    d = np.zeros(16, np.uint8)
    _check(L.tmc2_point_set_checksum(_ptr(xyz), None if rgb is None else _ptr(rgb), len(xyz), int(bool(reorder)), _ptr(d)))
    return d.tobytes()


def host_orient_normals(xyz, knn, normals):
    L = load_library()
    xyz = np.ascontiguousarray(xyz, dtype=np.int16)
    knn = np.ascontiguousarray(knn, dtype=np.uint32)
    out = np.array(normals, dtype=np.float64, order="C", copy=True)
    _check(L.tmc2_host_orient_normals(_ptr(xyz), len(xyz), _ptr(knn), int(knn.shape[1]), _ptr(out)))
    return out


def _color_smoothing_arrays(xyz, colors16, boundary, patch_index):
    xyz = np.ascontiguousarray(xyz, dtype=np.int16)
    out = np.array(colors16, dtype=np.uint16, order="C", copy=True)
    bt = np.ascontiguousarray(boundary, dtype=np.uint16)
    patch = np.ascontiguousarray(patch_index, dtype=np.uint32)
    if xyz.shape != (len(xyz), 3) or out.shape != xyz.shape or bt.shape != (len(xyz),) or patch.shape != (len(xyz),):
        raise Tmc2Error("color_smoothing: xyz [M][3], colors16 [M][3], boundary [M] and patch_index [M] of one M expected")
    return xyz, out, bt, patch


def host_color_smoothing(xyz, colors16, boundary, patch_index, grid_size, bits3d, thr_smoothing=10.0, thr_difference=10.0,
                         thr_variation=6.0):
    """tmc2_host_color_smoothing: PCCCodec::colorSmoothing restated on the host (no device); returns the smoothed colours."""
    L = load_library()
    a = _color_smoothing_arrays(xyz, colors16, boundary, patch_index)
    _check(L.tmc2_host_color_smoothing(_ptr(a[0]), _ptr(a[1]), _ptr(a[2]), _ptr(a[3]), len(a[0]), int(grid_size), int(bits3d),
                                       thr_smoothing, thr_difference, thr_variation))
    return a[1]


def host_metrics_compute(src_xyz, src_rgb, rec_xyz, rec_rgb, normals=None, resolution=1023.0, params=None):
    """tmc2_host_metrics_compute: PCCMetrics::compute restated on the host (no device) -> (q[3][14], counts[2]).  Raises Tmc2Error
    with error -6 (TMC2_E_ORDER) where the answer depends on the k-d tree's visiting order."""
    a = np.ascontiguousarray(src_xyz, np.int16)
    b = np.ascontiguousarray(src_rgb, np.uint8)
    c = np.ascontiguousarray(rec_xyz, np.int16)
    d = np.ascontiguousarray(rec_rgb, np.uint8)
    nm = None if normals is None else np.ascontiguousarray(normals, np.float64)
    out, counts = np.zeros((3, 14), np.float64), np.zeros(2, np.int64)
    st = (params or MetricsParams()).struct()
    _check(load_library().tmc2_host_metrics_compute(_ptr(a), _ptr(b), len(a), _ptr(c), _ptr(d), len(c), None if nm is None else _ptr(nm),
                                                    resolution, C.byref(st), _ptr(out), _ptr(counts)))
    return out, counts


def host_patch_border_filtering(patches, width, height, occ_precision, occ_video, geometry_d0, block_to_patch, passes, filter_size,
                                log2_threshold, threshold_om=0):
    """tmc2_host_patch_border_filtering: PatchBlockFiltering::patchBorderFiltering restated on the host (no device) -> (occupancy,
    border) as Frame.get_patch_border_filtering returns them."""
    L = load_library()
    pt = np.ascontiguousarray(patches, dtype=PATCH_DTYPE)
    ov = np.ascontiguousarray(occ_video, dtype=np.uint8)
    geo = np.ascontiguousarray(geometry_d0, dtype=np.uint16)
    b2p = np.ascontiguousarray(block_to_patch, dtype=np.uint32)
    if width <= 0 or height <= 0 or occ_precision <= 0 or ov.size != (height // occ_precision) * (width // occ_precision) or \
            geo.size != height * width or b2p.size != (height // 16) * (width // 16):
        raise Tmc2Error("host_patch_border_filtering: canvases do not match %dx%d at precision %d" % (width, height, occ_precision))
    n = int(sum(int(t["sizeU0"]) * int(t["sizeV0"]) * 256 for t in pt if t["sizeU0"] > 0 and t["sizeV0"] > 0))
    occ, border = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    _check(L.tmc2_host_patch_border_filtering(_ptr(pt), len(pt), int(width), int(height), int(occ_precision), _ptr(ov), _ptr(geo), _ptr(b2p),
                                              int(threshold_om), int(passes), int(filter_size), int(log2_threshold), _ptr(occ), _ptr(border)))
    return occ, border


def host_convert_points_to_voxels(xyz, vox_dim, bits3d):
    """tmc2_host_convert_points_to_voxels: PCCPatchSegmenter3::convertPointsToVoxels restated on the host (no device) -> (voxel
    positions [V][3] in first-occurrence order, the rank of every point's voxel [n])."""
    a = np.ascontiguousarray(xyz, np.int16).reshape(-1, 3)
    vox, rank, count = np.zeros((len(a), 3), np.int16), np.zeros(len(a), np.uint32), C.c_uint64()
    _check(load_library().tmc2_host_convert_points_to_voxels(_ptr(a), len(a), int(vox_dim), int(bits3d), _ptr(vox), C.byref(count), _ptr(rank)))
    return vox[:count.value].copy(), rank


def host_refine_segmentation(xyz, normals, partition, max_nn=256, lam=3.0, iterations=100, with_adjacency=False):
    """tmc2_host_refine_segmentation: PCCPatchSegmenter3::refineSegmentation restated on the host (no device) -> the refined
    partition, or (partition, adjacency [n][max_nn] in nanoflann's result order) with with_adjacency."""
    a = np.ascontiguousarray(xyz, np.int16).reshape(-1, 3)
    nrm = np.ascontiguousarray(normals, np.float64).reshape(-1, 3)
    out = np.array(partition, dtype=np.uint32, order="C", copy=True).reshape(-1)
    if len(nrm) != len(a) or len(out) != len(a):
        raise Tmc2Error("host_refine_segmentation: xyz [n][3], normals [n][3] and partition [n] of one n expected")
    adj = np.zeros((len(a), max(int(max_nn), 0) if int(max_nn) <= 1024 else 0), np.uint32) if with_adjacency else None
    _check(load_library().tmc2_host_refine_segmentation(_ptr(a), len(a), _ptr(nrm), _ptr(out), int(max_nn), lam, int(iterations),
                                                        None if adj is None else _ptr(adj)))
    return (out, adj) if with_adjacency else out


def selftest_std_sort(pairs, offsets):
    """tmc2_selftest_std_sort: the real std::sort( .., dist < dist ) on every list of pairs [total][2] = (distance, payload), list l
    = [offsets[l], offsets[l + 1]); returns the sorted copy (host only)."""
    out = np.ascontiguousarray(pairs, dtype=np.uint32).copy()
    off = np.ascontiguousarray(offsets, dtype=np.uint32)
    if out.ndim != 2 or out.shape[1] != 2 or len(off) < 1 or int(off[-1]) != len(out) or (np.diff(off.astype(np.int64)) < 0).any():
        raise Tmc2Error("selftest_std_sort: pairs [total][2] and rising offsets that end at total expected")
    _check(load_library().tmc2_selftest_std_sort(_ptr(out), _ptr(off), len(off) - 1))
    return out


def option_check(key, value):
    """tmc2_option_check: raises Tmc2Error where Context.set_option would refuse this value for this option (host only)."""
    _check(load_library().tmc2_option_check(key.encode(), None if value is None else str(value).encode()))


# ---- the prototypes of include/tmc2hip.h (declare, above) ---------------------------------------------
TMC2HIP = """
int tmc2_ctx_create(int, tmc2_ctx**)
void tmc2_ctx_destroy(tmc2_ctx*)
const char* tmc2_last_error(void)
int tmc2_ctx_synchronize(tmc2_ctx*)
int tmc2_host_alloc(size_t, void**)
void tmc2_host_free(void*)
int tmc2_host_register(void*, size_t)
int tmc2_host_unregister(void*)
int tmc2_host_gate_create(int, tmc2_host_gate**)
void tmc2_host_gate_destroy(tmc2_host_gate*)
int tmc2_ctx_set_host_gate(tmc2_ctx*, tmc2_host_gate*)
void tmc2_set_host_parallelism(int)
int tmc2_ctx_set_option(tmc2_ctx*, const char*, const char*)
const char* tmc2_ctx_get_option(tmc2_ctx*, const char*)
int tmc2_option_check(const char*, const char*)
int tmc2_ctx_reserve(tmc2_ctx*, uint64_t, int, int, int, int)
int tmc2_ctx_pool_stats(tmc2_ctx*, uint64_t*, uint64_t*, double*, uint64_t*)
int tmc2_ctx_device_alloc(tmc2_ctx*, size_t, void**)
int tmc2_ctx_device_free(tmc2_ctx*, void*)
int tmc2_ctx_upload(tmc2_ctx*, void*, const void*, size_t)
int tmc2_ctx_download(tmc2_ctx*, void*, const void*, size_t)
void* tmc2_ctx_stream(tmc2_ctx*)
int tmc2_ctx_device(tmc2_ctx*)
int tmc2_ctx_make_current(tmc2_ctx*)
int tmc2_ctx_stage_count(tmc2_ctx*)
const char* tmc2_ctx_stage_name(tmc2_ctx*, int)
double tmc2_ctx_stage_ms(tmc2_ctx*, int)
long tmc2_ctx_stage_calls(tmc2_ctx*, int)
void tmc2_ctx_stage_reset(tmc2_ctx*)
void tmc2_ctx_set_timing(tmc2_ctx*, int)
int tmc2_frame_create(tmc2_ctx*, const int16_t*, const uint8_t*, uint64_t, tmc2_frame**)
void tmc2_frame_destroy(tmc2_frame*)
int tmc2_kdtree_build(tmc2_frame*)
void tmc2_set_kdtree_placement(int)
void tmc2_set_refine_overlap(int)
int tmc2_frame_get_kdtree_order(tmc2_frame*, uint32_t*, int32_t*)
uint64_t tmc2_frame_point_count(const tmc2_frame*)
int tmc2_frame_reset(tmc2_frame*)
int tmc2_kdtree_search(tmc2_frame*, const int16_t*, uint64_t, int, uint32_t*, uint32_t*)
int tmc2_kdtree_search_wide(tmc2_frame*, const int16_t*, uint64_t, int, uint32_t*)
int tmc2_normals_compute_normals(tmc2_frame*, int)
int tmc2_normals_orient(tmc2_frame*)
int tmc2_normals_compute(tmc2_frame*, int, int)
int tmc2_frame_get_normals(tmc2_frame*, double*)
int tmc2_frame_set_normals(tmc2_frame*, const double*)
int tmc2_frame_get_adjacency(tmc2_frame*, uint32_t*)
int tmc2_weight_normal(tmc2_frame*, int, double, double[3])
int tmc2_segmenter_initial_segmentation(tmc2_frame*, const double[3])
int tmc2_segmenter_refine_grid_based(tmc2_frame*, int, double, int, int, int)
int tmc2_segmenter_refine(tmc2_frame*, int, double, int)
int tmc2_frame_get_partition(tmc2_frame*, uint32_t*)
int tmc2_frame_set_partition(tmc2_frame*, const uint32_t*)
int tmc2_segmenter_segment_patches(tmc2_frame*, const tmc2_segmenter_params*)
int tmc2_segmenter_compute(tmc2_frame*, const tmc2_segmenter_params*)
int tmc2_segmenter_params_check(const tmc2_segmenter_params*)
int tmc2_segmenter_compute_grid_based(tmc2_frame*, const tmc2_segmenter_params*, int)
int tmc2_segmenter_compute_knn_refine(tmc2_frame*, const tmc2_segmenter_params*, int)
int tmc2_segmenter_convert_points_to_voxels(tmc2_ctx*, const int16_t*, uint64_t, int, int, int16_t*, uint64_t*, uint32_t*)
int tmc2_frame_patch_count(tmc2_frame*)
int tmc2_frame_patch_pool_sizes(tmc2_frame*, int64_t*, int64_t*)
int tmc2_frame_get_patches(tmc2_frame*, tmc2_patch*, int16_t*, int16_t*, uint8_t*)
int tmc2_encoder_pack_flexible(tmc2_frame*, int, int, double, int32_t*)
int tmc2_encoder_pack_spatial_consistency(tmc2_frame*, tmc2_frame*, int, int, double, int32_t*)
int tmc2_frame_get_packed_size(tmc2_frame*, int32_t*, int32_t*)
int tmc2_frame_get_patch_matches(tmc2_frame*, int32_t*)
int tmc2_encoder_global_patch_allocation(tmc2_frame**, int, int, int, int32_t*, int32_t*)
int tmc2_frame_set_packing(tmc2_frame*, const tmc2_patch*, int, const int32_t*, const uint8_t*, int64_t, int, int)
int tmc2_frame_get_patch_order(tmc2_frame*, int32_t*)
int tmc2_encoder_canvas_size(const int32_t*, int, int, int, int, int32_t*, int32_t*)
int tmc2_encoder_generate_geometry_images(tmc2_frame*, int, int, int)
int tmc2_frame_get_geometry_images(tmc2_frame*, uint8_t*, uint8_t*, uint32_t*, uint16_t*, uint16_t*)
int tmc2_encoder_generate_attribute_images(tmc2_frame*)
int tmc2_transfer_colors(tmc2_ctx*, const int16_t*, const uint8_t*, uint64_t, const int16_t*, uint64_t, uint8_t*)
void tmc2_color_transfer_params_default(tmc2_color_transfer_params*)
int tmc2_color_transfer_params_check(const tmc2_color_transfer_params*)
int tmc2_transfer_colors_ex(tmc2_ctx*, const int16_t*, const uint8_t*, uint64_t, const int16_t*, uint64_t, const tmc2_color_transfer_params*, uint8_t*)
int tmc2_encoder_generate_attribute_images_ex(tmc2_frame*, const tmc2_color_transfer_params*)
int64_t tmc2_frame_recon_count(tmc2_frame*)
int tmc2_frame_get_reconstruction(tmc2_frame*, int16_t*, uint8_t*, uint32_t*)
int tmc2_frame_get_attribute_images(tmc2_frame*, uint8_t*)
int tmc2_frame_set_decoded_geometry(tmc2_frame*, const uint8_t*, const uint16_t*)
int tmc2_frame_device_images(tmc2_frame*, void**, void**, void**, void**)
int tmc2_frame_device_attribute(tmc2_frame*, void**)
int tmc2_color_convert_rgb444_to_yuv420(tmc2_ctx*, const uint8_t*, int, int, int, uint8_t*)
int tmc2_color_convert_yuv420_to_yuv444(tmc2_ctx*, const uint8_t*, int, int, int, uint16_t*)
int tmc2_encoder_attribute_to_yuv420(tmc2_frame*, int, uint8_t*)
int tmc2_codec_set_decoded_attribute_yuv420(tmc2_frame*, const uint8_t*, int)
int tmc2_frame_get_decoded_attribute(tmc2_frame*, uint16_t*)
int tmc2_decoder_frame_create(tmc2_ctx*, const tmc2_patch*, int, int, int, int, const uint8_t*, const uint16_t*, tmc2_frame**)
int tmc2_codec_generate_point_cloud(tmc2_frame*)
int tmc2_codec_generate_point_cloud_pbf(tmc2_frame*, int, int, int, int)
int tmc2_frame_patch_border_filtering_size(tmc2_frame*, int64_t*)
int tmc2_frame_get_patch_border_filtering(tmc2_frame*, uint8_t*, uint8_t*)
int tmc2_codec_identify_boundary_points(tmc2_frame*)
int tmc2_codec_color_point_cloud(tmc2_frame*, const uint16_t*)
int tmc2_codec_smooth_point_cloud_postprocess(tmc2_frame*, int, double)
int tmc2_codec_transfer_colors_16bit_bp(tmc2_frame*)
int tmc2_codec_color_smoothing(tmc2_frame*, int, double, double, double)
int tmc2_frame_set_geometry_bit_depth_3d(tmc2_frame*, int)
int tmc2_color_smoothing(tmc2_ctx*, const int16_t*, uint16_t*, const uint16_t*, const uint32_t*, uint64_t, int, int, double, double, double)
int tmc2_codec_convert_yuv16_to_rgb8(tmc2_frame*)
int tmc2_frame_get_post_reconstruction(tmc2_frame*, int16_t*, uint16_t*, uint8_t*, uint16_t*)
int tmc2_metrics_compute(tmc2_ctx*, const int16_t*, const uint8_t*, uint64_t, const int16_t*, const uint8_t*, uint64_t, const double*, double, double*, int64_t*)
int tmc2_metrics_compute_frame(tmc2_frame*, int, int, double, double*, int64_t*)
int tmc2_metrics_compute_frame_source(tmc2_frame*, int, const int16_t*, const uint8_t*, uint64_t, const double*, double, double*, int64_t*)
void tmc2_metrics_params_default(tmc2_metrics_params*)
int tmc2_metrics_compute_ex(tmc2_ctx*, const int16_t*, const uint8_t*, uint64_t, const int16_t*, const uint8_t*, uint64_t, const double*, double, const tmc2_metrics_params*, double*, int64_t*)
int tmc2_metrics_compute_frame_ex(tmc2_frame*, int, int, double, const tmc2_metrics_params*, double*, int64_t*)
int tmc2_metrics_compute_frame_source_ex(tmc2_frame*, int, const int16_t*, const uint8_t*, uint64_t, const double*, double, const tmc2_metrics_params*, double*, int64_t*)
int tmc2_metrics_ordered_sums(tmc2_ctx*, const double*, uint64_t, const double*, uint64_t, double*)
int tmc2_metrics_display(const double*, uint64_t, uint64_t, const int64_t*, uint64_t, int, int, char*, uint64_t, uint64_t*)
int tmc2_metrics_display_ex(const double*, const tmc2_metrics_params*, uint64_t, uint64_t, const int64_t*, uint64_t, int, int, char*, uint64_t, uint64_t*)
int tmc2_ply_info(const char*, int, uint64_t*, int*, int*)
int tmc2_ply_read(const char*, int16_t*, uint8_t*, double*, uint64_t, int, uint64_t*)
int tmc2_ply_write(const char*, const int16_t*, const uint8_t*, const double*, uint64_t, int)
int tmc2_point_set_checksum(const int16_t*, const uint8_t*, uint64_t, int, uint8_t[16])
int tmc2_checksum_file_write(const char*, const uint8_t*, uint64_t)
int tmc2_checksum_file_read(const char*, uint8_t*, uint64_t, uint64_t*)
int tmc2_host_kdtree_build(const int16_t*, uint64_t, uint32_t*, uint64_t*, int32_t*)
int tmc2_host_pack_flexible(tmc2_patch*, int, const uint8_t*, int, int, double, int32_t*, int32_t*)
int tmc2_host_global_patch_allocation(int, int32_t*, tmc2_patch*, const uint8_t*, const int64_t*, int32_t*, int, int, int, int, uint8_t*, int64_t, int64_t*, int32_t*, int32_t*)
int tmc2_host_pack_spatial_consistency(tmc2_patch*, int, const uint8_t*, const tmc2_patch*, int, int, int, double, int32_t*, int32_t*, int32_t*)
int tmc2_host_place_segments(int, const int32_t*, tmc2_patch*, const uint8_t*, const int64_t*, int, int, int, int, double, int32_t*, uint8_t*, int64_t, int64_t*, int32_t*, int32_t*)
int tmc2_host_orient_normals(const int16_t*, uint64_t, const uint32_t*, int, double*)
int tmc2_host_color_smoothing(const int16_t*, uint16_t*, const uint16_t*, const uint32_t*, uint64_t, int, int, double, double, double)
int tmc2_host_metrics_compute(const int16_t*, const uint8_t*, uint64_t, const int16_t*, const uint8_t*, uint64_t, const double*, double, const tmc2_metrics_params*, double*, int64_t*)
int tmc2_host_patch_border_filtering(const tmc2_patch*, int, int, int, int, const uint8_t*, const uint16_t*, const uint32_t*, int, int, int, int, uint8_t*, uint8_t*)
int tmc2_host_convert_points_to_voxels(const int16_t*, uint64_t, int, int, int16_t*, uint64_t*, uint32_t*)
int tmc2_host_refine_segmentation(const int16_t*, uint64_t, const double*, uint32_t*, int, double, int, uint32_t*)
int tmc2_host_transfer_colors(const int16_t*, const uint8_t*, uint64_t, const int16_t*, uint64_t, const tmc2_color_transfer_params*, uint8_t*)
int tmc2_selftest_scan(tmc2_ctx*, const uint32_t*, uint32_t*, uint64_t, uint32_t*, uint32_t*, const uint32_t*, int, uint64_t)
int tmc2_selftest_fill(tmc2_ctx*, const uint64_t*, int)
int tmc2_selftest_work_map(tmc2_ctx*, uint64_t, int, uint64_t, uint64_t, uint32_t*, uint32_t*)
int tmc2_selftest_components(tmc2_ctx*, const uint32_t*, const uint8_t*, const uint8_t*, const uint32_t*, uint64_t, uint32_t*, uint32_t*)
int tmc2_selftest_union_find(tmc2_ctx*, int, uint32_t*, uint64_t, const uint32_t*, uint64_t, int, int, uint32_t*, uint32_t*, uint32_t*)
int tmc2_selftest_cand_sort(tmc2_ctx*, uint32_t*, const uint32_t*, uint64_t, uint32_t*)
int tmc2_selftest_std_sort(uint32_t*, const uint32_t*, uint64_t)
int tmc2_selftest_marked_cells(tmc2_ctx*, const int16_t*, const uint8_t*, uint64_t, int, int, int, uint32_t*, uint32_t*, uint32_t*, const uint32_t*, uint64_t, uint32_t*)
int tmc2_selftest_wave(tmc2_ctx*, int, int, const void*, void*, uint32_t*, uint64_t)
int tmc2_selftest_pool_probe(tmc2_ctx*, uint64_t, uint8_t*, uint64_t*)
int tmc2_selftest_pool_poisoned(tmc2_ctx*, uint64_t*)
""".strip().split("\n")
