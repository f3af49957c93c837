"""Generate tests/golden/metrics_options.npz from the UNMODIFIED reference's PCCMetrics::compute / display.

Run where the reference is (needs oracle/_ref/libtmc2ref.so: `make -C oracle ref`):
    python tests/golden/make_metrics_options_golden.py
The oracle's harness runs the metric at the defaults of PCCMetricsParameters only, so a shim of our own
(metrics_options_shim.cpp, next to this file) is compiled into a TEMPORARY directory against the reference's headers and
oracle/_ref/libtmc2ref.so with the include paths and flags of oracle/Makefile.  Everything stored is DATA the reference produced
(per case and parameter set the 3 x 14 doubles, the two counts, the MD5 of the text display() printed, its own time) -- no
reference text.  The inputs are rebuilt by the tests from tests/metrics_option_cases.py; their digests are stored."""
import ctypes as C
import hashlib
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "mpeg-pcc-tmc2_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import metrics_option_cases as mc  # noqa: E402

REF = os.environ.get("REF", "/root/reference")
LIBDIRS = ("PccLibCommon", "PccLibBitstreamCommon", "PccLibMetrics")


def build_shim(tmp):
    ref_dir = os.path.join(ROOT, "oracle", "_ref")
    out = os.path.join(tmp, "libmetricsoptionsshim.so")
    inc = ["-I" + os.path.join(ref_dir, "gen")] + ["-I%s/source/lib/%s/include" % (REF, d) for d in LIBDIRS] + \
          ["-I%s/dependencies/nanoflann" % REF, "-I%s/dependencies/libmd5" % REF]
    subprocess.check_call(["g++", "-O3", "-DNDEBUG", "-std=c++14", "-fPIC", "-w", "-shared"] + inc +
                          [os.path.join(HERE, "metrics_options_shim.cpp"), "-o", out, "-L" + ref_dir, "-ltmc2ref", "-Wl,-rpath," + ref_dir])
    return C.CDLL(out)


def reference_metrics(shim, src, sc, rec, rc, normals, params, resolution=1023.0):
    """-> (q[3][14], counts[2], display text, seconds inside compute)"""
    a, b = np.ascontiguousarray(src, np.int16), np.ascontiguousarray(sc, np.uint8)
    c, d = np.ascontiguousarray(rec, np.int16), np.ascontiguousarray(rc, np.uint8)
    nm = None if normals is None else np.ascontiguousarray(normals, np.float64)
    st = params.struct()
    flags = (C.c_int * 6)(st.computeC2c, st.computeC2p, st.computeColor, st.computeHausdorff, st.dropDuplicates, st.neighborsProc)
    out, counts, sec = np.zeros((3, 14), np.float64), np.zeros(2, np.int64), C.c_double()
    text = C.create_string_buffer(1 << 16)
    p = lambda x: x.ctypes.data_as(C.c_void_p)  # noqa: E731
    shim.mo_metrics.restype = C.c_long
    size = shim.mo_metrics(p(a), p(b), C.c_size_t(len(a)), p(c), p(d), C.c_size_t(len(c)), None if nm is None else p(nm),
                           C.c_double(resolution), flags, p(out), p(counts), text, C.c_long(len(text)), C.byref(sec))
    assert 0 < size < len(text)
    return out, counts, text.value.decode(), sec.value


def generate(shim):
    out = {}
    for name in mc.CASES:
        src, sc, rec, rc, nrm = mc.case(name)
        out[name + "__input_md5"] = np.array(mc.digest(src, sc, rec, rc, nrm))
        seconds = []
        for set_name, params in mc.PARAM_SETS.items():
            q, counts, text, sec = reference_metrics(shim, src, sc, rec, rc, mc.normals_for(name, params, nrm), params)
            k = mc.key(name, set_name)
            out[k + "__q"], out[k + "__counts"] = q, counts
            out[k + "__display_md5"] = np.array(hashlib.md5(text.encode()).hexdigest() if mc.display_is_defined(params) else "")
            seconds.append(sec)
        out[name + "__reference_seconds"] = np.array(seconds)
        print("%-17s %5d / %5d points, reference compute per set: %s s" % (name, len(src), len(rec), " ".join("%.2f" % s for s in seconds)),
              flush=True)
    out["cases"], out["sets"] = np.array(list(mc.CASES)), np.array(list(mc.PARAM_SETS))
    return out


def main():
    path = os.path.join(HERE, "metrics_options.npz")
    with tempfile.TemporaryDirectory() as tmp:
        out = generate(build_shim(tmp))
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
