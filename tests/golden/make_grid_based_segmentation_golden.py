"""Generate tests/golden/grid_based_segmentation.npz from the UNMODIFIED reference's fast mode (gridBasedSegmentation).

Run where the reference is (needs oracle/_ref/libtmc2ref.so: `make -C oracle ref`):
    python tests/golden/make_grid_based_segmentation_golden.py
The oracle's harness keeps the flag off, so a shim of our own (grid_based_segmentation_shim.cpp, next to this file) is compiled
into a TEMPORARY directory against the reference's headers and oracle/_ref/libtmc2ref.so with the include paths and flags of
oracle/Makefile.  Every case of tests/grid_based_cases.CHAIN runs in a CHILD process under a time limit: PCCPatchSegmenter3::compute
with the flag (the patch list), the same without it, and the members compute() calls between convertPointsToVoxels and
applyVoxelsDataToPoints (voxel count, partition of the points).  The fixture holds digests, counts and the reference's own seconds
only -- data produced by running the reference, no reference text.

The generator refuses to write a fixture in which the fast result equals the plain result on every case: it would pin nothing."""
import argparse
import concurrent.futures
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "mpeg-pcc-tmc2_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import grid_based_cases as gc  # noqa: E402
import oracle_binding as ob  # noqa: E402
import param_cases as pc  # noqa: E402

REF = os.environ.get("REF", "/root/reference")
LIBDIRS = ("PccLibCommon", "PccLibBitstreamCommon", "PccLibBitstreamWriter", "PccLibVideoEncoder", "PccLibColorConverter",
           "PccLibEncoder", "PccLibMetrics", "PccLibVideoDecoder")
KEYS = ("partition", "patches", "depth0", "depth1", "occupancy")


def build_shim(tmp):
    ref_dir = os.path.join(ROOT, "oracle", "_ref")
    out = os.path.join(tmp, "libgridbasedsegmentationshim.so")
    inc = ["-I" + os.path.join(ref_dir, "gen")] + ["-I%s/source/lib/%s/include" % (REF, d) for d in LIBDIRS] + \
          ["-I%s/dependencies/nanoflann" % REF, "-I%s/dependencies/libmd5" % REF]
    subprocess.check_call(["g++", "-O3", "-DNDEBUG", "-std=c++14", "-fPIC", "-w", "-shared"] + inc +
                          [os.path.join(HERE, "grid_based_segmentation_shim.cpp"), "-o", out, "-L" + ref_dir, "-ltmc2ref", "-Wl,-rpath," + ref_dir])
    return out


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _split(sp):
    """the parameter struct as the shim takes it: its 20 int32 fields and its 6 doubles"""
    names = [n for n, _ in ob.SegParams._fields_]
    ip = np.array([getattr(sp, n) for n in names[:20]], np.int32)
    dp = np.array([sp.maxAllowedDist2RawPointsDetection, sp.maxAllowedDist2RawPointsSelection, sp.lambdaRefineSegmentation] + list(sp.weightNormal), np.float64)
    return ip, dp


def _compute(shim, xyz, rgb, sp, grid_based, vox_dim):
    ip, dp = _split(sp)
    sizes, sec = np.zeros(2, np.int64), C.c_double()
    count = shim.gbs_compute(_p(xyz), _p(rgb), C.c_size_t(len(xyz)), _p(ip), _p(dp), int(grid_based), int(vox_dim), _p(sizes), C.byref(sec))
    rec, d0, d1, occ = np.zeros((count, 22), np.int32), np.zeros(sizes[0], np.int16), np.zeros(sizes[0], np.int16), np.zeros(sizes[1], np.uint8)
    shim.gbs_patches(_p(rec), _p(d0), _p(d1), _p(occ))
    patches = np.zeros(count, ob.PATCH_DTYPE)
    for j, name in enumerate(pc.PATCH_FIELDS):
        patches[name] = rec[:, j]
    return dict(patches=patches, depth0=d0, depth1=d1, occupancy=occ), sec.value


def child(shim_path, index):
    case = gc.CHAIN[index]
    name, vox_dim, orientation = case
    xyz, rgb = gc.cloud(name)
    xyz, rgb = np.ascontiguousarray(xyz, np.int16), np.ascontiguousarray(rgb, np.uint8)
    shim = C.CDLL(shim_path)
    shim.gbs_partition.restype = C.c_long
    sp = gc.oracle_fast_params(ob.Oracle(), xyz, orientation)
    fast, fast_seconds = _compute(shim, xyz, rgb, sp, 1, vox_dim)
    plain, plain_seconds = _compute(shim, xyz, rgb, sp, 0, vox_dim)
    ip, dp = _split(sp)
    partition, normals = np.zeros(len(xyz), np.uint32), np.zeros((len(xyz), 3), np.float64)
    voxels = shim.gbs_partition(_p(xyz), _p(rgb), C.c_size_t(len(xyz)), _p(ip), _p(dp), int(vox_dim), _p(partition), _p(normals))
    vox, rank = gc.voxelize(xyz, vox_dim)
    assert voxels == len(vox), "the restatement of the voxelisation counts %d voxels, the reference %d" % (len(vox), voxels)
    # a point's normal is its voxel's, bit for bit: the reference's copy back agrees with the ranks of the restatement
    first = np.zeros(len(vox), np.int64)
    first[rank[::-1]] = np.arange(len(xyz))[::-1]
    assert np.array_equal(normals.view(np.uint64), normals[first][rank].view(np.uint64)), "the reference's copy back disagrees with the restated ranks"
    print(json.dumps(dict(fast=gc.digests(voxels, partition, fast), plain=pc.result_digests(plain), seconds=[fast_seconds, plain_seconds],
                          normals=pc.digest(normals), points=len(xyz))))


def run(shim_path, index, limit):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", str(index), "--shim", shim_path], timeout=limit,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    if r.returncode != 0:
        raise RuntimeError("%s: exit %d\n%s" % (gc.chain_id(gc.CHAIN[index]), r.returncode, r.stderr[-2000:]))
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", type=int)
    ap.add_argument("--shim")
    ap.add_argument("--limit", type=float, default=600.0)
    ap.add_argument("--jobs", type=int, default=8)
    a = ap.parse_args()
    if a.case is not None:
        return child(a.shim, a.case)
    with tempfile.TemporaryDirectory() as tmp:
        shim_path = build_shim(tmp)
        with concurrent.futures.ThreadPoolExecutor(a.jobs) as ex:
            results = list(ex.map(lambda i: run(shim_path, i, a.limit), range(len(gc.CHAIN))))
    out, differing = {"names": np.array([gc.chain_id(c) for c in gc.CHAIN])}, 0
    for case, r in zip(gc.CHAIN, results):
        name, fast = gc.chain_id(case), r["fast"]
        same = all(fast[k] == r["plain"][k] for k in ("patch_count", "patches", "depth0", "depth1", "occupancy"))
        differing += not same
        print("%-28s %7d points %7d voxels %4d patches (plain: %4d%s)  reference %.3f s with the flag, %.3f s without" % (
            name, r["points"], fast["voxel_count"], fast["patch_count"], r["plain"]["patch_count"], ", the same result" if same else "", *r["seconds"]))
        out[name + "/input_md5"] = np.array(gc.input_digest(case))
        out[name + "/voxel_count"] = np.int32(fast["voxel_count"])
        out[name + "/patch_count"] = np.int32(fast["patch_count"])
        out[name + "/normals_md5"] = np.array(r["normals"])
        for k in KEYS:
            out[name + "/" + k + "_md5"] = np.array(fast[k])
        out[name + "/reference_seconds"] = np.array(r["seconds"])
    if differing == 0:
        sys.exit("the fast result equals the plain result on every case: such a fixture pins nothing")
    np.savez_compressed(gc.FIXTURE, **out)
    print("%d cases (%d on which the flag changes the patches) -> %s, %d bytes" % (len(gc.CHAIN), differing, gc.FIXTURE, os.path.getsize(gc.FIXTURE)))


if __name__ == "__main__":
    main()
