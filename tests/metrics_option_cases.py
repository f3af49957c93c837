"""The clouds and parameter sets of the metric's option tests (tmc2_metrics_compute_ex / tmc2_host_metrics_compute against
tests/golden/metrics_options.npz, which tests/golden/make_metrics_options_golden.py records from the unmodified reference).
Every cloud is rebuilt from a seed; the fixture stores a digest of each so that a drifted generator is caught.  Clouds have
2 000 - 3 000 points: the reference takes well under a second per parameter set."""
import functools
import hashlib
import itertools
import os

import numpy as np

import tmc2_amd as T
from tmc2_amd.synth import synth_cloud

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "metrics_options.npz")
E_ORDER = "tmc2hip error -6: "                      # TMC2_E_ORDER, as lib._check words it

P = T.MetricsParams
PARAM_SETS = {
    "default": P(),
    "hausdorff": P(compute_hausdorff=True),
    "dd0": P(drop_duplicates=0),
    "dd1": P(drop_duplicates=1),
    "np0": P(neighbors_proc=0),
    "np2": P(neighbors_proc=2),
    "np3": P(neighbors_proc=3),
    "np4": P(neighbors_proc=4),
    "no_c2c": P(compute_c2c=False),
    "no_c2p": P(compute_c2p=False),
    "no_color": P(compute_color=False),
    "hausdorff_no_c2c": P(compute_hausdorff=True, compute_c2c=False),
    "combined": P(drop_duplicates=0, neighbors_proc=4, compute_hausdorff=True),
}


def digest(*arrays):
    h = hashlib.md5()
    for a in arrays:
        if a is not None:
            h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def _unit(rng, n):
    """Unit normals rounded to multiples of 2^-20.  Sums of a few of them are exact, so the normal scaleNormals gives a reconstructed
    point nobody voted for -- the sum over its nearest source points in the k-d tree's RESULT order -- does not depend on that order,
    and the host form, which does not know it, can follow.  The point-to-plane terms built from them (a division by the group size,
    by the vote count) are doubles with full mantissas all the same."""
    v = rng.normal(size=(n, 3))
    return np.round(v / np.linalg.norm(v, axis=1, keepdims=True) * 2.0 ** 20) / 2.0 ** 20


def _tiny(rng, n=3000):
    """n distinct points of the `tiny` synthetic body, in a shuffled order"""
    xyz, rgb = synth_cloud("tiny")
    _, first = np.unique(xyz, axis=0, return_index=True)
    pick = rng.permutation(np.sort(first))[:n]
    return xyz[pick].copy(), rgb[pick].copy()


def ordinary(seed=11):
    """the tiny body against a jittered, recoloured copy (the jitter makes duplicates in the reconstruction); normals"""
    rng = np.random.default_rng(seed)
    xyz, rgb = _tiny(rng)
    move = rng.random(len(xyz)) < 0.3
    rec = xyz.copy()
    rec[move] += rng.integers(-1, 2, (int(move.sum()), 3)).astype(np.int16)
    col = np.clip(rgb.astype(np.int32) + rng.integers(-12, 13, rgb.shape), 0, 255).astype(np.uint8)
    order = rng.permutation(len(rec))
    return xyz, rgb, rec[order], col[order], _unit(rng, len(xyz))


def _with_repeats(rng, xyz, share, long_run):
    """share of the positions again 1-4 more times (2-5 in all), the position of row 0 `long_run` times in all; shuffled"""
    again = np.flatnonzero(rng.random(len(xyz)) < share)
    again = again[again != 0]
    extra = np.repeat(again, rng.integers(1, 5, len(again)))
    rows = np.concatenate([np.arange(len(xyz)), extra, np.zeros(max(long_run - 1, 0), np.int64)])
    rows = rows[rng.permutation(len(rows))]
    return xyz[rows], rng.integers(0, 256, (len(rows), 3)).astype(np.uint8)


def duplicates(seed=23, long_run=40):
    """A quarter of the positions 2-5 times with different colours, in both clouds; one position 40 times in both (with
    dropDuplicates 0 a minimum-distance group above the cap of 30); duplicated source points with differing normals (copyNormals'
    last-wins rule).  The reference refuses normals on a source with duplicates unless dropDuplicates is 0: see normals_for."""
    rng = np.random.default_rng(seed)
    cells = rng.permutation(40 ** 3)[:1300]
    base = np.stack([cells // 1600, (cells // 40) % 40, cells % 40], 1).astype(np.int16) * 2 + 100
    src, sc = _with_repeats(rng, base, 0.25, long_run)
    shifted = base.copy()
    move = rng.random(len(base)) < 0.4
    move[0] = False                                   # the long run sits at one place in both clouds
    shifted[move] += rng.integers(-1, 2, (int(move.sum()), 3)).astype(np.int16)
    rec, rc = _with_repeats(rng, shifted, 0.25, long_run)
    return src, sc, rec, rc, _unit(rng, len(src))


def duplicates_light(seed=29):
    """the same without the run of 40: what the host form can follow with dropDuplicates 0"""
    return duplicates(seed, long_run=1)


def lattice(seed=31, side=12):
    """Reconstruction on the even lattice, source at odd midpoints: every source point has 2, 4 or 8 equidistant nearest
    neighbours with distinct colours, and the first in search order is not always the smallest index."""
    rng = np.random.default_rng(seed)
    rec = np.array(list(itertools.product(range(side + 1), repeat=3)), np.int16) * 2 + 50
    mid = np.array([p for p in itertools.product(range(2 * side + 1), repeat=3) if any(c & 1 for c in p)], np.int16) + 50
    src = mid[rng.permutation(len(mid))[:2600]]
    rec = rec[rng.permutation(len(rec))]
    return (src, rng.integers(0, 256, (len(src), 3)).astype(np.uint8), rec, rng.integers(0, 256, (len(rec), 3)).astype(np.uint8),
            _unit(rng, len(src)))


def identical(seed=37):
    """a cloud against itself: every distance 0, the Hausdorff maxima stay at DBL_MIN"""
    rng = np.random.default_rng(seed)
    xyz, rgb = _tiny(rng, 2000)
    return xyz, rgb, xyz.copy(), rgb.copy(), _unit(rng, len(xyz))


def point0(seed=41):
    """as ordinary, with point 0 of either cloud in an extreme colour: neighborsProc 3 and 4 fall back to it"""
    xyz, rgb, rec, col, nrm = ordinary(seed)
    rgb, col = rgb.copy(), col.copy()
    rgb[0], col[0] = (0, 255, 0), (255, 0, 255)
    return xyz, rgb, rec, col, nrm


CASES = {"ordinary": ordinary, "duplicates": duplicates, "duplicates_light": duplicates_light, "lattice": lattice, "identical": identical,
         "point0": point0}


@functools.lru_cache(maxsize=None)
def case(name):
    out = CASES[name]()
    for a in out:
        a.setflags(write=False)
    return out


def normals_for(name, params, nrm):
    """PCCPointSet3::copyNormals exits unless the de-duplicated source has as many points as the normal cloud: the cases whose
    source has duplicates carry normals only with dropDuplicates 0."""
    return None if name.startswith("duplicates") and params.drop_duplicates != 0 else nrm


def runs():
    return [(c, s) for c in CASES for s in PARAM_SETS]


def key(case_name, set_name):
    return "%s__%s" % (case_name, set_name)


def display_is_defined(params):
    """With computeColor off the reference's symmetric row prints colorMse_[1 .. 2] and colorPsnr_[1 .. 2] of a QualityMetrics whose
    constructor never set them: that text is not a function of the input, and no digest of it is stored."""
    return params.compute_color
