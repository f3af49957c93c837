"""Inputs of the colour-smoothing tests (tests/test_color_smoothing_host.py, tests/test_gpu_color_smoothing.py) and of the
generator of their fixture (tests/golden/make_color_smoothing_golden.py): arbitrary clouds by seed -- the fixture
tests/golden/color_smoothing.npz stores only their MD5 and what the unmodified reference made of them -- plus a small, slow
numpy restatement of PCCCodec::colorSmoothing with a switch for the abs() form, which the generator uses to COUNT the cases
whose result depends on the reference's abs() being the integer one (a test cannot see that from the outside)."""
import hashlib
import os

import numpy as np

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "color_smoothing.npz")
PIPELINE_THRESHOLDS = ((10.0, 10.0, 6.0), (1.0, 10.0, 6.0), (0.5, 2.0, 1.0))   # on the tiny GOF and the full-size frame: grid 4, 11 bits
RANDOM_SEEDS = range(48)
DENSE_SEEDS = range(12)


def digest(a):
    return hashlib.md5(np.ascontiguousarray(a).tobytes()).hexdigest()


def input_digest(xyz, c16, bt, part):
    return digest(xyz) + digest(c16) + digest(bt) + digest(part)


def random_case(seed):
    """Clouds in the style of test_oracle_golden.random_tail_cloud (noisy sheets, blobs with duplicate positions, dense cubes,
    dust; random or region-wise patch ids), at least half of the points of boundary type 1 (a few of type 3), colour spreads
    300 / 3 000 / 30 000, grids 2 / 4 / 8 at 10 bits, thresholds down to 0.1 / 1 / 0.002.
    -> (xyz, c16, bt, part, grid, bits, (thr_smoothing, thr_difference, thr_variation))"""
    rng = np.random.default_rng(9000 + seed)
    kind, n = int(rng.choice([0, 0, 1, 1, 2, 2, 3])), int(rng.integers(50, 3000))
    if kind == 0:
        base = rng.integers(8, 200, (n, 3))
        base[:, 2] = base[:, 0] // 3 + rng.integers(0, 4, n)
    elif kind == 1:
        c = rng.integers(16, 300, (int(rng.integers(2, 12)), 3))
        base = c[rng.integers(0, len(c), n)] + rng.integers(-6, 7, (n, 3))
    elif kind == 2:
        base = rng.integers(20, 20 + int(rng.integers(6, 30)), (n, 3))
    else:
        base = rng.integers(0, 1024, (n, 3))
    xyz = np.clip(base, 0, 1023).astype(np.int16)
    bt = (rng.random(n) < rng.choice([0.5, 0.8, 1.0])).astype(np.uint16)
    bt[rng.random(n) < 0.03] = 3
    part = rng.integers(0, int(rng.integers(2, 6)), n).astype(np.uint32)
    if rng.random() < 0.5:
        part = ((xyz[:, 0] // int(rng.integers(8, 64))) % 5).astype(np.uint32)
    spread = int(rng.choice([300, 3000, 30000]))
    c16 = np.clip(32768 + rng.integers(-spread, spread + 1, (n, 3)), 0, 65535).astype(np.uint16)
    grid = int(rng.choice([4, 4, 2, 8]))
    thr = (float(rng.choice([10, 1, 0.1, 0.1, 0.1])), float(rng.choice([100, 10, 10, 1])), float(rng.choice([6, 6, 6, 0.5, 0.05, 0.002])))
    return xyz, c16, bt, part, grid, 10, thr


def dense_case(seed):
    """3 000 points in a cube of 6-14 a side, colours 50 000-65 535, grids 8 / 16: cells of several hundred points whose float
    colour sums pass 2^24, where the order of the additions shows."""
    rng = np.random.default_rng(9100 + seed)
    n = 3000
    xyz = rng.integers(20, 20 + int(rng.integers(6, 15)), (n, 3)).astype(np.int16)
    bt = np.ones(n, np.uint16)
    part = rng.integers(0, 3, n).astype(np.uint32)
    c16 = rng.integers(50000, 65536, (n, 3)).astype(np.uint16)
    grid = int(rng.choice([8, 16]))
    thr = (float(rng.choice([10, 1, 0.1, 0.1])), float(rng.choice([10, 10, 1])), float(rng.choice([6, 6, 0.5, 0.05, 0.002])))
    return xyz, c16, bt, part, grid, 10, thr


def handbuilt_case():
    """One cell with lumas 100, 100, 102 from two patches and thresholdColorVariation 0.002: |mean - median| = 0.67 against
    0.512, which the integer abs turns into 0 -- the cell takes part in the blend (its chroma is far from the points' own);
    with a floating-point abs it would not."""
    xyz = np.array([[41, 41, 41], [42, 41, 41], [41, 42, 41], [44, 41, 41], [45, 41, 41]], np.int16)
    c16 = np.array([[100, 30000, 30000], [100, 1000, 1000], [102, 30000, 30000], [5000, 20000, 20000], [5100, 20000, 20000]], np.uint16)
    bt = np.ones(5, np.uint16)
    part = np.array([0, 1, 0, 2, 2], np.uint32)
    return xyz, c16, bt, part, 4, 10, (0.1, 100.0, 0.002)


def arbitrary_cases():
    """name -> case, in the fixture's order"""
    out = {"hand": handbuilt_case()}
    out.update({"rand%d" % s: random_case(s) for s in RANDOM_SEEDS})
    out.update({"dense%d" % s: dense_case(s) for s in DENSE_SEEDS})
    return out


def max_cell_sum(xyz, c16, bt, grid, bits):
    """the largest colour total of a marked cell (the ordered float sum matters from 2^24 on)"""
    th, half = 1 << bits, grid // 2
    disth, w = max(half, 1), (1 << bits) // grid
    P = xyz.astype(np.int64)
    inside = (bt == 1) & (P >= disth).all(1) & (P + disth < th).all(1)
    q = P[inside] // grid - (P[inside] % grid < half)
    marked = set()
    for d in range(8):
        c = q + np.array([d & 1, (d >> 1) & 1, d >> 2])
        marked.update(((c[:, 2] * w + c[:, 1]) * w + c[:, 0]).tolist())
    key = (P[:, 2] // grid * w + P[:, 1] // grid) * w + P[:, 0] // grid
    sel = np.isin(key, np.fromiter(marked, np.int64, len(marked)))
    if not sel.any():
        return 0
    _, inv = np.unique(key[sel], return_inverse=True)
    return int(max(np.bincount(inv, weights=c16[sel][:, k].astype(np.float64)).max() for k in range(3)))


def restatement(xyz, c16, bt, patch, grid, bits, thr, integer_abs=True):
    """PCCCodec::colorSmoothing in slow numpy (the generator's yardstick for the abs() form only; the product's restatement is
    tmc2_host_color_smoothing)."""
    ts, td, tv = thr
    th, half = 1 << bits, grid // 2
    disth = max(half, 1)
    P = xyz.astype(np.int64)

    def outside(p):
        return (p < disth).any() or (th <= p + disth).any()

    def lower(p):
        c = p // grid
        return c + np.where(p - c * grid < half, -1, 0)

    marked = set()
    for i in range(len(P)):
        if bt[i] == 1 and not outside(P[i]):
            q = lower(P[i])
            marked.update((q[0] + (d & 1), q[1] + ((d >> 1) & 1), q[2] + (d >> 2)) for d in range(8))
    cells = {}
    for i in range(len(P)):
        k = tuple(P[i] // grid)
        if k in marked:
            cells.setdefault(k, []).append(i)
    A = (lambda v: float(abs(int(v)))) if integer_abs else abs
    stat = {}
    for k, idx in cells.items():
        s = np.zeros(3, np.float32)
        for i in idx:
            s = (s + c16[i].astype(np.float32)).astype(np.float32)
        lum, n = np.sort(c16[idx, 0]), len(idx)
        mean = float(lum.astype(np.int64).sum()) / n
        med = float(lum[n // 2]) if n % 2 else (float(lum[n // 2]) + float(lum[n // 2 - 1])) / 2.0
        stat[k] = (n, s, len(set(int(patch[i]) for i in idx)) > 1, n > 1 and A(mean - med) > tv * 256.0)
    out = c16.copy()
    for i in range(len(P)):
        if bt[i] != 1 or outside(P[i]):
            continue
        S, cur = lower(P[i]), c16[i].astype(np.float64)
        st = [stat.get((S[0] + (d & 1), S[1] + ((d >> 1) & 1), S[2] + (d >> 2)), (0, None, False, False)) for d in range(8)]
        if not any(v[2] and v[0] for v in st):
            continue
        Wt = (P[i] - S * grid - half) * 2 + 1
        G = 2 * grid - Wt
        cen, Y0, early = np.zeros(3), 0.0, False
        for d, (n, s, _, varied) in enumerate(st):
            dst = cur
            if n > 0:
                dst = np.array([float(s[c]) / float(n) for c in range(3)])
                if d == 0:
                    if varied:
                        early = True
                        break
                elif A(Y0 - dst[0]) > td * 256.0 or varied:
                    dst = cur
            if d == 0:
                Y0 = dst[0]
            cen = cen + dst * float((Wt[0] if d & 1 else G[0]) * (Wt[1] if (d >> 1) & 1 else G[1]) * (Wt[2] if d >> 2 else G[2]))
        if early:
            continue
        cen = np.trunc(cen / float((2 * grid) ** 3) + 0.5)
        if A(cen[0] - cur[0]) * 10.0 / 256.0 >= ts:
            out[i] = cen.astype(np.int64).astype(np.uint16)
    return out


def pack_changes(before, after):
    """what the fixture stores of one result: indices and colours of the changed points, the MD5 of all colours"""
    idx = np.flatnonzero((before != after).any(1)).astype(np.uint32)
    return idx, after[idx], digest(after)
