"""Inputs of the patch-border-filtering tests (tests/test_patch_border_filtering_host.py, tests/test_gpu_patch_border_filtering.py)
and of the generator of their fixture (tests/golden/make_patch_border_filtering_golden.py): hand-built canvases, the 256
orientation-table canvases, seeded random canvases -- the fixture tests/golden/patch_border_filtering.npz stores only their MD5 and
what the unmodified reference made of them -- plus a small, slow Python restatement of the filter with three switches (double
accumulation, last-wins landings, a forced orientation), which the generator uses to COUNT what the cases pin (a test cannot see
that from the outside).  The product's restatement is tmc2_host_patch_border_filtering."""
import hashlib
import os

import numpy as np

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "patch_border_filtering.npz")
# (occupancy precision, (passesCount, filterSize, log2Threshold)) on the 2-frame tiny GOF; thresholdLossyOM 0
PIPELINE_SETS = ((4, (2, 4, 2)), (4, (1, 2, 1)), (4, (3, 5, 4)), (4, (1, 1, 2)), (2, (1, 2, 2)), (8, (4, 8, 3)), (1, (1, 1, 2)))
FULL_SIZE_PARAMS = (2, 4, 2)
RANDOM_SEEDS = range(20)
TABLE_PARAMS = (1, 4, 1, 0)   # one pass, window 9 x 5, reach 1: the table canvases
PATCH_FIELDS = ("index", "viewId", "normalAxis", "tangentAxis", "bitangentAxis", "projectionMode", "u1", "v1", "d1", "sizeU", "sizeV", "sizeD",
                "sizeDPixel", "sizeU0", "sizeV0", "size2DXInPixel", "size2DYInPixel", "d0Count", "eomAndD1Count", "u0", "v0", "patchOrientation")
PATCH_DTYPE = np.dtype([(n, np.int32) for n in PATCH_FIELDS] + [("depthOffset", np.int64), ("occOffset", np.int64)])

# the non-zero orientations by 8-neighbour pattern (top-left = bit 7 .. bottom-right = bit 0), grouped by orientation
ORIENTATION_PATTERNS = {1: (208, 209, 212, 240, 244, 246, 252), 2: (64, 224, 248, 253), 3: (104, 105, 108, 232, 233, 235, 249),
                        4: (8, 41, 107, 239), 5: (11, 15, 43, 47, 63, 111, 139), 6: (2, 7, 31, 191), 7: (22, 23, 54, 150, 151, 159, 215)}
ORIENTATION = np.zeros(256, np.int64)
for _o, _ps in ORIENTATION_PATTERNS.items():
    ORIENTATION[list(_ps)] = _o
STEP_X = (1, 1, 0, -1, -1, -1, 0, 1)


def step(o):
    return STEP_X[o], STEP_X[(o + 6) % 8]


def digest(a):
    return hashlib.md5(np.ascontiguousarray(a).tobytes()).hexdigest()


# what the filter and the reconstruction read of a patch record
USED_FIELDS = ("normalAxis", "tangentAxis", "bitangentAxis", "projectionMode", "u1", "v1", "d1", "sizeU0", "sizeV0", "u0", "v0", "patchOrientation")


def input_digest(case):
    records = np.stack([np.asarray(case["patches"][n], np.int32) for n in USED_FIELDS], 1) if len(case["patches"]) else np.zeros((0, 12), np.int32)
    return digest(records) + digest(case["occ_video"]) + digest(case["geo"]) + digest(case["block_to_patch"]) + \
        digest(np.array([case["width"], case["height"], case["precision"]] + list(case["params"]), np.int64))


def border_width(precision):
    return 16 if precision >= 8 else 8


def to_canvas(t, u, v):
    if t["patchOrientation"] == 0:
        return u + t["u0"] * 16, v + t["v0"] * 16
    return v + t["u0"] * 16, u + t["v0"] * 16


def derive_block_to_patch(patches, occ_video, width, height, precision):
    """as the library's decoder-side frame derives it: the LAST patch of the list whose rectangle covers the block, for blocks with
    any occupancy-video sample set"""
    cells = 16 // precision
    b2p = np.zeros((height // 16, width // 16), np.uint32)
    for by in range(height // 16):
        for bx in range(width // 16):
            if not occ_video[by * cells:(by + 1) * cells, bx * cells:(bx + 1) * cells].any():
                continue
            for k, t in enumerate(patches):
                w, h = (t["sizeU0"], t["sizeV0"]) if t["patchOrientation"] == 0 else (t["sizeV0"], t["sizeU0"])
                if t["u0"] <= bx < t["u0"] + w and t["v0"] <= by < t["v0"] + h:
                    b2p[by, bx] = k + 1
    return b2p


def build_case(precision, blocks_w, blocks_h, specs, params, block_to_patch=None):
    """specs: per patch a dict with u0, v0, sizeU0, sizeV0 [blocks], orient, axes (normal, tangent, bitangent), mode, u1, v1, d1,
    occ [sizeV0*16/p][sizeU0*16/p] (occupancy-video values), depth [sizeV0*16][sizeU0*16] (geometry map 0 samples), and
    optionally delta (map 1 = map 0 + delta).  Painted in list order in patch-local coordinates; a later patch overwrites."""
    W, H, p = blocks_w * 16, blocks_h * 16, precision
    occ_video = np.zeros((H // p, W // p), np.uint8)
    geo = np.zeros((2, H, W), np.uint16)
    patches = np.zeros(len(specs), PATCH_DTYPE)
    for k, s in enumerate(specs):
        t = patches[k]
        t["index"], t["normalAxis"], t["tangentAxis"], t["bitangentAxis"] = k, s["axes"][0], s["axes"][1], s["axes"][2]
        t["projectionMode"], t["viewId"] = s["mode"], s["axes"][0] + 3 * s["mode"]
        t["u1"], t["v1"], t["d1"] = s["u1"], s["v1"], s["d1"]
        t["sizeU0"], t["sizeV0"], t["u0"], t["v0"], t["patchOrientation"] = s["sizeU0"], s["sizeV0"], s["u0"], s["v0"], s["orient"]
        t["sizeU"], t["sizeV"] = s["sizeU0"] * 16, s["sizeV0"] * 16
        t["size2DXInPixel"], t["size2DYInPixel"] = t["sizeU"], t["sizeV"]
        occ = np.asarray(s["occ"]).astype(np.uint8)
        depth = np.asarray(s["depth"]).astype(np.int64)
        delta = np.asarray(s.get("delta", np.zeros_like(depth))).astype(np.int64)
        assert occ.shape == (s["sizeV0"] * 16 // p, s["sizeU0"] * 16 // p) and depth.shape == (s["sizeV0"] * 16, s["sizeU0"] * 16)
        vs, us = np.nonzero(np.kron(occ, np.ones((p, p), np.uint8)))
        for u, v in zip(us, vs):
            x, y = to_canvas(t, int(u), int(v))
            occ_video[y // p, x // p] = occ[v // p, u // p]
            geo[0, y, x] = depth[v, u] & 0xFFFF
            geo[1, y, x] = (depth[v, u] + delta[v, u]) & 0xFFFF
    b2p = derive_block_to_patch(patches, occ_video, W, H, p) if block_to_patch is None else np.asarray(block_to_patch, np.uint32)
    return dict(patches=patches, width=W, height=H, precision=p, occ_video=occ_video, geo=geo, block_to_patch=b2p, params=tuple(params))


def case_from_canvases(img, precision, params):
    """a frame of Reference.phase_a / Oracle.phase_a as a case (thresholdLossyOM 0)"""
    patches = np.zeros(len(img["patches"]), PATCH_DTYPE)
    for n in PATCH_DTYPE.names:
        patches[n] = img["patches"][n]
    return dict(patches=patches, width=int(img["width"]), height=int(img["height"]), precision=precision,
                occ_video=np.ascontiguousarray(img["occ_video"], np.uint8), geo=np.stack([img["geo0"], img["geo1"]]).astype(np.uint16),
                block_to_patch=np.ascontiguousarray(img["block_to_patch"], np.uint32), params=tuple(params) + (0,))


def interior_pixels(case):
    return int(sum(int(t["sizeU0"]) * int(t["sizeV0"]) * 256 for t in case["patches"]))


# ---- the slow restatement (the generator's yardstick for its counts only) -----------------------------------------------------
def _wrap32(v):
    v &= 0xFFFFFFFF
    return v - (1 << 32) if v >= (1 << 31) else v


def _i16(v):
    v &= 0xFFFF
    return v - 65536 if v >= 32768 else v


def local_maps(case):
    """-> per patch (occ uint8, depth int64 holding int16 values), padded"""
    p, W = case["precision"], case["width"]
    b = border_width(p)
    thr = case["params"][3]
    out = []
    for k, t in enumerate(case["patches"]):
        su, sv = int(t["sizeU0"]) * 16, int(t["sizeV0"]) * 16
        occ = np.zeros((sv + 2 * b, su + 2 * b), np.uint8)
        depth = np.zeros((sv + 2 * b, su + 2 * b), np.int64)
        for vb in range(int(t["sizeV0"])):
            for ub in range(int(t["sizeU0"])):
                bx, by = (ub + t["u0"], vb + t["v0"]) if t["patchOrientation"] == 0 else (vb + t["u0"], ub + t["v0"])
                if case["block_to_patch"][by, bx] != k + 1:
                    continue
                for v in range(vb * 16, vb * 16 + 16):
                    for u in range(ub * 16, ub * 16 + 16):
                        x, y = to_canvas(t, u, v)
                        if case["occ_video"][y // p, x // p] > thr:
                            occ[v + b, u + b] = 1
                            depth[v + b, u + b] = _i16(int(case["geo"][0, y, x]))
        out.append((occ, depth))
    return out


def border_points(case, maps):
    """-> per patch (list of (raster index, (x, y, z))), box (lo[3], hi[3])"""
    b = border_width(case["precision"])
    out = []
    for t, (occ, depth) in zip(case["patches"], maps):
        pts, lo, hi = [], [32767] * 3, [-32768] * 3
        su = int(t["sizeU0"]) * 16
        for v, u in np.argwhere(occ[b:-b, b:-b]):
            r, c = v + b, u + b
            nb = (occ[r, c - 1], occ[r, c + 1], occ[r - 1, c], occ[r + 1, c], occ[r, c - 2], occ[r, c + 2], occ[r - 2, c], occ[r + 2, c],
                  occ[r + 1, c - 1], occ[r + 1, c + 1], occ[r - 1, c - 1], occ[r - 1, c + 1])
            if all(nb):
                continue
            d = int(depth[r, c]) & 0xFFFF
            q = [0, 0, 0]
            q[t["tangentAxis"]] = _i16(int(u) + int(t["u1"]))
            q[t["bitangentAxis"]] = _i16(int(v) + int(t["v1"]))
            q[t["normalAxis"]] = _i16(d + int(t["d1"]) if t["projectionMode"] == 0 else max(0, int(t["d1"]) - d))
            pts.append((int(v) * su + int(u), tuple(q)))
            lo = [min(a, c_) for a, c_ in zip(lo, q)]
            hi = [max(a, c_) for a, c_ in zip(hi, q)]
        out.append((pts, (lo, hi)))
    return out


def restatement(case, accumulate="float", last_wins=False, force_orientation=None):
    """-> dict(occ, border: per patch interior maps; nd: per patch padded neighbour depths; stats)"""
    passes, fsize, l2t, _ = case["params"]
    b = border_width(case["precision"])
    maps = local_maps(case)
    pts = border_points(case, maps)
    stats = dict(occupied_before=0, occupied_after=0, border_points=sum(len(p[0]) for p in pts), pairs=0, sum_branch=0, sum_branch_empty=0,
                 ties=0, removed=0)
    res_occ, res_border, res_nd = [], [], []
    for k, t in enumerate(case["patches"]):
        occ, depth = maps[k]
        h, w = occ.shape
        nd = np.full((h, w), 32767, np.int64)
        lo, hi = pts[k][1]
        for j in range(len(case["patches"])):
            lo2, hi2 = pts[j][1]
            if j == k or not all(hi[a] >= lo2[a] and lo[a] <= hi2[a] for a in range(3)):
                continue
            stats["pairs"] += 1
            for _, q in pts[j][0]:
                if any(q[a] < _i16(lo[a] - 8) or q[a] > _i16(hi[a] + 8) for a in range(3)):
                    continue
                nrm = q[t["normalAxis"]]
                d = _i16(nrm - int(t["d1"]) if t["projectionMode"] == 0 else int(t["d1"]) - nrm)
                cu, cv = q[t["tangentAxis"]] - int(t["u1"]) + b, q[t["bitangentAxis"]] - int(t["v1"]) + b
                if not (0 <= cu < w and 0 <= cv < h):
                    continue
                dist, held = abs(d - int(depth[cv, cu])), abs(int(nd[cv, cu]) - int(depth[cv, cu]))
                if dist <= l2t * l2t and (dist < held or (last_wins and dist == held and nd[cv, cu] != 32767)):
                    nd[cv, cu] = d
        src = occ.copy()
        stats["occupied_before"] += int(src.sum())
        for it in range(passes):
            dst = np.zeros_like(src)
            for v, u in np.argwhere(src[b:-b, b:-b]):
                r, c = v + b, u + b
                n = int(src[r, c - 1]) + int(src[r, c + 1]) + int(src[r - 1, c]) + int(src[r + 1, c])
                if n == 0:
                    continue
                if n == 4:
                    dst[r, c] = 1
                    continue
                pat = (int(src[r - 1, c - 1]) << 7) | (int(src[r - 1, c]) << 6) | (int(src[r - 1, c + 1]) << 5) | (int(src[r, c - 1]) << 4) | \
                      (int(src[r, c + 1]) << 3) | (int(src[r + 1, c - 1]) << 2) | (int(src[r + 1, c]) << 1) | int(src[r + 1, c + 1])
                orx = int(ORIENTATION[pat])
                forced = (force_orientation or {}).get(k)
                if forced is not None and (int(v), int(u)) == forced[:2]:
                    orx = forced[2]
                (xx, xy), (yx, yy) = step(orx), step((orx + 2) % 8)
                dE, dP = int(depth[r - xy, c - xx]), int(depth[r, c])
                f32 = accumulate == "float"
                sumE = sumP = np.float32(0) if f32 else np.float64(0)
                count = 0
                with np.errstate(invalid="ignore"):
                    for dx in range(-fsize, fsize + 1):
                        for dy in range(-(fsize >> 1), (fsize >> 1) + 1):
                            du, dv = dx * xx + dy * yx, dx * xy + dy * yy
                            val = int(nd[r + dv, c + du])
                            if val == 32767:
                                continue
                            rp = np.sqrt(np.float64(_wrap32(du * du + dv * dv + (val - dP) ** 2)))
                            re = np.sqrt(np.float64(_wrap32((du + xx) ** 2 + (dv + xy) ** 2 + (val - dE) ** 2)))
                            sumP = np.float32(np.float64(sumP) + rp) if f32 else sumP + rp
                            sumE = np.float32(np.float64(sumE) + re) if f32 else sumE + re
                            count += 1
                stats["sum_branch"] += 1
                stats["sum_branch_empty"] += count == 0
                stats["ties"] += bool(count and sumE == sumP)
                dst[r, c] = 1 if (count == 0 or sumE >= sumP) else 0
            src = dst
        stats["occupied_after"] += int(src.sum())
        flag = np.zeros_like(src)
        for r in range(b, h - b):
            for c in range(b, w - b):
                flag[r, c] = 0 if src[r - 2:r + 3, c - 2:c + 3].all() else 1
        res_occ.append(src[b:-b, b:-b].copy())
        res_border.append(flag[b:-b, b:-b].copy())
        res_nd.append(nd)
    stats["removed"] = stats["occupied_before"] - stats["occupied_after"]
    stats["sum_branch_nonempty"] = stats["sum_branch"] - stats["sum_branch_empty"]
    return dict(occ=res_occ, border=res_border, nd=res_nd, stats=stats)


def flatten(maps):
    return np.concatenate([m.reshape(-1) for m in maps]).astype(np.uint8) if maps else np.zeros(0, np.uint8)


def reconstruct(case, occupancy, border):
    """generatePointCloud on the filtered maps (flat, as the library returns them): points in patch list order, block raster, pixel
    raster, D0 before D1 -> (xyz int16 [M][3], pointToPixel uint32 [M][3], boundary uint16 [M])"""
    xyz, p2p, bt, at = [], [], [], 0
    for k, t in enumerate(case["patches"]):
        su, sv = int(t["sizeU0"]) * 16, int(t["sizeV0"]) * 16
        occ = occupancy[at:at + su * sv].reshape(sv, su)
        flag = border[at:at + su * sv].reshape(sv, su)
        at += su * sv
        for vb in range(sv // 16):
            for ub in range(su // 16):
                bx, by = (ub + t["u0"], vb + t["v0"]) if t["patchOrientation"] == 0 else (vb + t["u0"], ub + t["v0"])
                if case["block_to_patch"][by, bx] != k + 1:
                    continue
                for v in range(vb * 16, vb * 16 + 16):
                    for u in range(ub * 16, ub * 16 + 16):
                        if not occ[v, u]:
                            continue
                        x, y = to_canvas(t, u, v)
                        q = [0, 0, 0]
                        q[t["tangentAxis"]], q[t["bitangentAxis"]] = u + int(t["u1"]), v + int(t["v1"])
                        coords = [int(g) + int(t["d1"]) if t["projectionMode"] == 0 else max(0, int(t["d1"]) - int(g)) for g in case["geo"][:, y, x]]
                        for layer in range(1 if coords[1] == coords[0] else 2):
                            q[t["normalAxis"]] = coords[layer]
                            xyz.append([_i16(c) for c in q])
                            p2p.append((x, y, layer))
                            bt.append(int(flag[v, u]))
    return np.array(xyz, np.int16).reshape(-1, 3), np.array(p2p, np.uint32).reshape(-1, 3), np.array(bt, np.uint16)


# ---- hand-built canvases ---------------------------------------------------------------------------------------------------
def _spec(u0, v0, su0, sv0, occ, depth, u1=0, v1=0, d1=0, orient=0, axes=(2, 0, 1), mode=0, delta=None):
    s = dict(u0=u0, v0=v0, sizeU0=su0, sizeV0=sv0, orient=orient, axes=axes, mode=mode, u1=u1, v1=v1, d1=d1, occ=occ, depth=depth)
    if delta is not None:
        s["delta"] = delta
    return s


def _noise(shape, seed, amp):
    return np.random.default_rng(seed).integers(-amp, amp + 1, shape)


def tilted_plane_case(mode, orient, precision=1, params=(2, 4, 2, 0), size=48, seed=1):
    """two patches that overlap along a ragged edge of one tilted, slightly rough plane: the border points of the one land on the
    rim of the other"""
    n = size
    vv, uu = np.mgrid[0:n, 0:n]
    plane = 40 + (uu + vv // 2) // 2 + _noise((n, n), seed, 1)
    edge = n // 2 + ((vv * 7) % 5) - 2
    left, right = uu < edge + 2, uu >= edge - 1   # (three shared columns: a border point lands where the other patch has a depth near its own)
    p = precision
    coarse = lambda m: m.reshape(n // p, p, n // p, p).any((1, 3)).astype(np.uint8)   # noqa: E731
    d1 = 0 if mode == 0 else 200
    depth = plane if mode == 0 else 200 - plane
    blocks = n // 16
    a = _spec(0, 0, blocks, blocks, coarse(left), depth, 10, 20, d1, orient, (2, 0, 1), mode, delta=(uu % 3 == 0).astype(np.int64))
    bpos = (blocks, 0)
    b = _spec(bpos[0], bpos[1], blocks, blocks, coarse(right), depth, 10, 20, d1, orient, (2, 0, 1), mode)
    return build_case(p, 2 * blocks, blocks, [a, b], params)


def handbuilt_cases():
    """name -> case, in the fixture's order"""
    out = {}
    for mode in (0, 1):
        for orient in (0, 1):
            out["plane_m%d_o%d" % (mode, orient)] = tilted_plane_case(mode, orient)
    out["plane_p4"] = tilted_plane_case(0, 0, 4, (2, 4, 2, 0), 64, 2)
    out["plane_p2_wide"] = tilted_plane_case(1, 1, 2, (3, 5, 4, 0), 64, 3)
    out["plane_p8"] = tilted_plane_case(0, 1, 8, (4, 8, 3, 0), 64, 4)
    out["plane_big"] = tilted_plane_case(0, 0, 1, (2, 4, 2, 0), 128, 5)
    disc = (np.hypot(*(np.mgrid[0:32, 0:32] - 15.5)) < 13).astype(np.uint8)
    flat = np.full((32, 32), 50)
    out["alone"] = build_case(1, 2, 2, [_spec(0, 0, 2, 2, disc, flat + _noise((32, 32), 6, 2), 5, 5, 3)], (2, 4, 2, 0))
    # an isolated pixel (and a 2x1 pair) next to a neighbour patch that covers them in 3-D
    iso = np.zeros((16, 16), np.uint8)
    iso[8, 8] = iso[3, 3] = iso[3, 4] = 1
    out["isolated"] = build_case(1, 3, 2, [_spec(0, 0, 1, 1, iso, np.full((16, 16), 20), 8, 8, 0),
                                           _spec(1, 0, 2, 2, disc, 21 + _noise((32, 32), 12, 1), 0, 0, 0)], (1, 2, 2, 0))
    # two neighbour points at depth + 2 and depth - 2 on one pixel of patch 0, in both orders of the two neighbours: the first stays
    sq = np.zeros((16, 16), np.uint8)
    sq[4:11, 4:11] = 1
    ramp = np.full((16, 16), 30) + (np.mgrid[0:16, 0:16][1] - 7)   # 27 .. 33 across the square: its box covers depth +- 2
    one = np.zeros((16, 16), np.uint8)
    one[7, 6] = 1
    up, down = np.full((16, 16), 31), np.full((16, 16), 27)         # pixel (u 6, v 7) of patch 0 has depth 29
    for name, order in (("tie_up_first", (up, down)), ("tie_down_first", (down, up))):
        out[name] = build_case(1, 3, 1, [_spec(0, 0, 1, 1, sq, ramp, 0, 0, 0), _spec(1, 0, 1, 1, one, order[0], 0, 0, 0),
                                         _spec(2, 0, 1, 1, one, order[1], 0, 0, 0)], (1, 2, 2, 0))
    # a 2x2-block patch one block of which a later patch owns
    full = np.ones((32, 32), np.uint8)
    full[:, 30:] = 0
    out["partly_owned"] = build_case(1, 3, 2, [_spec(0, 0, 2, 2, full, 60 + _noise((32, 32), 7, 1), 0, 0, 0),
                                               _spec(1, 1, 1, 1, np.ones((16, 16), np.uint8), 61 + _noise((16, 16), 8, 1), 24, 0, 0)], (2, 4, 2, 0))
    # occupancy-video samples 0 .. 255 against thresholdLossyOM 0, 1, 128
    vals = ((np.arange(64).reshape(8, 8) * 4 + 1) % 256).astype(np.uint8)
    vals[0, 0], vals[0, 1], vals[7, 7], vals[3, 3] = 0, 1, 255, 128
    for thr in (0, 1, 128):
        out["threshold_%d" % thr] = build_case(4, 4, 2, [_spec(0, 0, 2, 2, vals, 80 + _noise((32, 32), 9, 1), 0, 0, 0),
                                                          _spec(2, 0, 2, 2, vals.T.copy(), 80 + _noise((32, 32), 10, 1), 30, 0, 0)], (2, 4, 2, thr))
    # a one-block patch, and a patch in the canvas's last block row and column
    blk = np.ones((16, 16), np.uint8)
    blk[0, :] = 0
    out["corner"] = build_case(1, 3, 3, [_spec(0, 0, 1, 1, blk, np.full((16, 16), 10), 0, 0, 0),
                                         _spec(2, 2, 1, 1, blk.T.copy(), np.full((16, 16), 11) + _noise((16, 16), 11, 1), 12, 0, 0, orient=1)],
                               (2, 4, 2, 0))
    # flat, mirror-symmetric neighbours: windows in which the two sums are equal
    half = np.zeros((32, 32), np.uint8)
    half[:, :16] = 1
    out["equal_sums"] = build_case(1, 4, 2, [_spec(0, 0, 2, 2, half, np.full((32, 32), 40), 1, 0, 0),
                                             _spec(2, 0, 2, 2, half[:, ::-1].copy(), np.full((32, 32), 40), 0, 0, 0)], (1, 1, 2, 0))
    # a patch with no occupied sample between two that have
    out["empty_patch"] = build_case(2, 3, 1, [_spec(0, 0, 1, 1, np.ones((8, 8), np.uint8), np.full((16, 16), 5), 0, 0, 0),
                                              _spec(1, 0, 1, 1, np.zeros((8, 8), np.uint8), np.zeros((16, 16)), 16, 0, 0),
                                              _spec(2, 0, 1, 1, np.ones((8, 8), np.uint8), np.full((16, 16), 6), 14, 0, 0)], (2, 4, 2, 0))
    # depths next to 32767, the value that means "no neighbour depth": a neighbour point of depth 32767 lands and counts as none
    uu = np.mgrid[0:32, 0:32][1]
    vv = np.mgrid[0:32, 0:32][0]
    out["near_undefined"] = build_case(1, 4, 2, [_spec(0, 0, 2, 2, half, 32752 + uu % 8, 0, 0, 0),
                                                 _spec(2, 0, 2, 2, half, 32759 + 8 * ((uu + vv) % 2), 14, 0, 0)], (2, 4, 3, 0))
    # geometry samples at and above 32768: the depth map holds them as int16, the points' coordinates wrap
    high = 32766 + uu // 6
    out["high_depth"] = build_case(1, 4, 2, [_spec(0, 0, 2, 2, half, high, 0, 0, 0), _spec(2, 0, 2, 2, half, high - 1, 14, 0, 0)], (2, 4, 2, 0))
    out["high_depth_m1"] = build_case(1, 4, 2, [_spec(0, 0, 2, 2, half, high, 0, 0, 32767, mode=1),
                                                _spec(2, 0, 2, 2, half, high - 2, 14, 0, 32767, mode=1)], (2, 4, 3, 0))
    return out


# ---- the orientation table: one canvas per 8-neighbour pattern ----------------------------------------------------------------
def table_case(pattern):
    """Eight copies of a one-block patch whose pixel (8, 8) has the 3x3 neighbourhood `pattern` (two far pixels widen its box), each
    next to a one-pixel patch that lands two pixels from (8, 8) in one of the 8 compass directions; all depths 0.  The pixel is
    dropped exactly when the lone neighbour depth lies in its window AND nearer to the pixel one step against the orientation: the
    eight outcomes of pixel (8, 8) single out the table's value (for the patterns that reach the table: 1 to 3 of the 4-neighbours)."""
    a = np.zeros((16, 16), np.uint8)
    a[8, 8] = a[0, 0] = a[15, 15] = 1
    bits = ((7, -1, -1), (6, 0, -1), (5, 1, -1), (4, -1, 0), (3, 1, 0), (2, -1, 1), (1, 0, 1), (0, 1, 1))
    for bit, dx, dy in bits:
        a[8 + dy, 8 + dx] = (pattern >> bit) & 1
    one = np.zeros((16, 16), np.uint8)
    one[8, 8] = 1
    zero = np.zeros((16, 16))
    specs = []
    for i in range(8):
        qx, qy = step(i)
        specs.append(_spec(2 * i, 0, 1, 1, a, zero, 100 * i, 0, 0))
        specs.append(_spec(2 * i + 1, 0, 1, 1, one, zero, 100 * i + 2 * qx, 2 * qy + 0, 0))
    for s in specs:
        s["v1"] += 4   # (room for the probes above the patch)
    return build_case(1, 16, 1, specs, TABLE_PARAMS)


def table_reaches_lookup(pattern):
    return 1 <= bin(pattern & 0b01011010).count("1") <= 3


def table_signature(case, occupancy):
    """pixel (8, 8) of the eight pattern patches"""
    return np.array([int(occupancy[2 * i * 256 + 8 * 16 + 8]) for i in range(8)], np.uint8)


# ---- seeded random canvases (device against host restatement) -----------------------------------------------------------------
def random_case(seed):
    """a few blobby patches with random depths around a common surface, orientations 0 / 1, precisions 1 / 2 / 4 / 8, overlapping in
    3-D so that they are neighbours of each other"""
    rng = np.random.default_rng(7000 + seed)
    p = int(rng.choice([1, 2, 4, 8]))
    count = int(rng.integers(2, 6))
    params = [(2, 4, 2), (1, 2, 1), (3, 5, 4), (1, 1, 2), (2, 3, 3)][int(rng.integers(0, 5))] if p < 8 else \
        [(4, 8, 3), (2, 4, 2), (1, 10, 2)][int(rng.integers(0, 3))]
    specs, x = [], 0
    rows = 0
    for k in range(count):
        su0, sv0 = int(rng.integers(1, 5)), int(rng.integers(1, 5))
        su, sv = su0 * 16, sv0 * 16
        vv, uu = np.mgrid[0:sv // p, 0:su // p]
        occ = np.zeros((sv // p, su // p), bool)
        for _ in range(int(rng.integers(1, 4))):
            cy, cx, r = rng.uniform(0, sv // p), rng.uniform(0, su // p), rng.uniform(1.5, max(su, sv) / p / 1.5)
            occ |= np.hypot(vv - cy, uu - cx) < r
        occ &= rng.random(occ.shape) > 0.03
        orient = int(rng.integers(0, 2))
        mode = int(rng.integers(0, 2))
        axes = [(2, 0, 1), (0, 2, 1), (1, 2, 0)][int(rng.integers(0, 3))] if k else (2, 0, 1)
        base = int(rng.integers(30, 60))
        tilt = (np.mgrid[0:sv, 0:su][1] * int(rng.integers(0, 3))) // 4
        depth = base + tilt + rng.integers(-2, 3, (sv, su))
        d1 = int(rng.integers(0, 8)) if mode == 0 else int(rng.integers(120, 140))
        depth = depth if mode == 0 else d1 - depth
        depth = np.clip(depth, 0, 255)
        w, h = (su0, sv0) if orient == 0 else (sv0, su0)
        specs.append(_spec(x, 0, su0, sv0, occ.astype(np.uint8) * int(rng.integers(1, 255)), depth, int(rng.integers(20, 50)),
                           int(rng.integers(20, 50)), d1, orient, axes, mode, delta=rng.integers(0, 3, (sv, su))))
        x += w
        rows = max(rows, h)
    return build_case(p, x, rows, specs, params + (int(rng.choice([0, 0, 0, 7])),))
