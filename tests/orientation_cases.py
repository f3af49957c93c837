"""Hand-built normal fields for the orientation (S3), and a plain classifier that says which path each must take.

The orientation only flips signs, `tmc2_frame_set_normals` lets a caller bring any finite field, and the stage counters record
which path ran -- so every case here is compared bit for bit with `oracle.orient_normals`, and where the classifier can tell, the
counters are asserted exactly.  numpy only (the PCA normals of a cloud come from the oracle handed to `cases()`).

    cases(oracle)                    -> (name, xyz, normals), seeded, 17 .. ~6 500 points each (noisy: 10.9 K, duplicates: 7.1 K)
    classify(knn, normals, tau)      -> "balanced" | "conflict" | "undetermined"
    expected_path(knn, normals, tau) -> (retries, regrowth) | None
    cross_pairs / compact_size       -> what the pair table and the speculative room must hold at a threshold

What the classifier restates (orient_host.cpp says why each holds):
  * an edge is strong if |n_u . n_v| >= tau and the dot product is not exactly 0 (the reference's "n_u . n_v < 0" is false for a
    zero whichever way u points: such an edge relates no two signs, at any threshold);
  * clusters = components of the MUTUAL strong edges (u lists v, v lists u), with a parity per point;
  * "conflict": a strong edge with both ends in one cluster -- mutual or one-way -- disagrees with the parities: the contraction
    must report the rung as inconsistent;
  * "balanced": the whole undirected strong graph, one-way edges included, admits one sign assignment: every order of absorbing
    strong edges gives the same signs, so the contraction and the walk over it must succeed at this rung;
  * "undetermined": only one-way edges BETWEEN clusters disagree; whether the walk meets the disagreement depends on directed
    reachability, which this file does not restate -- no counter is asserted then.
"""
import numpy as np

from tmc2_amd.synth import synth_cloud

K = 16
DEFAULT_TAU = 0.98
LADDER = (0.99, 0.995, 0.998)
NO_CONTRACTION_ABOVE = 1.5   # ORIENT_TAU above this: the hook sends the frame straight to the plain growth

# seeds found by search_conflict_seeds() (test_orientation_cases.py checks that they still are the first)
ONE_WAY_CONFLICT = (65, 0.9)   # (seed, ORIENT_TAU)
MUTUAL_CONFLICT = (0, 0.5)

# case name -> facts about its construction that test_orientation_cases.py checks
META = {}


# ---- the classifier ---------------------------------------------------------------------------------------------------------------
def edge_dots(knn, normals):
    """d[u][j] = n_u . n_knn[u][j] as the reference evaluates it: three products, summed left to right, no fused multiply-add."""
    a = normals[:, None, :]
    b = normals[knn]
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def mutual_mask(knn):
    """m[u][j]: knn[u][j] lists u back."""
    n = len(knn)
    out = np.zeros(knn.shape, bool)
    for j in range(knn.shape[1]):                                   # (one column at a time: n * 16 words of scratch, not n * 256)
        out[:, j] = (knn[knn[:, j]] == np.arange(n, dtype=knn.dtype)[:, None]).any(1)
    return out


class _ParityForest:
    """union-find with parity, plain loops"""

    def __init__(self, n):
        self.parent = list(range(n))
        self.par = [0] * n

    def find(self, x):
        parent, par = self.parent, self.par
        r, p = x, 0
        while parent[r] != r:
            p ^= par[r]
            r = parent[r]
        q = p
        while parent[x] != x:                                        # compress: everything on the path points at the root
            nxt, step = parent[x], par[x]
            parent[x], par[x] = r, q
            q ^= step
            x = nxt
        return r, p

    def union(self, u, v, s):
        """u and v must differ in sign iff s; False if they are joined already the other way round"""
        ru, pu = self.find(u)
        rv, pv = self.find(v)
        if ru == rv:
            return (pu ^ pv) == s
        self.parent[ru] = rv
        self.par[ru] = pu ^ pv ^ s
        return True


def analyse(knn, normals, tau):
    """The facts about one rung: how many strong edges of each kind disagree, and the clusters."""
    n = len(knn)
    d = edge_dots(knn, normals)
    strong = (np.abs(d) >= tau) & (d != 0.0)        # (a dot product of exactly zero relates no two signs: never strong)
    mutual = mutual_mask(knn)
    src = np.broadcast_to(np.arange(n, dtype=np.int64)[:, None], knn.shape)
    forest = _ParityForest(n)
    mutual_bad = 0
    sel = strong & mutual & (knn < src)                              # every mutual edge once, self edges never
    for u, v, s in zip(src[sel].tolist(), knn[sel].tolist(), (d[sel] < 0.0).tolist()):
        mutual_bad += not forest.union(u, v, int(s))
    found = [forest.find(i) for i in range(n)]
    root = np.array([f[0] for f in found], np.int64)
    par = np.array([f[1] for f in found], np.int64)
    neg = (d < 0.0).astype(np.int64)
    inside = root[knn] == root[:, None]
    wrong = strong & inside & ((par[:, None] ^ par[knn]) != neg)
    one_way_bad = int((wrong & ~mutual).sum())
    mutual_bad += int((wrong & mutual).sum())
    cross_bad = 0
    if mutual_bad == 0:                                              # do the strong edges BETWEEN clusters admit one sign assignment?
        sel = strong & ~inside
        for u, v, s in zip(src[sel].tolist(), knn[sel].tolist(), neg[sel].tolist()):
            cross_bad += not forest.union(u, v, s)
    return {"d": d, "strong": strong, "root": root, "parity": par, "mutual_bad": mutual_bad, "one_way_bad": one_way_bad,
            "cross_bad": cross_bad}


def classify(knn, normals, tau):
    a = analyse(knn, normals, tau)
    if a["mutual_bad"] or a["one_way_bad"]:
        return "conflict"
    return "undetermined" if a["cross_bad"] else "balanced"


def ladder(first_tau):
    return [first_tau] + [t for t in LADDER if t > first_tau]


def expected_path(knn, normals, first_tau=DEFAULT_TAU):
    """(orient_tau_retry, orient_normals_regrowth) the counters must show, or None where a rung's outcome is not decided by the
    classifier (or the hook switches the contraction off)."""
    if first_tau > NO_CONTRACTION_ABOVE:
        return None
    rungs = ladder(first_tau)
    for retries, tau in enumerate(rungs):
        verdict = classify(knn, normals, tau)
        if verdict == "balanced":
            return retries, 0
        if verdict == "undetermined":
            return None
    return len(rungs) - 1, 1


def final_tau(knn, normals, first_tau=DEFAULT_TAU):
    """the rung the contraction succeeds at, or None (as expected_path: None also where it cannot tell)"""
    path = expected_path(knn, normals, first_tau)
    return None if path is None or path[1] else ladder(first_tau)[path[0]]


def _cross_edges(knn, normals, tau):
    a = analyse(knn, normals, tau)
    assert a["mutual_bad"] == 0 and a["one_way_bad"] == 0, "no contraction at this threshold"
    root, par, d = a["root"], a["parity"], a["d"]
    cu = np.broadcast_to(root[:, None], knn.shape)
    cv = root[knn]
    cross = cu != cv
    key = cu[cross] * len(knn) + cv[cross]                           # the ordered pair of clusters
    cls = ((d[cross] < 0.0).astype(np.int64) ^ np.broadcast_to(par[:, None], knn.shape)[cross] ^ par[knn][cross])
    return len(np.unique(root)), key, np.abs(d[cross]), a["strong"][cross], cls


def cross_pairs(knn, normals, tau):
    """distinct ordered pairs of clusters joined by an edge: what the device's pair table must hold"""
    return len(np.unique(_cross_edges(knn, normals, tau)[1]))


def compact_size(knn, normals, tau):
    """(clusters, edges) of the compact graph: per ordered pair of clusters the light edges that tie at the pair's largest
    |n_u . n_v|, and one strong edge per implied relative sign"""
    clusters, key, w, strong, cls = _cross_edges(knn, normals, tau)
    edges = len(np.unique(key[strong] * 2 + cls[strong]))
    if (~strong).any():
        uniq, inv = np.unique(key[~strong], return_inverse=True)
        best = np.full(len(uniq), -1.0)
        np.maximum.at(best, inv, w[~strong])
        edges += int((w[~strong] == best[inv]).sum())
    return clusters, edges


# ---- the clouds -------------------------------------------------------------------------------------------------------------------
def _unit(v):
    return v / np.linalg.norm(v, axis=1)[:, None]


def _moebius_band():
    """A closed band round the z axis, three layers thick; the normal turns half a turn on the way round, so every cycle round the
    band is frustrated however tight the threshold: the seam's edges are as strong as any and negative."""
    rng = np.random.default_rng(4101)
    th = np.arange(900) * (2 * np.pi / 900)
    ring = np.unique(np.stack([np.rint(512 + 130 * np.cos(th)), np.rint(512 + 130 * np.sin(th))], 1).astype(np.int64), axis=0)
    xyz = np.concatenate([np.concatenate([ring, np.full((len(ring), 1), z)], 1) for z in (40, 41, 42)])
    xyz = xyz[rng.permutation(len(xyz))]
    ang = np.mod(np.arctan2(xyz[:, 1] - 512.0, xyz[:, 0] - 512.0), 2 * np.pi)
    nrm = np.stack([np.cos(ang / 2) * np.cos(ang), np.cos(ang / 2) * np.sin(ang), np.sin(ang / 2)], 1)
    return xyz.astype(np.int16), nrm


def _moebius_short():
    """40 rings of N = 17 .. 22 points, 100 apart.  Point i of a ring carries cos(a_i) e_x + sin(a_i) e_z with a_i = pi i / N:
    neighbours on the ring meet at cos(pi / N), in [0.98, 0.99); the seam at -cos(pi / N); next-nearest at cos(2 pi / N) < 0.96.
    (A fixed frame instead of the band's e_r, so that the dot product of two ring neighbours is cos(pi / N) and nothing else.)"""
    rng = np.random.default_rng(4102)
    pts, nrm, rings = [], [], []
    for r in range(40):
        N = 17 + r % 6
        th = np.arange(N) * (2 * np.pi / N)
        c = np.array([60 + 100 * (r % 8), 60 + 100 * (r // 8), 60 + 7 * r])
        pts.append(np.stack([np.rint(c[0] + 12 * np.cos(th)), np.rint(c[1] + 12 * np.sin(th)), np.full(N, c[2])], 1))
        nrm.append(np.stack([np.cos(th / 2), np.zeros(N), np.sin(th / 2)], 1))
        rings += [r] * N
    pts, nrm, rings = np.concatenate(pts), np.concatenate(nrm), np.array(rings)
    order = rng.permutation(len(pts))
    META["moebius_short"] = {"ring": rings[order]}
    return pts[order].astype(np.int16), nrm[order]


def _islands():
    """64 clumps of 17 .. 48 points in 4 x 4 x 4 cells, 200 apart, and up to three satellites 24 off a clump's corner: a satellite
    lists itself and 15 points of its clump, nobody lists it.  In shuffled order: a satellite is a seed of its own, before its clump
    (the point-before-the-seed branch, or the view point for point 0) or after it (every neighbour oriented already)."""
    rng = np.random.default_rng(4103)
    pts, clump, sat = [], [], []
    cells = np.stack(np.meshgrid(np.arange(4), np.arange(4), np.arange(4), indexing="ij"), -1).reshape(-1, 3)
    for c in range(64):
        corner = np.array([40 + 200 * (c % 4), 40 + 200 * ((c // 4) % 4), 40 + 200 * (c // 16)])
        m = int(rng.integers(17, 49))
        body = corner + cells[rng.permutation(64)[:m]]
        sats = [corner + off for off in ([24, 1, 2], [1, 24, 2], [2, 1, 24])][:int(rng.integers(0, 4))]
        pts += list(body) + sats
        clump += [c] * (m + len(sats))
        sat += [False] * m + [True] * len(sats)
    order = rng.permutation(len(pts))
    META["islands"] = META["islands_random_signs"] = {"clump": np.array(clump)[order], "satellite": np.array(sat)[order]}
    return np.array(pts)[order].astype(np.int16)


MAJORITY_NEGATIVES = (20, 300, 2100)      # one block; three blocks; more wavefronts than the 64 folded counters


def _majority(m, n, seed):
    """n - m points on the plane z = 0 (n . (0 - p) is exactly 0 for n = (0, 0, +-1): they count on neither side) and m on z = 3;
    point 0 is on z = 0 and carries +z, so the growth turns every normal to +z and exactly the m points on z = 3 look away from the
    origin.  The reference flips everything iff m > (n + 1) / 2."""
    rng = np.random.default_rng(seed)
    side = int(np.ceil(np.sqrt(max(m, n - m))))
    grid = np.stack(np.meshgrid(np.arange(side), np.arange(side), indexing="ij"), -1).reshape(-1, 2) + 100
    xyz = np.concatenate([np.concatenate([grid[:n - m], np.zeros((n - m, 1), np.int64)], 1),
                          np.concatenate([grid[:m], np.full((m, 1), 3)], 1)])
    nrm = np.zeros((n, 3))
    nrm[:, 2] = rng.choice([-1.0, 1.0], n)
    nrm[0, 2] = 1.0
    return xyz.astype(np.int16), nrm


def majority_members():
    """(name, negatives m, points n, flips): per m the four sizes round the boundary -- n = 2m - 1 and 2m put m exactly at (n + 1) / 2
    (odd and even n: no flip), n = 2m - 3 and 2m - 2 put it one over (odd and even: flip)."""
    return [("majority_m%d_n%d" % (m, n), m, n, m > (n + 1) // 2) for m in MAJORITY_NEGATIVES for n in (2 * m - 3, 2 * m - 2, 2 * m - 1, 2 * m)]


PALETTE = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [0.6, 0.8, 0], [0.8, 0.6, 0], [0.6, 0, 0.8], [0.8, 0, 0.6], [0, 0.6, 0.8],
                    [0, 0.8, 0.6], [-0.6, 0.8, 0], [0.6, 0, -0.8], [0, -0.6, 0.8]], np.float64)


def _cell_hash(xyz):
    c = (xyz.astype(np.int64) >> 4)
    h = ((c[:, 0] * 73856093) ^ (c[:, 1] * 19349663) ^ (c[:, 2] * 83492791)) & 0xFFFFFFFF
    h = ((h ^ (h >> 16)) * 0x7FEB352D) & 0xFFFFFFFF
    h = ((h ^ (h >> 15)) * 0x846CA68B) & 0xFFFFFFFF
    return h ^ (h >> 16)


def conflict_cloud(seed):
    """the noisy tiny body at a height of 25 voxels, ~850 points: at 0.9 its mutual strong edges mostly agree while a few one-way
    ones inside the clusters do not (the full-height body has mutual disagreements at every seed)"""
    return synth_cloud("tiny_noisy", seed=seed, height=25)[0]


def follows_one_way_edge(knn, a, oriented):
    """the reference's growth took a one-way edge first: two points joined by a mutual strong edge came out against each other"""
    return bool((a["strong"] & mutual_mask(knn) & (edge_dots(knn, oriented) < 0.0)).any())


def search_conflict_seeds(oracle, seeds=range(80), taus=(0.5, 0.9)):
    """The first (seed, tau) of a noisy tiny cloud whose ONLY disagreement at its first rung is one-way strong edges inside a cluster
    -- the mutual edges agree, the edges between clusters agree -- and whose growth FOLLOWS such an edge, so that the reference orients
    points against their cluster (the stand-in for the frame that broke round 4: a contraction that overlooks the edge gives other
    normals); and the first whose mutual strong edges disagree."""
    one_way = mutual = None
    for seed in seeds:
        xyz = conflict_cloud(seed)
        knn = oracle.knn_self(xyz, K)
        raw = oracle.compute_normals(xyz, knn)
        for tau in taus:
            a = analyse(knn, raw, tau)
            if (one_way is None and a["one_way_bad"] and not a["mutual_bad"] and not a["cross_bad"] and
                    follows_one_way_edge(knn, a, oracle.orient_normals(xyz, knn, raw))):
                one_way = (seed, tau)
            if mutual is None and a["mutual_bad"]:
                mutual = (seed, tau)
        if one_way and mutual:
            break
    return one_way, mutual


def cases(oracle):
    """(name, xyz, normals); xyz int16 [n][3], normals float64 [n][3]"""
    def pca(xyz):
        return oracle.compute_normals(xyz, oracle.knn_self(xyz, K))

    body = synth_cloud("tiny")[0]
    raw = pca(body)
    n = len(body)
    rng = np.random.default_rng(4100)
    yield "pca", body, raw
    yield "pca_random_signs", body, raw * rng.choice([-1.0, 1.0], n)[:, None]
    yield "constant", body, np.tile([0.0, 0.0, 1.0], (n, 1))
    yield "alternating", body, np.stack([np.zeros(n), np.zeros(n), 1.0 - 2.0 * (np.arange(n) % 2)], 1)
    yield "palette", body, PALETTE[_cell_hash(body) % len(PALETTE)]
    yield "zeros", body, np.zeros((n, 3))
    slab = (body[:, 1] > np.percentile(body[:, 1], 40)) & (body[:, 1] < np.percentile(body[:, 1], 60))
    yield "half_zeros", body, np.where(slab[:, None], 0.0, raw)
    yield "scaled", body, raw * 3.0
    yield "random", body, _unit(rng.normal(size=(n, 3)))
    noisy = synth_cloud("tiny_noisy")[0]
    yield "noisy", noisy, pca(noisy)
    band, twist = _moebius_band()
    yield "moebius", band, twist
    yield "moebius_scaled", band, twist * 3.0                      # (|n_u . n_v| ~ 9: strong at ANY finite threshold the ladder ends with)
    yield ("moebius_short",) + _moebius_short()
    isl = _islands()
    isl_raw = pca(isl)
    yield "islands", isl, isl_raw
    yield "islands_random_signs", isl, isl_raw * rng.choice([-1.0, 1.0], len(isl))[:, None]
    for m in (17, 31, 255, 256, 257, 4097):
        yield "sizes_%d" % m, body[:m], pca(body[:m])
    dup = np.concatenate([body, body[::10]])
    dup = dup[rng.permutation(len(dup))]
    yield "duplicates", dup, pca(dup)
    for name, m, nn, _ in majority_members():
        yield (name,) + _majority(m, nn, 4200 + nn)
    for name, found in (("one_way_conflict", ONE_WAY_CONFLICT), ("mutual_conflict", MUTUAL_CONFLICT)):
        cloud = conflict_cloud(found[0])
        yield name, cloud, pca(cloud)


CONFLICT_TAU = {"one_way_conflict": ONE_WAY_CONFLICT[1], "mutual_conflict": MUTUAL_CONFLICT[1]}   # the first rung each shows at


class Case:
    """One case with what every test needs of it, each computed once per session."""

    def __init__(self, oracle, name, xyz, normals):
        self.name, self.xyz, self.normals = name, np.ascontiguousarray(xyz), np.ascontiguousarray(normals, np.float64)
        self.knn = oracle.knn_self(self.xyz, K)
        self.expected = oracle.orient_normals(self.xyz, self.knn, self.normals)
        self._memo = {}

    def _once(self, key, fn):
        if key not in self._memo:
            self._memo[key] = fn()
        return self._memo[key]

    def classify(self, tau):
        return self._once(("c", tau), lambda: classify(self.knn, self.normals, tau))

    def path(self, tau=DEFAULT_TAU):
        return self._once(("p", tau), lambda: expected_path(self.knn, self.normals, tau))

    def final_tau(self, tau=DEFAULT_TAU):
        return self._once(("f", tau), lambda: final_tau(self.knn, self.normals, tau))

    def cross_pairs(self, tau):
        return self._once(("x", tau), lambda: cross_pairs(self.knn, self.normals, tau))

    def compact_size(self, tau):
        return self._once(("s", tau), lambda: compact_size(self.knn, self.normals, tau))


_CASES = {}


def all_cases(oracle):
    """name -> Case, built once"""
    if not _CASES:
        for name, xyz, normals in cases(oracle):
            _CASES[name] = Case(oracle, name, xyz, normals)
    return _CASES


def case_names():
    """the names cases() yields, without building anything (for parametrize)"""
    return (["pca", "pca_random_signs", "constant", "alternating", "palette", "zeros", "half_zeros", "scaled", "random", "noisy",
             "moebius", "moebius_scaled", "moebius_short", "islands", "islands_random_signs"] +
            ["sizes_%d" % m for m in (17, 31, 255, 256, 257, 4097)] + ["duplicates"] + [m[0] for m in majority_members()] +
            ["one_way_conflict", "mutual_conflict"])
