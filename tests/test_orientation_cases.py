"""CPU tier for the hand-built orientation cases (orientation_cases.py): the construction claims each case rests on, the
classifier on graphs small enough to read, and the host orientation against the oracle's growth, bit for bit.  The same cases
run on the device in test_gpu_orientation.py; what that file asserts about counters is shown to be live here."""
import numpy as np
import pytest

import orientation_cases as oc
import tmc2_amd as T

NAMES = oc.case_names()
TAUS = ["0.0", "0.5", "0.9", "0.9999", "1.0", "1.5", "1.6", "4"]
TAU_CASES = ["pca", "noisy", "palette", "random", "islands", "one_way_conflict", "mutual_conflict"]
HOOK_CASES = ["pca", "palette", "random", "noisy", "islands", "moebius_short"]
SIGN = np.uint64(1) << np.uint64(63)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def assert_signs_only(out, field):
    """every normal comes back as it went in or with all three sign bits turned, nothing else"""
    same = (bits(out) == bits(field)).all(1)
    turned = (bits(out) == (bits(field) ^ SIGN)).all(1)
    assert (same | turned).all()


@pytest.fixture(scope="module")
def cases(oracle):
    return oc.all_cases(oracle)


def test_case_list(cases):
    assert list(cases) == NAMES and len(set(NAMES)) == len(NAMES)


# ---- the classifier on graphs one can read --------------------------------------------------------------------------------------
def _planar(deg):
    a = np.radians(np.asarray(deg, np.float64))
    return np.stack([np.cos(a), np.sin(a), np.zeros(len(a))], 1)


def test_classifier_on_toy_graphs():
    tri = np.array([[0, 1, 2], [1, 0, 2], [2, 0, 1]], np.uint32)     # three points that all list each other
    n = _planar([0, 70, 140])                                        # dots: 0.34, 0.34, -0.77
    assert oc.classify(tri, n, 0.3) == "conflict"                    # a frustrated mutual triangle
    assert oc.classify(tri, n, 0.5) == "balanced"                    # only the negative edge is strong
    assert oc.expected_path(tri, n, 0.3) == (1, 0) and oc.expected_path(tri, n, 0.0) == (1, 0)
    e = np.array([[1.0, 0, 0], [0.6, 0.8, 0], [-1.0, 0, 0]])         # dots: 0.6, -0.6, -1 -- clusters {0, 2} and {1} at 0.9
    assert oc.classify(tri, e, 0.9) == "balanced" and oc.cross_pairs(tri, e, 0.9) == 2
    assert oc.compact_size(tri, e, 0.9) == (2, 4)                    # both light edges of either pair tie at 0.6: both are kept
    # two mutual pairs {0, 1} and {2, 3}; the one-way edges 0 -> 2 (+) and 1 -> 3 (-) between them disagree
    two = np.array([[0, 1, 2], [1, 0, 3], [2, 3, 1], [3, 2, 0]], np.uint32)
    m = _planar([0, 80, -80, -160])
    a = oc.analyse(two, m, 0.1)
    assert (a["mutual_bad"], a["one_way_bad"]) == (0, 0) and a["cross_bad"] > 0
    assert oc.classify(two, m, 0.1) == "undetermined" and oc.expected_path(two, m, 0.1) is None
    # a chain 0 - 1 - 2 - 3 of mutual edges (0.77 each) is one cluster; 0 -> 3 is one-way, strong at 0.4 and negative
    one = np.array([[0, 1, 3], [1, 0, 2], [2, 1, 3], [3, 2, 1]], np.uint32)
    b = oc.analyse(one, _planar([0, 40, 80, 120]), 0.4)
    assert (b["mutual_bad"], b["one_way_bad"]) == (0, 1) and oc.classify(one, _planar([0, 40, 80, 120]), 0.4) == "conflict"
    assert oc.classify(one, _planar([0, 40, 80, 120]), 0.6) == "balanced"
    # an exactly zero dot product is never strong, not even at threshold 0: it says nothing about the two signs
    z = np.array([[1.0, 0, 0], [0, 1.0, 0], [0, 0, 0]])
    assert not oc.analyse(tri, z, 0.0)["strong"][0, 1] and oc.analyse(tri, z, 0.0)["strong"][0, 0]
    assert oc.ladder(0.98) == [0.98, 0.99, 0.995, 0.998] and oc.ladder(0.995) == [0.995, 0.998] and oc.ladder(4.0) == [4.0]
    assert oc.expected_path(tri, n, 1.6) is None


# ---- what each case claims about itself ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_case_shape(cases, name):
    c = cases[name]
    n = len(c.xyz)
    assert c.xyz.dtype == np.int16 and c.xyz.shape == (n, 3) and c.normals.shape == (n, 3) and np.isfinite(c.normals).all()
    assert 17 <= n <= {"noisy": 11000, "duplicates": 7200}.get(name, 6500)
    assert c.xyz.min() >= 0 and c.xyz.max() < 1024
    distinct = len(np.unique(c.xyz, axis=0))
    assert n - distinct == ((distinct + 9) // 10 if name == "duplicates" else 0)
    assert c.path() is not None, "every case is decided at the default threshold"


def test_default_paths_by_construction(cases):
    for name in ("pca", "constant", "alternating", "random", "zeros", "islands"):
        assert cases[name].path() == (0, 0), name
    assert cases["moebius"].path() == (3, 1) and cases["moebius_scaled"].path() == (3, 1)
    assert cases["moebius_short"].path() == (1, 0)
    assert [cases["moebius"].classify(t) for t in oc.ladder(0.98)] == ["conflict"] * 4


def test_fields_over_the_body(cases):
    body = cases["pca"]
    d = oc.edge_dots(body.knn, cases["constant"].normals)
    assert (d == 1.0).all()
    d = oc.edge_dots(body.knn, cases["alternating"].normals)
    assert (np.abs(d) == 1.0).all() and (d < 0).any()
    assert not cases["zeros"].normals.any()
    hz = cases["half_zeros"].normals
    zero = ~hz.any(1)
    assert 0.1 < zero.mean() < 0.4 and np.array_equal(hz[~zero], body.normals[~zero])
    assert np.abs(oc.edge_dots(body.knn, cases["scaled"].normals)).max() > 8.9
    assert np.array_equal(np.abs(cases["pca_random_signs"].normals), np.abs(body.normals))
    assert not np.array_equal(cases["pca_random_signs"].normals, body.normals)
    r = cases["random"].normals
    assert np.allclose((r * r).sum(1), 1.0, rtol=0, atol=1e-12)
    clusters, _ = cases["random"].compact_size(0.98)
    assert clusters > 0.8 * len(r) and cases["random"].cross_pairs(0.98) > 12 * len(r)


def test_palette_ties(cases):
    """about a dozen exact unit vectors: the weights of the cross edges are a handful of values, so the best light edge of a pair
    of clusters is usually SEVERAL edges that tie -- all of which the compact graph has to keep"""
    c = cases["palette"]
    used = np.unique(c.normals, axis=0)
    assert len(oc.PALETTE) == 12 and len(used) >= 10 and all((oc.PALETTE == u).all(1).any() for u in used)
    w = np.unique(np.round(np.abs(oc.edge_dots(c.knn, c.normals)), 12))
    assert set(w) <= {0.0, 0.28, 0.36, 0.48, 0.6, 0.64, 0.8, 0.96, 1.0} and {0.0, 0.28, 0.6, 0.8, 0.96} <= set(w)
    tau = c.final_tau()
    _, key, _, strong, cls = oc._cross_edges(c.knn, c.normals, tau)
    kept_light = c.compact_size(tau)[1] - len(np.unique(key[strong] * 2 + cls[strong]))
    assert kept_light > len(np.unique(key[~strong])) + 100, "pairs of clusters whose best light edges tie are common"


def test_moebius_band(cases):
    c = cases["moebius"]
    assert len(np.unique(c.xyz, axis=0)) == len(c.xyz) >= 1200
    a = oc.analyse(c.knn, c.normals, 0.998)
    assert a["strong"].all(), "every neighbour edge is strong at the last rung"
    assert (a["d"] < 0).any() and a["mutual_bad"] > 0                # the seam: strong, negative, and part of mutual cycles
    assert np.array_equal(cases["moebius_scaled"].normals, c.normals * 3.0)
    assert np.abs(oc.edge_dots(c.knn, c.normals * 3.0)).min() > 4.0  # strong at any threshold the ladder could end with


def test_moebius_short_rings(cases):
    c = cases["moebius_short"]
    ring = oc.META["moebius_short"]["ring"]
    sizes = np.bincount(ring)
    assert len(sizes) == 40 and sizes.min() == 17 and sizes.max() == 22
    assert (ring[c.knn] == ring[:, None]).all(), "the rings are far apart: a point's neighbours are its ring"
    for N in range(17, 23):
        assert 0.98 <= np.cos(np.pi / N) < 0.99 and np.cos(2 * np.pi / N) < 0.96
    self_edge = c.knn == np.arange(len(c.knn), dtype=np.uint32)[:, None]
    a = oc.analyse(c.knn, c.normals, 0.98)
    assert (a["strong"] & ~self_edge).sum() == 2 * len(ring)         # each point: its two ring neighbours, nothing else
    assert a["mutual_bad"] > 0 and a["one_way_bad"] == 0
    assert not (oc.analyse(c.knn, c.normals, 0.99)["strong"] & ~self_edge).any()


@pytest.mark.parametrize("name", ["islands", "islands_random_signs"])
def test_islands(cases, name):
    c = cases[name]
    clump, sat = oc.META[name]["clump"], oc.META[name]["satellite"]
    sizes = np.bincount(clump[~sat])
    assert len(sizes) == 64 and sizes.min() >= 17 and sizes.max() <= 48
    assert (clump[c.knn] == clump[:, None]).all()
    listed = np.zeros(len(c.xyz), bool)
    rows = np.broadcast_to(np.arange(len(c.xyz))[:, None], c.knn.shape)
    listed[c.knn[c.knn != rows]] = True
    assert sat.sum() >= 40 and not listed[sat].any(), "nobody lists a satellite"
    first = np.array([np.nonzero(clump == k)[0].min() for k in range(64)])
    before = sat & (np.arange(len(sat)) == first[clump])             # satellites that open their clump: no oriented neighbour
    assert before.sum() >= 3 and (sat & ~before).sum() >= 20
    assert np.array_equal(np.abs(cases["islands"].normals), np.abs(c.normals))


def test_sizes_and_duplicates(cases):
    body = cases["pca"].xyz
    for m in (17, 31, 255, 256, 257, 4097):
        assert np.array_equal(cases["sizes_%d" % m].xyz, body[:m])
    dup = cases["duplicates"].xyz
    assert len(dup) == len(body) + (len(body) + 9) // 10


@pytest.mark.parametrize("name,m,n,flips", oc.majority_members())
def test_majority_boundary(cases, name, m, n, flips):
    c = cases[name]
    assert len(c.xyz) == n and set(np.unique(c.xyz[:, 2])) == {0, 3} and not c.normals[:, :2].any()
    assert (np.abs(c.normals[:, 2]) == 1.0).all() and c.xyz[0, 2] == 0 and c.normals[0, 2] == 1.0
    grown = np.tile([0.0, 0.0, 1.0], (n, 1))                         # the growth turns every normal the way point 0 looks
    negatives = int(((grown * (0.0 - c.xyz.astype(np.float64))).sum(1) < 0.0).sum())
    assert negatives == m == (n + 1) // 2 + (1 if flips else 0)      # exactly at the bound, or one over
    assert (c.expected[:, 2] == (-1.0 if flips else 1.0)).all()


def test_majority_family_covers_both_parities():
    seen = {(n % 2, flips) for _, _, n, flips in oc.majority_members()}
    assert seen == {(0, False), (0, True), (1, False), (1, True)}


def test_conflict_seeds(cases, oracle):
    one, mut = cases["one_way_conflict"], cases["mutual_conflict"]
    a = oc.analyse(one.knn, one.normals, oc.CONFLICT_TAU["one_way_conflict"])
    assert (a["mutual_bad"], a["cross_bad"]) == (0, 0) and a["one_way_bad"] >= 1, "only one-way strong edges inside clusters disagree"
    assert oc.follows_one_way_edge(one.knn, a, one.expected), "and the reference follows one: points end up against their cluster"
    assert oc.analyse(mut.knn, mut.normals, oc.CONFLICT_TAU["mutual_conflict"])["mutual_bad"] >= 1
    assert one.path(oc.CONFLICT_TAU["one_way_conflict"]) == (1, 0)
    assert mut.path(oc.CONFLICT_TAU["mutual_conflict"]) is not None and mut.path(oc.CONFLICT_TAU["mutual_conflict"])[0] >= 1
    assert oc.search_conflict_seeds(oracle) == (oc.ONE_WAY_CONFLICT, oc.MUTUAL_CONFLICT)


def test_gpu_counter_assertions_are_live(cases):
    """what test_gpu_orientation.py asserts about counters, derived here without a GPU: every figure it waits for occurs"""
    paths = {cases[name].path() for name in NAMES}
    assert (3, 1) in paths and (1, 0) in paths and (0, 0) in paths
    overflow = repeat = fits = 0
    for name in HOOK_CASES:
        c = cases[name]
        tau = c.final_tau()
        assert tau is not None, name
        overflow += sum(c.cross_pairs(tau) > cap for cap in (16, 256))
        clusters, edges = c.compact_size(tau)
        repeat += sum(edges > e or clusters + 1 > r for e, r in ((64, 16), (1, 2)))
        fits += sum(not (edges > e or clusters + 1 > r) for e, r in ((64, 16), (1, 2)))
    assert overflow >= 8 and repeat >= 8
    decided = sum(cases[name].path(float(t)) is not None for name in TAU_CASES for t in TAUS)
    assert decided >= 30


# ---- the host orientation against the oracle's growth ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_host_orientation_matches_oracle(cases, name):
    c = cases[name]
    got = T.host_orient_normals(c.xyz, c.knn, c.normals)
    assert_signs_only(c.expected, c.normals)
    assert np.array_equal(bits(got), bits(c.expected))


@pytest.mark.parametrize("tau", TAUS)
@pytest.mark.parametrize("name", TAU_CASES)
def test_host_orientation_thresholds(cases, monkeypatch, name, tau):
    """(the host-only entry has no context: it reads its options from the environment, at every call)"""
    c = cases[name]
    monkeypatch.setenv("TMC2_ORIENT_TAU", tau)
    assert np.array_equal(bits(T.host_orient_normals(c.xyz, c.knn, c.normals)), bits(c.expected))
