"""Inputs and plain references for the shared device primitives (tmc2_selftest_*: csrc/selftest.hip): the exclusive scan, the
several-regions fill, the XCD work mapping, the two union-finds (S7's kernels over a 16-neighbour table; explicit edge lists, with
and without parity), CandSort, the marked cells of a boundary-cell grid and the cross-lane idioms of csrc/wave.h.  numpy only.  tests/test_primitive_cases.py checks the references themselves (every graph family
has a component count known in closed form); tests/test_gpu_primitives.py compares the device with them, integer for integer."""
import functools

import numpy as np

K = 16                                  # neighbours per row of S7's table
UF_MULTIPLIER = 2654435761              # ufPriority (csrc/union_find.h): x * 2654435761 mod 2^32, a bijection


# ---- scan ---------------------------------------------------------------------------------------------------------------
SCAN_SIZES = (0, 1, 7, 8, 9, 2047, 2048, 2049, 4096, 131072, 131073, 133121, 264197, 1000003)
SCAN_PATTERNS = ("zero", "one", "flags", "counts", "first", "last", "max")


def scan_input(pattern, n, seed=0):
    rng = np.random.default_rng([seed, n, SCAN_PATTERNS.index(pattern)])
    if pattern == "zero":
        return np.zeros(n, np.uint32)
    if pattern == "one":
        return np.ones(n, np.uint32)
    if pattern == "flags":
        return rng.integers(0, 2, n, dtype=np.uint32)
    if pattern == "counts":
        return rng.integers(0, 1 << 16, n, dtype=np.uint32)
    if pattern == "max":                                        # the sums wrap modulo 2^32, as the reference's do
        return np.full(n, 0xFFFFFFFF, np.uint32)
    a = np.zeros(n, np.uint32)
    if n:
        a[0 if pattern == "first" else n - 1] = 0x89ABCDEF
    return a


def scan_reference(a):
    """(exclusive prefix sums, total) of uint32 modulo 2^32: np.cumsum in uint32, shifted by one"""
    a = np.asarray(a, np.uint32)
    inc = np.cumsum(a, dtype=np.uint32)
    out = np.zeros(len(a), np.uint32)
    out[1:] = inc[:-1]
    return out, np.uint32(inc[-1] if len(a) else 0)


# ---- fill ---------------------------------------------------------------------------------------------------------------
FILL_GUARD = 0xA5
FILL_LENGTHS = tuple(range(41)) + (16383, 16384, 16385, 32769, 100003)


def fill_layout(gap=80):
    """Every head offset 0..15 x every length, laid out in ONE buffer of guard bytes: [(start, length, value)], total bytes.  A
    region starts `head` bytes into a 16-byte line; at least `gap` guard bytes lie between two regions."""
    regions, at = [], 256
    for head in range(16):
        for i, length in enumerate(FILL_LENGTHS):
            at = (at + 15) // 16 * 16 + head
            value = 1 + 37 * len(regions) % 251                # (any twelve regions in a row: twelve values)
            if value == FILL_GUARD:
                value = 252
            regions.append((at, length, value))
            at += length + gap
    return regions, at + 256


def fill_reference(total, regions):
    buf = np.full(total, FILL_GUARD, np.uint8)
    for start, length, value in regions:
        buf[start:start + length] = value
    return buf


# ---- work map -----------------------------------------------------------------------------------------------------------
WORK_GRIDS = tuple(range(8, 65, 8)) + (1024,)
WORK_GRIDS_UNCHUNKED = (1, 7, 9, 1001)


def work_sizes(grid, threads):
    """n: a full grid, one short of it, one past the last full block of an eighth, 1, 0"""
    full = grid * threads
    eighth = max(grid // 8, 1) * threads
    return sorted({full, full - 1, min(full, eighth + 1), 1, 0})


def work_map_reference(grid, live=0):
    """logical block of every workgroup (0xFFFFFFFF: a surplus block of the live form leaves)"""
    b = np.arange(grid, dtype=np.int64)
    if live:
        per = (live + 7) // 8
        lg = (b % 8) * per + b // 8
        return np.where(b // 8 < per, lg, 0xFFFFFFFF).astype(np.uint32)
    if grid % 8:
        return b.astype(np.uint32)
    return ((b % 8) * (grid // 8) + b // 8).astype(np.uint32)


# ---- union-find references ----------------------------------------------------------------------------------------------
def uf_priority(x):
    return ((np.asarray(x, np.uint64) * UF_MULTIPLIER) & 0xFFFFFFFF).astype(np.uint32)


def components(n, a, b):
    """label[u] = the smallest member of u's component under the undirected edges (a[i], b[i]): a sequential union-find, path
    halving, the smaller root wins"""
    parent = list(range(n))
    for u, v in zip(np.asarray(a).tolist(), np.asarray(b).tolist()):
        while parent[u] != u:
            parent[u] = parent[parent[u]]
            u = parent[u]
        while parent[v] != v:
            parent[v] = parent[parent[v]]
            v = parent[v]
        if u < v:
            parent[v] = u
        elif v < u:
            parent[u] = v
    label = np.empty(n, np.int64)
    for u in range(n):                   # parents have smaller indices: one pass in index order settles everything
        label[u] = u if parent[u] == u else label[parent[u]]
    return label


def components_by_sweeps(n, a, b):
    """the same labels by another road (min-label propagation to the fixpoint, with pointer jumping): checks `components`"""
    a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
    label = np.arange(n, dtype=np.int64)
    while True:
        new = label.copy()
        np.minimum.at(new, a, label[b])
        np.minimum.at(new, b, label[a])
        new = new[new]
        if np.array_equal(new, label):
            return label
        label = new


def same_partition(label, root, members=None):
    """root (the device's) and label (the reference's, smallest member) describe ONE partition of `members`: root is constant on
    every component, and the root of u lies in u's component -- so two elements share a root exactly when they share a label"""
    label, root = np.asarray(label, np.int64), np.asarray(root, np.int64)
    m = np.arange(len(label)) if members is None else np.asarray(members)
    if len(m) == 0:
        return True
    r = root[m]
    if r.min() < 0 or r.max() >= len(label):
        return False
    return bool(np.array_equal(root[label[m]], r) and np.array_equal(label[r], label[m]))


# ---- S7's kernels: 16-neighbour tables ------------------------------------------------------------------------------------
GRAPH_FAMILIES = ("path", "path_perm", "tree16", "grid", "groups", "twice", "one_way", "two_paths")


def _table(n, columns):
    """rows padded with the point itself (which the mask kernel skips); a column entry < 0 or >= n is 'no neighbour'"""
    t = np.tile(np.arange(n, dtype=np.int64)[:, None], (1, K))
    for j, c in enumerate(columns):
        c = np.asarray(c, np.int64)
        ok = (c >= 0) & (c < n)
        t[ok, j] = c[ok]
    return t.astype(np.uint32)


def graph_table(family, n, seed=0):
    """(knn [n][16], the number of components it has while every point is raw and of one plane)"""
    i = np.arange(n, dtype=np.int64)
    if family == "path":
        return _table(n, [i - 1, i + 1]), 1
    if family == "path_perm":
        p = np.random.default_rng([seed, n, 1]).permutation(n)
        before, after = np.full(n, -1, np.int64), np.full(n, -1, np.int64)
        before[p[1:]], after[p[:-1]] = p[:-1], p[1:]
        return _table(n, [before, after]), 1
    if family == "tree16":                                       # parent + 15 children: the row is full
        cols = [np.where(i > 0, (i - 1) // 15, -1)] + [15 * i + 1 + c for c in range(15)]
        return _table(n, cols), 1
    if family == "grid":
        w = int(np.ceil(np.sqrt(n)))
        return _table(n, [np.where(i % w > 0, i - 1, -1), np.where(i % w < w - 1, i + 1, -1), i - w, i + w]), 1
    if family == "groups":                                       # of every six points: a pair, a triple (a path), an isolated one
        r, base = i % 6, i - i % 6
        c0 = np.select([r == 0, r == 1, r == 2, r == 3, r == 4], [base + 1, base, base + 3, base + 2, base + 3], -1)
        c1 = np.where(r == 3, base + 4, -1)
        full, rest = divmod(n, 6)
        # the last, cut group: 1 point: itself; 2: the pair; 3: pair + a lone triple head; 4, 5: pair + (part of) the triple
        return _table(n, [c0, c1]), 3 * full + (0, 1, 1, 2, 2, 2)[rest]
    if family == "twice":                                        # a path whose rows list the next point twice
        return _table(n, [i + 1, i - 1, i + 1]), 1
    if family == "one_way":                                      # i lists i + 1, which does not list i: joins nothing
        return _table(n, [i + 1, i + 2, i + 3]), n
    if family == "two_paths":                                    # 0 .. h-1 and h .. n-1, joined by the edge (h-1, n-1) at the last index
        h = n // 2
        a = np.where((i > 0) & (i != h), i - 1, -1)
        b = np.where((i + 1 < n) & (i + 1 != h), i + 1, -1)
        c = np.select([i == h - 1, i == n - 1], [n - 1, h - 1], -1)
        return _table(n, [a, b, c]), 1
    raise ValueError(family)


def graph_cuts(n, seed):
    """random raw = 0 holes (one point in eight) and three planes that cut edges"""
    rng = np.random.default_rng([seed, n, 2])
    return (rng.random(n) >= 0.125).astype(np.uint8), rng.integers(0, 3, n).astype(np.uint8)


def eligible_edges(knn, raw, partition):
    """the edges S7 unites: u != v, each in the other's row, both raw, one plane; each once (u > v)"""
    knn = np.asarray(knn, np.int64)
    n = len(knn)
    u = np.repeat(np.arange(n), K)
    v = knn.reshape(-1)
    listed = np.zeros(len(u), bool)
    for j in range(K):                                           # is u in row v?
        listed |= knn[v, j] == u
    keep = listed & (u > v) & (raw[u] != 0) & (raw[v] != 0) & (partition[u] == partition[v])
    return u[keep], v[keep]


@functools.lru_cache(maxsize=None)
def graph_case(family, n, cut, seed=0):
    """(knn, partition, raw, labels of the reference, component count among the raw points); cached: computed once per session"""
    knn, count = graph_table(family, n, seed)
    raw, partition = graph_cuts(n, seed) if cut else (np.ones(n, np.uint8), np.zeros(n, np.uint8))
    a, b = eligible_edges(knn, raw, partition)
    label = components(n, a, b)
    for x in (knn, raw, partition, label):
        x.setflags(write=False)
    members = np.flatnonzero(raw)
    return knn, partition, raw, label, len(np.unique(label[members]))


# ---- edge lists for UnionFind<false / true> -------------------------------------------------------------------------------
UF_N = 100000
EDGE_FAMILIES = ("star", "repeated", "loops", "path", "path_priority", "random", "cliques")


def edge_list(family, n=UF_N, seed=0):
    """(a, b, component count from the identity forest or None where no closed form exists)"""
    rng = np.random.default_rng([seed, n, 3, EDGE_FAMILIES.index(family)])
    i = np.arange(n, dtype=np.int64)
    if family == "star":                                         # n - 1 leaves on one hub
        hub = n // 3
        leaves = i[i != hub]
        return leaves, np.full(n - 1, hub), 1
    if family == "repeated":                                     # one edge 4 096 times
        return np.full(4096, 5), np.full(4096, n - 7), n - 1
    if family == "loops":
        return i, i, n
    if family == "path":
        return i[:-1], i[1:], 1
    if family == "path_priority":                                # neighbours in priority: every hook races with the next
        o = np.argsort(uf_priority(i), kind="stable")
        return o[:-1], o[1:], 1
    if family == "random":
        return rng.integers(0, n, 2 * n), rng.integers(0, n, 2 * n), None
    if family == "cliques":                                      # 1 000 cliques of 20 random members each
        members = rng.permutation(n)[:20000].reshape(1000, 20)
        ia, ib = np.triu_indices(20, 1)
        return members[:, ia].reshape(-1), members[:, ib].reshape(-1), n - 1000 * 19
    raise ValueError(family)


def hidden_signs(n=UF_N, seed=0):
    return np.random.default_rng([seed, n, 4]).integers(0, 2, n).astype(np.uint32)


def initial_forest(kind, n=UF_N, seed=0, sign=None):
    """(parent, parity-to-parent): 'identity', or 'hooked': every element under a random element at most 8 indices away if that one
    has the smaller priority (the header's rule: links fall in priority), with the true parity sign[x] ^ sign[parent]"""
    i = np.arange(n, dtype=np.int64)
    if kind == "identity":
        return i.copy(), np.zeros(n, np.uint32)
    rng = np.random.default_rng([seed, n, 5])
    other = np.clip(i + rng.integers(-8, 9, n), 0, n - 1)
    prio = uf_priority(i)
    parent = np.where(prio[other] < prio, other, i)
    sign = np.zeros(n, np.uint32) if sign is None else sign
    return parent, (sign ^ sign[parent]).astype(np.uint32)


def forest_words(parent, parity, with_parity):
    return ((parent << 1) | parity).astype(np.uint32) if with_parity else parent.astype(np.uint32)


def word_parents(words, with_parity):
    return (np.asarray(words, np.int64) >> 1) if with_parity else np.asarray(words, np.int64)


def links_fall_in_priority(parent):
    """every link goes to the element itself (a root) or to one of smaller priority"""
    parent = np.asarray(parent, np.int64)
    i = np.arange(len(parent))
    if parent.min() < 0 or parent.max() >= len(parent):
        return False
    return bool(np.all((parent == i) | (uf_priority(parent) < uf_priority(i))))


def parity_consistent(root, root_parity, sign):
    """per component, root_parity[u] ^ sign[u] is one value: that of the root itself, whose parity to itself is 0"""
    root = np.asarray(root, np.int64)
    return bool(np.all(root_parity[root] == 0) and np.array_equal(root_parity ^ sign, sign[root]))


@functools.lru_cache(maxsize=None)
def edge_case(family, forest, seed=0):
    """(a, b, hidden sign, parent0, parity0 under that sign, labels of the reference over edges + forest links)"""
    a, b, _ = edge_list(family, UF_N, seed)
    sign = hidden_signs(UF_N, seed)
    parent, parity = initial_forest(forest, UF_N, seed, sign)
    label = components(UF_N, np.concatenate([a, np.arange(UF_N)]), np.concatenate([b, parent]))
    for x in (a, b, sign, parent, parity, label):
        x.setflags(write=False)
    return a, b, sign, parent, parity, label


# ---- CandSort -----------------------------------------------------------------------------------------------------------
SORT_LENGTHS = tuple(range(18)) + (31, 32, 33, 100)
SORT_KEYS = ("1", "2", "3", "50", "sorted", "reversed", "organ_pipe")
SORT_LONG_KEYS = SORT_KEYS[:-1]


def sort_keys(kind, length, rng):
    if kind in ("1", "2", "3", "50"):
        return rng.integers(0, int(kind), length).astype(np.uint32) * 977 + 3
    up = np.sort(rng.integers(0, max(length // 2, 1), length)).astype(np.uint32)      # (ties within the run, too)
    if kind == "sorted":
        return up
    if kind == "reversed":
        return up[::-1].copy()
    return np.concatenate([up[0::2], up[1::2][::-1]])                                 # rises, then falls


def sort_lists(count=20000, seed=0):
    """(pairs [total][2] = (key, position in its list), offsets [count + 1]): lengths 0..17, 31..33, 100 in turn, the last lists of
    1 000 and 5 000 elements; every key pattern at every length"""
    rng = np.random.default_rng([seed, count, 6])
    lengths = [SORT_LENGTHS[l % len(SORT_LENGTHS)] for l in range(count)]
    kinds = [SORT_KEYS[(l // len(SORT_LENGTHS)) % len(SORT_KEYS)] for l in range(count)]
    # the long ones: each pattern at 1 000 and at 5 000 -- but the organ pipe, which drives libstdc++'s median of three into its
    # depth limit from 1 000 elements on (std::sort turns to heapsort there, which CandSort does not replay: it reports it)
    for t, kind in enumerate(SORT_LONG_KEYS):
        lengths[count - 1 - t], kinds[count - 1 - t] = 1000, kind
        lengths[count - 1 - len(SORT_LONG_KEYS) - t], kinds[count - 1 - len(SORT_LONG_KEYS) - t] = 5000, kind
    offsets = np.zeros(count + 1, np.uint32)
    offsets[1:] = np.cumsum(lengths)
    pairs = np.zeros((int(offsets[-1]), 2), np.uint32)
    for l in range(count):
        lo, hi = int(offsets[l]), int(offsets[l + 1])
        pairs[lo:hi, 0] = sort_keys(kinds[l], hi - lo, rng)
        pairs[lo:hi, 1] = np.arange(hi - lo)
    return pairs, offsets


# ---- marked cells of a boundary-cell grid (csrc/cell_grid.h, cell_grid.hip) ---------------------------------------------------
CELL_POINTS = (1, 63, 64, 65, 4097)
CELL_GRIDS = ((3, 16), (4, 4), (11, 6), (35, 2), (3, 64))       # (cells a side, gridSize): 27 cells = one partial word, 64 = two full words
# (even grid sizes only: with an odd one a point in the last cell before a face has its upper cell outside the grid)
CELL_CLOUDS = ("random", "one_cell", "near_faces", "word_ends")
NO_SLOT = 0xFFFFFFFF


def cell_geometry(w, grid_size):
    """(half, disth, th) of the grid of w cells a side"""
    half = grid_size // 2
    return half, max(half, 1), grid_size * w


def cell_cloud(kind, m, w, grid_size, seed=0):
    """(xyz4 [m][4] int16 = (x, y, z, 0), boundary type [m] uint8) on the grid of w cells a side"""
    rng = np.random.default_rng([seed, m, w, grid_size, CELL_CLOUDS.index(kind)])
    half, disth, th = cell_geometry(w, grid_size)
    btype = rng.choice(np.array([0, 1, 1, 3], np.uint8), m)      # types 0 and 3 among the 1s: they mark nothing
    if kind == "random":                                          # some beyond the faces and below zero
        p = rng.integers(-2, th + 3, (m, 3))
    elif kind == "one_cell":                                      # every point in one inner cell, in either half of it
        p = rng.integers(1, w - 1, 3) * grid_size + rng.integers(0, grid_size, (m, 3))
        btype[:] = 1
    elif kind == "near_faces":                                    # type 1 only within disth of a face; the others anywhere
        p = rng.integers(0, th + 1, (m, 3))
        axis, low = rng.integers(0, 3, m), rng.integers(0, 2, m).astype(bool)
        near = np.where(low, rng.integers(0, disth, m), th - disth + rng.integers(0, disth + 1, m))
        one = btype == 1
        p[one, axis[one]] = near[one]
    elif kind == "word_ends":                                     # the upper half of cells whose key sits on bit 0 or bit 31 of a word
        key = np.arange(w ** 3)
        cx, cy, cz = key % w, key // w % w, key // (w * w)
        ends = key[((key % 32 == 0) | (key % 32 == 31)) & (cx < w - 1) & (cy < w - 1) & (cz < w - 1)]
        pick = rng.choice(ends, m)
        p = np.stack([pick % w, pick // w % w, pick // (w * w)], 1) * grid_size + rng.integers(half, grid_size, (m, 3))
        btype[:] = 1
    else:
        raise ValueError(kind)
    xyz4 = np.zeros((m, 4), np.int16)
    xyz4[:, :3] = p
    return xyz4, btype


def marked_cells_reference(xyz4, btype, w, grid_size):
    """(bit words [ceil(w^3 / 32)], marked cells before each word, slot of every key [w^3]: its rank in raster order, NO_SLOT if
    not marked): the eight cells around every type-1 point inside the faces"""
    half, disth, th = cell_geometry(w, grid_size)
    p = np.asarray(xyz4)[:, :3].astype(np.int64)
    inside = (np.asarray(btype) == 1) & np.all((p >= disth) & (p + disth < th), axis=1)
    q = p[inside]
    cell = q // grid_size
    low = cell - (q - cell * grid_size < half)
    marked = np.zeros((w ** 3 + 31) // 32 * 32, bool)
    for k in range(8):
        marked[((low[:, 2] + (k >> 2)) * w + low[:, 1] + ((k >> 1) & 1)) * w + low[:, 0] + (k & 1)] = True
    bits = np.packbits(marked, bitorder="little").view(np.uint32)
    per_word = marked.reshape(-1, 32).sum(axis=1)
    rank = (np.cumsum(per_word) - per_word).astype(np.uint32)
    slot = np.where(marked, np.cumsum(marked) - 1, NO_SLOT).astype(np.uint32)[:w ** 3]
    return bits, rank, slot


# ---- the cross-lane idioms of csrc/wave.h (tmc2_selftest_wave) -------------------------------------------------------------
WAVE_OPS = {"scan": 0, "scan16": 1, "sum": 2, "sum16": 3, "min": 4, "max": 5, "compact": 6, "sort": 7, "block_scan": 8}
WAVE_TYPES = {"uint32": 0, "int32": 1, "float64": 2}
WAVE_U32_PATTERNS = ("zero", "one", "index", "max", "first", "last", "middle", "random")
WAVE_PREDICATES = ("none", "all", "alternating", "lane0", "lane63", "random")
WAVE_SORT_LENGTHS = (64, 128, 2048)
WAVE_SORT_KINDS = ("duplicates", "padded", "sorted", "reversed")
WAVE_BLOCK_WAVES = (1, 2, 4, 16)
WAVE_NO_LANE = 0xFFFFFFFF


def wave_u32(size, groups=4, seed=0):
    """every pattern, `groups` groups of `size` values each, back to back: zeros, ones, the index in the group (plus 1000 per
    group), 0xFFFFFFFF everywhere (the sums wrap), one non-zero at the first, the last and the middle place, random words"""
    rng = np.random.default_rng([seed, size, groups])
    out = np.zeros((len(WAVE_U32_PATTERNS), groups, size), np.uint32)
    out[1] = 1
    out[2] = np.arange(size, dtype=np.uint32)[None, :] + 1000 * np.arange(groups, dtype=np.uint32)[:, None]
    out[3] = 0xFFFFFFFF
    for row, place in ((4, 0), (5, size - 1), (6, size // 2)):
        out[row, :, place] = 0x89ABCDEF + np.arange(groups, dtype=np.uint32)
    out[7] = rng.integers(0, 1 << 32, (groups, size), dtype=np.uint32)
    return out.reshape(-1)


def wave_i32(extremes, blocks=2, seed=0):
    """mixed signs, four wavefronts of their own per block; extremes: the whole range with INT_MIN and INT_MAX in every wavefront
    (for min and max), else small enough that no sum overflows"""
    rng = np.random.default_rng([seed, int(extremes), blocks])
    if not extremes:
        return rng.integers(-(1 << 20), 1 << 20, blocks * 256).astype(np.int32)
    a = rng.integers(-(1 << 31), 1 << 31, (blocks * 4, 64)).astype(np.int32)
    for w in range(len(a)):
        a[w, (7 * w) % 64], a[w, (7 * w + 33) % 64] = -(1 << 31), (1 << 31) - 1
    a[0, :] = np.where(np.arange(64) % 2, -(1 << 31), (1 << 31) - 1)      # (nothing but the two ends)
    return a.reshape(-1)


def wave_f64(blocks=2, seed=0):
    """magnitudes 2^-40 .. 2^40 with full mantissas and mixed signs: the order of a sum shows in its low bits"""
    rng = np.random.default_rng([seed, blocks, 64])
    n = blocks * 256
    return np.ldexp(rng.uniform(1.0, 2.0, n), rng.integers(-40, 41, n)) * rng.choice([-1.0, 1.0], n)


def wave_scan_reference(a, width=64):
    """the shuffle loop itself: for off = 1, 2, 4 .. < width, lanes at or past off in their group add the value off lanes below"""
    v = np.array(a)
    place = np.arange(len(v)) % width
    off = 1
    while off < width:
        t = np.roll(v, off)
        v = np.where(place >= off, v + t, v)
        off <<= 1
    return v


def wave_reduce_reference(a, op, width=64):
    """the butterfly itself: for off = width / 2 .. 1, v = op( v, v[lane ^ off] ); op: np.add, np.minimum, np.maximum"""
    v = np.array(a)
    lane = np.arange(len(v))
    off = width // 2
    while off:
        v = op(v, v[lane ^ off])
        off >>= 1
    return v


def wave_predicates(blocks=1, seed=0):
    """every predicate pattern over `blocks` workgroups of four wavefronts each, as uint32 0 / 1"""
    rng = np.random.default_rng([seed, blocks, 6])
    out = np.zeros((len(WAVE_PREDICATES), blocks * 4, 64), np.uint32)
    out[1] = 1
    out[2, :, ::2] = 1
    out[2, 1::2] ^= 1                                             # (odd wavefronts: the odd lanes)
    out[3, :, 0] = 1
    out[4, :, 63] = 1
    out[5] = rng.integers(0, 2, out[5].shape, dtype=np.uint32)
    return out.reshape(-1)


def wave_compact_reference(pred):
    """(per wavefront: the set lanes back to back, then WAVE_NO_LANE; per lane: the wavefront's count)"""
    p = np.asarray(pred).reshape(-1, 64) != 0
    out = np.full(p.shape, WAVE_NO_LANE, np.uint32)
    for w, row in enumerate(p):
        lanes = np.flatnonzero(row)
        out[w, :len(lanes)] = lanes
    return out.reshape(-1), np.repeat(p.sum(axis=1), 64).astype(np.uint32)


def wave_sort_lists(length, seed=0):
    """one list of `length` keys per kind: few distinct keys; a valid length that is no power of two, padded with 0xFFFFFFFF (which
    is also one of the valid keys); already sorted; reverse sorted"""
    rng = np.random.default_rng([seed, length])
    dup = rng.integers(0, 7, length, dtype=np.uint32) * 0x10000001
    valid = length - length // 4 - 3
    padded = np.full(length, 0xFFFFFFFF, np.uint32)
    padded[:valid] = rng.integers(0, 1 << 32, valid, dtype=np.uint32)
    padded[valid // 2] = 0xFFFFFFFF
    rising = np.sort(rng.integers(0, 1 << 32, length, dtype=np.uint32))
    return np.concatenate([dup, padded, rising, rising[::-1]])


def wave_block_scan_reference(a, waves):
    """(per thread: the sum of the workgroup's values before it, per thread: the workgroup's total), uint32 modulo 2^32"""
    g = np.asarray(a, np.uint32).reshape(-1, 64 * waves)
    inc = np.cumsum(g, axis=1, dtype=np.uint32)
    return (inc - g).reshape(-1), np.repeat(inc[:, -1], 64 * waves)
