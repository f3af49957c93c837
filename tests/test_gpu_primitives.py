"""GPU tier: the shared device primitives on their own (tmc2_selftest_*: csrc/selftest.hip, and S7's kernels in csrc/patches.hip)
against the plain references of tests/primitive_cases.py -- the exclusive scan, the several-regions fill, the XCD work mapping,
S7's union-find kernels on neighbour tables no cloud produces, both union-finds over explicit edge lists, CandSort against the
real std::sort, the marked cells of a boundary-cell grid, and the cross-lane idioms of csrc/wave.h.  Every comparison is exact: integer
equality, float64 as bit patterns.  The entries queue on the context's stream and do not wait: a test
queues all its calls, then reads back."""
import ctypes as C
import threading

import numpy as np
import pytest

import primitive_cases as pc
import tmc2_amd as T
from tmc2_amd import lib

SENTINEL = 0xDEADBEEF


class Dev:
    """the device buffers of one test (tmc2_ctx_device_alloc), freed when it ends"""

    def __init__(self, ctx):
        self.ctx, self.held = ctx, []

    def alloc(self, nbytes):
        self.held.append(self.ctx.device_alloc(max(int(nbytes), 1)))
        return self.held[-1]

    def put(self, array):
        a = np.ascontiguousarray(array)
        p = self.alloc(a.nbytes)
        if a.nbytes:
            self.ctx.upload(p, a)
        return p

    def get(self, p, shape, dtype):
        out = np.empty(shape, dtype)
        if out.nbytes:
            self.ctx.download(out, p)                              # (ends with a synchronisation of the stream)
        return out

    def close(self):
        self.ctx.synchronize()
        for p in self.held:
            self.ctx.device_free(p)
        self.held = []


def at(p, nbytes):
    return C.c_void_p(p.value + int(nbytes))


@pytest.fixture
def dev(gpu_ctx):
    d = Dev(gpu_ctx)
    yield d
    d.close()


@pytest.fixture
def fresh_ctx():
    """a context of its own: its scan state starts unallocated, at epoch 0"""
    ctx = T.Context(0)
    d = Dev(ctx)
    yield ctx, d
    d.close()
    ctx.close()


# ---- scan ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("n", pc.SCAN_SIZES)
def test_gpu_scan_is_the_cumsum(gpu_ctx, dev, n):
    """every pattern, out of place and in place, with and without the device total (131 073: the first scan that needs a second
    look-back window of 64 tiles)"""
    jobs = []
    for pattern in pc.SCAN_PATTERNS:
        a = pc.scan_input(pattern, n)
        want, total = pc.scan_reference(a)
        d_in = dev.put(a)
        for in_place in (False, True):
            for with_total in (False, True):
                src = dev.put(a) if in_place else d_in
                dst = src if in_place else dev.put(np.full(n, SENTINEL, np.uint32))
                d_total = dev.put(np.array([SENTINEL], np.uint32)) if with_total else None
                gpu_ctx.selftest_scan(src, dst, n, d_total)
                jobs.append((pattern, in_place, dst, d_total, want, total))
        jobs.append((pattern, "input", d_in, None, a, None))          # the out-of-place scans left their input alone
    for pattern, form, dst, d_total, want, total in jobs:
        assert np.array_equal(dev.get(dst, (n,), np.uint32), want), (pattern, form)
        if d_total is not None:                                       # (n = 0 leaves the total at 0)
            assert int(dev.get(d_total, (1,), np.uint32)[0]) == int(total), (pattern, form)


@pytest.mark.gpu
def test_gpu_scan_answer_line_and_its_carry_words(gpu_ctx, dev):
    """the total in word 0 of a page-locked line, the carry words behind it unchanged, nothing beyond them; no element: refused"""
    lines = T.host_array((9, 16), np.uint32)
    lines[:] = 0xA5A5A5A5
    carry = np.arange(7, dtype=np.uint32) * 0x01010101 + 0x80000001
    d_carry = dev.put(carry)
    jobs = []
    for row, (words, n) in enumerate((w, n) for w in (0, 1, 7) for n in (1, 2049, 131073)):
        a = pc.scan_input("counts", n, seed=words)
        want, total = pc.scan_reference(a)
        d_in, d_out, d_total = dev.put(a), dev.alloc(4 * n), dev.put(np.array([SENTINEL], np.uint32))
        gpu_ctx.selftest_scan(d_in, d_out, n, d_total, C.c_void_p(lines[row].ctypes.data), d_carry if words else None, words)
        jobs.append((row, words, n, d_out, d_total, want, total))
    for row, words, n, d_out, d_total, want, total in jobs:
        assert np.array_equal(dev.get(d_out, (n,), np.uint32), want), (words, n)
        assert int(dev.get(d_total, (1,), np.uint32)[0]) == int(total)
        assert int(lines[row, 0]) == int(total), (words, n)
        assert np.array_equal(lines[row, 1:1 + words], carry[:words]) and (lines[row, 1 + words:] == 0xA5A5A5A5).all(), (words, n)
    assert np.array_equal(dev.get(d_carry, (7,), np.uint32), carry)
    d_total = dev.put(np.array([SENTINEL], np.uint32))
    with pytest.raises(T.Tmc2Error, match="answer line needs at least one element"):
        gpu_ctx.selftest_scan(d_carry, d_carry, 0, d_total, C.c_void_p(lines[0].ctypes.data), None, 0)
    assert int(dev.get(d_total, (1,), np.uint32)[0]) == 0
    with pytest.raises(T.Tmc2Error, match="selftest_scan: invalid argument"):
        gpu_ctx.selftest_scan(d_carry, d_carry, 7, None, None, d_carry, 8)


def _queue_scans(ctx, d, sizes, seed):
    """scans of the given sizes back to back, no synchronisation in between; inputs at every alignment, outputs in distinct
    buffers; returns the checks to make afterwards"""
    rng = np.random.default_rng(seed)
    pool = rng.integers(0, 1 << 16, 2 * max(sizes) + 64, dtype=np.uint32)
    d_pool = d.put(pool)
    d_out = d.put(np.full(int(np.sum(sizes)) + 1, SENTINEL, np.uint32))
    jobs, where = [], 0
    for n in sizes:
        start = int(rng.integers(0, len(pool) - n))
        ctx.selftest_scan(at(d_pool, 4 * start), at(d_out, 4 * where), n)
        jobs.append((start, where, n))
        where += n
    out = d.get(d_out, (where + 1,), np.uint32)
    assert out[where] == SENTINEL
    return [(n, out[w:w + n], pc.scan_reference(pool[s:s + n])[0]) for s, w, n in jobs]


@pytest.mark.gpu
def test_gpu_scan_200_queued_scans_of_random_sizes(fresh_ctx):
    """one context, no synchronisation: the words a larger, earlier scan left must read as 'not yet published'"""
    ctx, d = fresh_ctx
    sizes = [int(n) for n in np.random.default_rng(7).integers(1, 300001, 200)]
    for k, (n, got, want) in enumerate(_queue_scans(ctx, d, sizes, 8)):
        assert np.array_equal(got, want), (k, n)


@pytest.mark.gpu
def test_gpu_scan_state_grows_past_4096_tiles(fresh_ctx):
    ctx, d = fresh_ctx
    for k, (n, got, want) in enumerate(_queue_scans(ctx, d, [3000, 2048 * 4096 + 1, 3000], 9)):
        assert np.array_equal(got, want), (k, n)


@pytest.mark.gpu
def test_gpu_scan_epoch_wrap(fresh_ctx):
    """epoch 0x3FFFFFFE set through the one back door; the next scans run at 0x3FFFFFFF, then wrap to a cleared state"""
    ctx, d = fresh_ctx
    first = _queue_scans(ctx, d, [1000003], 10)                         # (the state holds words of a large scan)
    one = d.put(np.ones(1, np.uint32))
    ctx.selftest_scan(one, one, 1, epoch=0x3FFFFFFE)
    for k, (n, got, want) in enumerate(first + _queue_scans(ctx, d, [264197, 7, 133121, 1000003], 11)):
        assert np.array_equal(got, want), (k, n)
    assert int(d.get(one, (1,), np.uint32)[0]) == 0


@pytest.mark.gpu
def test_gpu_scan_epochs_differ_in_their_top_bit(fresh_ctx):
    """all 30 bits of the epoch tell one call's words from another's: a scan at epoch 0x20000001 over the words a scan of the same
    tiles left at epoch 1 (an epoch compared, or kept, one bit short would take them for its own predecessors' sums)"""
    ctx, d = fresh_ctx
    n = 1000003
    a, b = pc.scan_input("one", n), pc.scan_input("counts", n, seed=3)
    d_a, d_b, d_out = d.put(a), d.put(b), d.alloc(4 * n)
    ctx.selftest_scan(d_a, d_a, n)
    ctx.selftest_scan(d_b, d_out, n, epoch=0x20000000)
    assert np.array_equal(d.get(d_a, (n,), np.uint32), pc.scan_reference(a)[0])
    assert np.array_equal(d.get(d_out, (n,), np.uint32), pc.scan_reference(b)[0])


@pytest.mark.gpu
def test_gpu_scan_two_contexts_from_two_threads():
    failures = []

    def run(seed):
        try:
            ctx = T.Context(0)
            d = Dev(ctx)
            try:
                sizes = [int(n) for n in np.random.default_rng(seed).integers(1, 300001, 50)]
                for k, (n, got, want) in enumerate(_queue_scans(ctx, d, sizes, seed + 100)):
                    if not np.array_equal(got, want):
                        failures.append((seed, k, n))
            finally:
                d.close()
                ctx.close()
        except Exception as e:                                         # noqa: BLE001 (reported by the asserting thread)
            failures.append((seed, repr(e)))

    threads = [threading.Thread(target=run, args=(seed,)) for seed in (21, 22)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not failures, failures


# ---- fill ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("per_call", [1, 12])
def test_gpu_fill_every_head_and_length_inside_guard_bytes(gpu_ctx, dev, per_call):
    """head offsets 0..15 x lengths 0..40 and around the 16 KiB block boundaries, one region or twelve regions (empty ones among
    them, every value different) per launch; no guard byte between the regions changes"""
    regions, total = pc.fill_layout()
    groups = [regions[k:k + per_call] for k in range(0, len(regions), per_call)]
    assert per_call == 1 or sum(any(length == 0 for _, length, _ in g) and len({v for _, _, v in g}) == 12 for g in groups) == 16
    base = dev.put(np.full(total, pc.FILL_GUARD, np.uint8))
    for k in range(0, len(regions), per_call):
        group = regions[k:k + per_call]
        gpu_ctx.selftest_fill([(base.value + start, length, value) for start, length, value in group])
    got, want = dev.get(base, (total,), np.uint8), pc.fill_reference(total, regions)
    wrong = np.flatnonzero(got != want)
    assert len(wrong) == 0, "first wrong byte at %d: %d for %d" % (wrong[0], got[wrong[0]], want[wrong[0]])


@pytest.mark.gpu
def test_gpu_fill_thirteen_regions_are_refused(gpu_ctx, dev):
    base = dev.put(np.full(13 * 64, pc.FILL_GUARD, np.uint8))
    thirteen = [(base.value + 64 * k + 3, 17, k + 1) for k in range(13)]
    with pytest.raises(T.Tmc2Error, match="more than 12 regions"):
        gpu_ctx.selftest_fill(thirteen)
    assert (dev.get(base, (13 * 64,), np.uint8) == pc.FILL_GUARD).all()      # refused whole: nothing was launched
    thirteen[5] = (thirteen[5][0], 0, 6)                                    # an empty region does not count
    gpu_ctx.selftest_fill(thirteen)
    want = pc.fill_reference(13 * 64, [(64 * k + 3, 0 if k == 5 else 17, k + 1) for k in range(13)])
    assert np.array_equal(dev.get(base, (13 * 64,), np.uint8), want)
    with pytest.raises(T.Tmc2Error, match="selftest_fill: invalid argument"):
        gpu_ctx.selftest_fill(thirteen + [thirteen[0]])
    gpu_ctx.selftest_fill([])


# ---- work map -----------------------------------------------------------------------------------------------------------
def _work_map(ctx, dev, grid, threads, n, live, launched=None):
    launched = grid if launched is None else launched
    d_hits = dev.put(np.zeros(2 * max(n, 1), np.uint32))
    d_logical = dev.put(np.full(launched + 16, SENTINEL, np.uint32))
    ctx.selftest_work_map(grid, threads, n, live, d_hits, d_logical)
    return dev.get(d_hits, (2, max(n, 1)), np.uint32)[:, :n], dev.get(d_logical, (launched + 16,), np.uint32)


@pytest.mark.gpu
@pytest.mark.parametrize("threads", [64, 256])
def test_gpu_work_map_visits_every_element_once(gpu_ctx, dev, threads):
    """every lane's chunkedIndex() / pointOfLane() element is hit exactly once; a chunked grid's logical blocks are a permutation
    and XCD x (workgroup b: b % 8) holds the x-th eighth; grids that are no multiple of 8 take their blocks as they come"""
    for grid in pc.WORK_GRIDS + pc.WORK_GRIDS_UNCHUNKED:
        for n in pc.work_sizes(grid, threads):
            hits, logical = _work_map(gpu_ctx, dev, grid, threads, n, 0)
            assert (hits == 1).all(), (grid, n, "hits", int((hits[0] != 1).sum()), int((hits[1] != 1).sum()))
            lg = logical[:grid].astype(np.int64)
            assert (logical[grid:] == SENTINEL).all()
            assert sorted(lg.tolist()) == list(range(grid)), (grid, n)
            if grid % 8 == 0:
                assert (lg // (grid // 8) == np.arange(grid) % 8).all(), (grid, n)
            assert np.array_equal(logical[:grid], pc.work_map_reference(grid)), (grid, n)
        dev.close()


@pytest.mark.gpu
@pytest.mark.parametrize("threads", [64, 256])
def test_gpu_work_map_live_blocks_form(gpu_ctx, dev, threads):
    """knnKernel's form: the eighths are those of the LIVE blocks; exactly the first ceil(live / 8) * 8 logical blocks act"""
    for grid in pc.WORK_GRIDS:
        for live in sorted({1, 8, 9, grid - 1}):
            if not 1 <= live <= grid:
                continue
            acting = (live + 7) // 8 * 8
            for n in pc.work_sizes(grid, threads):
                hits, logical = _work_map(gpu_ctx, dev, grid, threads, n, live)
                want = (np.arange(n) < acting * threads).astype(np.uint32)
                assert np.array_equal(hits[0], want) and np.array_equal(hits[1], want), (grid, live, n)
                assert np.array_equal(logical[:grid], pc.work_map_reference(grid, live)) and (logical[grid:] == SENTINEL).all()
                assert sorted(int(x) for x in logical[:grid] if x != 0xFFFFFFFF) == list(range(acting)), (grid, live, n)
        dev.close()
    with pytest.raises(T.Tmc2Error, match="selftest_work_map"):
        _work_map(gpu_ctx, dev, 12, threads, 5, 3)                      # live blocks on a grid that is no multiple of 8
    with pytest.raises(T.Tmc2Error, match="selftest_work_map"):
        _work_map(gpu_ctx, dev, 8, threads, 5, 9)


@pytest.mark.gpu
@pytest.mark.parametrize("threads", [64, 256])
def test_gpu_work_map_grid_of_a_pass_is_a_multiple_of_8(gpu_ctx, dev, threads):
    """no grid given: the grid the stages give a chunked pass (chunkedGrid: the blocks n needs, rounded up to 8)"""
    for blocks in (1, 2, 4, 5, 8, 9, 12, 17, 1001):
        for n in (blocks * threads, blocks * threads - threads + 1):
            grid = (blocks + 7) // 8 * 8
            hits, logical = _work_map(gpu_ctx, dev, 0, threads, n, 0, launched=grid)
            assert (hits == 1).all(), (blocks, n)
            assert np.array_equal(logical[:grid], pc.work_map_reference(grid)) and (logical[grid:] == SENTINEL).all(), (blocks, n)


# ---- S7's kernels on neighbour tables no cloud produces ---------------------------------------------------------------------
CROSSES = [(pre, scope, order) for pre in (None, "0") for scope in (None, "agent") for order in ("input", "chunk", "tree")]


def _components(ctx, dev, family, n, cut, perm):
    knn, partition, raw, label, _ = pc.graph_case(family, n, cut)
    d_root, d_bad = dev.put(np.full(n, 0xFFFFFFFF, np.uint32)), dev.put(np.zeros(2, np.uint32))
    ctx.selftest_components(dev.put(knn), dev.put(partition), dev.put(raw), dev.put(perm), n, d_root, d_bad)
    return raw, label, d_root, d_bad


def _check_components(dev, raw, label, d_root, d_bad, what):
    n = len(raw)
    root, bad = dev.get(d_root, (n,), np.uint32).astype(np.int64), dev.get(d_bad, (2,), np.uint32)
    members = np.flatnonzero(raw)
    assert bad.tolist() == [0, 0], (what, bad.tolist())
    assert (root[raw == 0] == 0xFFFFFFFF).all(), what                   # a point that is not raw takes no part
    assert root[members].max() < n, what
    assert np.array_equal(root[root[members]], root[members]), what     # a root is its own root
    # root[u] == root[v] exactly when the reference puts u and v in one component, and root[u] lies in u's component
    assert pc.same_partition(label, root, members), what


def _set_cross(ctx_options, cross):
    pre, scope, order = cross
    ctx_options.setenv("TMC2_UF_CHECK", "1")
    ctx_options.setenv("TMC2_UF_PRECHECK", pre)
    ctx_options.setenv("TMC2_UF_SCOPE", scope)
    ctx_options.setenv("TMC2_MUTUAL_ORDER", order)


@pytest.mark.gpu
@pytest.mark.parametrize("cut", [False, True], ids=["whole", "cut"])
@pytest.mark.parametrize("family", pc.GRAPH_FAMILIES)
def test_gpu_components_of_graph_families(gpu_ctx, ctx_options, dev, family, cut):
    """one block (300 points) and a partial eighth (4 099), under every form of the union pass"""
    for n in (300, 4099):
        perm = np.random.default_rng([n, 5]).permutation(n).astype(np.uint32)
        jobs = []
        for cross in CROSSES:
            _set_cross(ctx_options, cross)
            jobs.append((cross, _components(gpu_ctx, dev, family, n, cut, perm)))
        for cross, job in jobs:
            _check_components(dev, *job, (family, cut, n, cross))


@pytest.mark.gpu
@pytest.mark.parametrize("cross", CROSSES, ids=["pre%s-%s-%s" % (p or "1", s or "wg", o) for p, s, o in CROSSES])
def test_gpu_components_many_blocks_on_all_xcds(gpu_ctx, ctx_options, dev, cross):
    n = 65536 + 17
    perm = np.random.default_rng([n, 5]).permutation(n).astype(np.uint32)
    _set_cross(ctx_options, cross)
    jobs = [((family, cut), _components(gpu_ctx, dev, family, n, cut, perm)) for family in pc.GRAPH_FAMILIES for cut in (False, True)]
    for what, job in jobs:
        _check_components(dev, *job, (what, n, cross))


# ---- both union-finds over explicit edge lists --------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("forest", ["identity", "hooked"])
@pytest.mark.parametrize("family", pc.EDGE_FAMILIES)
@pytest.mark.parametrize("parity", [0, 1], ids=["plain", "parity"])
def test_gpu_union_find_over_edge_lists(gpu_ctx, dev, parity, family, forest):
    """the partition is the reference's, every root is its own root, the parities compose to the hidden signs, the settled links
    still fall in priority and the coherent climb finds nothing broken -- with and without the pre-check, at both scopes"""
    n = pc.UF_N
    a, b, sign, parent0, parity0, label = pc.edge_case(family, forest)
    edges = np.stack([a, b, (sign[a] ^ sign[b]) if parity else np.zeros(len(a), np.uint32)], axis=1).astype(np.uint32)
    d_edges = dev.put(edges)
    words0 = pc.forest_words(parent0, parity0 if parity else np.zeros(n, np.uint32), parity)
    jobs = []
    for precheck in (0, 1):
        for agent in (0, 1):
            d_word, d_bad = dev.put(words0), dev.put(np.zeros(2, np.uint32))
            d_root, d_rp = dev.put(np.full(n, 0xFFFFFFFF, np.uint32)), dev.put(np.full(n, 0xFFFFFFFF, np.uint32))
            gpu_ctx.selftest_union_find(parity, d_word, n, d_edges, len(edges), precheck, agent, d_root, d_rp, d_bad)
            jobs.append(((precheck, agent), d_word, d_root, d_rp, d_bad))
    for what, d_word, d_root, d_rp, d_bad in jobs:
        root, rp = dev.get(d_root, (n,), np.uint32).astype(np.int64), dev.get(d_rp, (n,), np.uint32)
        assert dev.get(d_bad, (2,), np.uint32).tolist() == [0, 0], what
        assert root.max() < n and np.array_equal(root[root], root), what
        assert pc.same_partition(label, root), what
        if parity:
            assert pc.parity_consistent(root, rp, sign), what
        else:
            assert not rp.any(), what
        settled = pc.word_parents(dev.get(d_word, (n,), np.uint32), parity)
        assert pc.links_fall_in_priority(settled), what
        assert np.array_equal(settled[root], root), what                # what find called a root links to itself


# ---- CandSort -------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_cand_sort_is_std_sort_pair_for_pair(gpu_ctx, dev):
    """20 000 lists, heavy ties: the device's replay leaves every (distance, payload) pair where libstdc++'s std::sort leaves it"""
    pairs, offsets = pc.sort_lists()
    want = lib.selftest_std_sort(pairs, offsets)
    lists = len(offsets) - 1
    d_lists, d_ok = dev.put(pairs), dev.put(np.full(lists, SENTINEL, np.uint32))
    gpu_ctx.selftest_cand_sort(d_lists, dev.put(offsets), lists, d_ok)
    got, ok = dev.get(d_lists, pairs.shape, np.uint32), dev.get(d_ok, (lists,), np.uint32)
    assert (ok == 1).all(), np.flatnonzero(ok != 1)[:8]
    differ = np.flatnonzero((got != want).any(axis=1))
    assert len(differ) == 0, "first difference in list %d" % (np.searchsorted(offsets, differ[0], side="right") - 1)


# ---- marked cells of a boundary-cell grid -----------------------------------------------------------------------------------
def _marked_cells_case(ctx, dev, xyz4, btype, w, grid_size, bits, what):
    want_bits, want_rank, want_slot = pc.marked_cells_reference(xyz4, btype, w, grid_size)
    words, cells = len(want_bits), w ** 3
    keys = np.concatenate([np.arange(cells, dtype=np.uint32), np.array([cells, cells + 31, 0x7FFFFFFF, pc.NO_SLOT], np.uint32)])
    d_bits, d_rank = dev.put(np.full(words + 1, SENTINEL, np.uint32)), dev.put(np.full(words + 1, SENTINEL, np.uint32))
    d_slots = dev.put(np.full(len(keys) + 1, SENTINEL, np.uint32))
    count = ctx.selftest_marked_cells(dev.put(xyz4), dev.put(btype), len(xyz4), grid_size, bits, 0 if bits else grid_size * w, d_bits,
                                      d_rank, dev.put(keys), len(keys), d_slots)
    got_bits, got_rank = dev.get(d_bits, (words + 1,), np.uint32), dev.get(d_rank, (words + 1,), np.uint32)
    got_slot = dev.get(d_slots, (len(keys) + 1,), np.uint32)
    assert count == int((want_slot != pc.NO_SLOT).sum()), what
    assert np.array_equal(got_bits[:words], want_bits) and np.array_equal(got_rank[:words], want_rank), what
    assert np.array_equal(got_slot[:cells], want_slot) and (got_slot[cells:-1] == pc.NO_SLOT).all(), what
    assert got_bits[words] == got_rank[words] == got_slot[-1] == SENTINEL, what
    return count


@pytest.mark.gpu
@pytest.mark.parametrize("w,grid_size", pc.CELL_GRIDS)
def test_gpu_marked_cells_are_the_reference(gpu_ctx, dev, w, grid_size):
    """bit words, ranks, the count and the slot of every key of the grid (and of keys beyond it) against the numpy reference: every
    cloud at every size, on the grid over [0, gridSize * w] as T3 lays it"""
    for kind in pc.CELL_CLOUDS:
        for m in pc.CELL_POINTS:
            xyz4, btype = pc.cell_cloud(kind, m, w, grid_size)
            count = _marked_cells_case(gpu_ctx, dev, xyz4, btype, w, grid_size, 0, (w, grid_size, kind, m))
            assert kind == "random" or (count == 0) == (kind == "near_faces"), (w, grid_size, kind, m)


@pytest.mark.gpu
def test_gpu_marked_cells_on_the_cube_and_without_outputs(gpu_ctx, dev):
    """T6's grid (2^bits / gridSize cells a side); no point at all; the optional outputs left out"""
    for grid_size, bits in ((4, 4), (2, 5), (16, 6)):
        w = (1 << bits) // grid_size
        for kind in ("random", "word_ends"):
            xyz4, btype = pc.cell_cloud(kind, 4097, w, grid_size)
            _marked_cells_case(gpu_ctx, dev, xyz4, btype, w, grid_size, bits, (grid_size, bits, kind))
    xyz4, btype = pc.cell_cloud("random", 65, 11, 6)
    want = int((pc.marked_cells_reference(xyz4, btype, 11, 6)[2] != pc.NO_SLOT).sum())
    assert gpu_ctx.selftest_marked_cells(dev.put(xyz4), dev.put(btype), 65, 6, 0, 66) == want > 0
    assert gpu_ctx.selftest_marked_cells(None, None, 0, 6, 0, 66) == 0
    with pytest.raises(T.Tmc2Error, match="selftest_marked_cells"):
        gpu_ctx.selftest_marked_cells(dev.put(xyz4), dev.put(btype), 65, 3, 0, 66)


# ---- the cross-lane idioms of csrc/wave.h --------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_wave_scans_and_reductions_are_the_shuffle_loops(gpu_ctx, dev):
    """waveInclusive and waveSum / waveMin / waveMax at width 64 and 16 (four groups per wavefront) on uint32, int32 and float64:
    workgroups of four wavefronts with data of their own; float64 compared as bit patterns"""
    u32, small, extremes, f64 = pc.wave_u32(64), pc.wave_i32(False), pc.wave_i32(True), pc.wave_f64()
    jobs = []
    for a, names in ((u32, ("scan", "scan16", "sum", "sum16", "min", "max")), (small, ("scan", "scan16", "sum", "sum16")),
                     (extremes, ("min", "max")), (f64, ("scan", "scan16", "sum", "sum16"))):
        d_in = dev.put(a)
        for name in names:
            width = 16 if name.endswith("16") else 64
            if name.startswith("scan"):
                want = pc.wave_scan_reference(a, width)
            else:
                want = pc.wave_reduce_reference(a, {"sum": np.add, "min": np.minimum, "max": np.maximum}[name.rstrip("16")], width)
            d_out = dev.put(np.full(a.nbytes // 4, SENTINEL, np.uint32))
            gpu_ctx.selftest_wave(pc.WAVE_OPS[name], pc.WAVE_TYPES[a.dtype.name], d_in, d_out, len(a))
            jobs.append((name, a, d_out, want))
        jobs.append(("input", a, d_in, a))
    bits = {4: np.uint32, 8: np.uint64}
    for name, a, d_out, want in jobs:
        assert want.dtype == a.dtype
        got = dev.get(d_out, a.shape, a.dtype)
        assert np.array_equal(got.view(bits[a.itemsize]), want.view(bits[a.itemsize])), (name, a.dtype.name)


@pytest.mark.gpu
def test_gpu_lane_rank_compacts_in_lane_order(gpu_ctx, dev):
    """no lane, every lane, alternating lanes, lane 0 alone, lane 63 alone (the mask of all 63 lanes below), a random mask per
    wavefront: the compacted order and the count"""
    pred = pc.wave_predicates(2)
    want, count = pc.wave_compact_reference(pred)
    d_out, d_aux = dev.put(np.full(len(pred), SENTINEL, np.uint32)), dev.put(np.full(len(pred), SENTINEL, np.uint32))
    gpu_ctx.selftest_wave(pc.WAVE_OPS["compact"], 0, dev.put(pred), d_out, len(pred), d_aux)
    assert np.array_equal(dev.get(d_out, pred.shape, np.uint32), want)
    assert np.array_equal(dev.get(d_aux, pred.shape, np.uint32), count)


@pytest.mark.gpu
@pytest.mark.parametrize("length", pc.WAVE_SORT_LENGTHS)
def test_gpu_lds_bitonic_sort_is_np_sort(gpu_ctx, dev, length):
    """keys with duplicates, a padded list, sorted and reverse sorted input, one wavefront per list; the input stays as it was"""
    lists = pc.wave_sort_lists(length)
    d_in, d_out = dev.put(lists), dev.put(np.full(len(lists), SENTINEL, np.uint32))
    gpu_ctx.selftest_wave(pc.WAVE_OPS["sort"], length, d_in, d_out, len(lists))
    assert np.array_equal(dev.get(d_out, (len(pc.WAVE_SORT_KINDS), length), np.uint32), np.sort(lists.reshape(-1, length), axis=1))
    assert np.array_equal(dev.get(d_in, lists.shape, np.uint32), lists)


@pytest.mark.gpu
@pytest.mark.parametrize("waves", pc.WAVE_BLOCK_WAVES)
def test_gpu_block_exclusive_is_the_cumsum(gpu_ctx, dev, waves):
    """every integer pattern, one workgroup each: the offsets per thread and the total as every thread has it"""
    a = pc.wave_u32(64 * waves, groups=1)
    before, total = pc.wave_block_scan_reference(a, waves)
    d_out, d_aux = dev.put(np.full(len(a), SENTINEL, np.uint32)), dev.put(np.full(len(a), SENTINEL, np.uint32))
    gpu_ctx.selftest_wave(pc.WAVE_OPS["block_scan"], waves, dev.put(a), d_out, len(a), d_aux)
    assert np.array_equal(dev.get(d_out, a.shape, np.uint32), before)
    assert np.array_equal(dev.get(d_aux, a.shape, np.uint32), total)
