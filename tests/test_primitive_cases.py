"""CPU tier: the references of tests/primitive_cases.py checked on their own -- every graph family has a component count known in
closed form, every reference is compared with a second, differently built one -- and the argument checks of the tmc2_selftest_*
entries that need no device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import primitive_cases as pc
import tmc2_amd as T
from tmc2_amd import lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_scan_reference_is_the_loop():
    for pattern in pc.SCAN_PATTERNS:
        for n in (0, 1, 9, 2049):
            a = pc.scan_input(pattern, n)
            out, total = pc.scan_reference(a)
            run, want = 0, []
            for v in a.tolist():
                want.append(run)
                run = (run + v) & 0xFFFFFFFF
            assert out.dtype == np.uint32 and out.tolist() == want and int(total) == run, (pattern, n)
    assert int(pc.scan_reference(pc.scan_input("max", 5))[1]) == 0xFFFFFFFB          # wraps modulo 2^32
    assert len(set(pc.SCAN_SIZES)) == 14 and 131073 in pc.SCAN_SIZES


def test_fill_layout_covers_every_head_and_length_apart():
    regions, total = pc.fill_layout()
    assert len(regions) == 16 * len(pc.FILL_LENGTHS) and len(pc.FILL_LENGTHS) == 46
    assert {(s % 16, l) for s, l, _ in regions} == {(h, l) for h in range(16) for l in pc.FILL_LENGTHS}
    assert all(v not in (0, pc.FILL_GUARD) for _, _, v in regions)
    ends = [s + l for s, l, _ in regions]
    assert all(s2 - e1 >= 64 for e1, (s2, _, _) in zip(ends, regions[1:])) and regions[0][0] >= 64 and total - ends[-1] >= 64
    ref = pc.fill_reference(total, regions)
    assert int((ref != pc.FILL_GUARD).sum()) == sum(l for _, l, _ in regions)


def test_work_map_reference_is_a_permutation_in_eighths():
    for grid in pc.WORK_GRIDS:
        lg = pc.work_map_reference(grid)
        assert sorted(lg.tolist()) == list(range(grid))
        per = grid // 8
        for b in range(grid):                                     # XCD x = b % 8 holds the x-th eighth
            assert per * (b % 8) <= lg[b] < per * (b % 8 + 1)
        for live in (1, 8, 9, grid - 1):
            if live < 1 or live > grid:                           # (the entry refuses more live blocks than the grid has)
                continue
            lv = pc.work_map_reference(grid, live)
            acting = sorted(int(x) for x in lv if x != 0xFFFFFFFF)
            assert acting == list(range((live + 7) // 8 * 8)), (grid, live)
    for grid in pc.WORK_GRIDS_UNCHUNKED:
        assert pc.work_map_reference(grid).tolist() == list(range(grid))
    assert pc.work_sizes(16, 64) == [0, 1, 129, 1023, 1024]


def test_priority_is_the_headers_bijection():
    x = np.arange(1 << 16)
    p = pc.uf_priority(x)
    assert p.dtype == np.uint32 and len(np.unique(p)) == len(x)
    assert [int(v) for v in pc.uf_priority([0, 1, 2, 3])] == [0, 2654435761, (2 * 2654435761) % 2**32, (3 * 2654435761) % 2**32]
    hdr = open(os.path.join(ROOT, "mpeg-pcc-tmc2_amd", "csrc", "union_find.h")).read()
    assert re.search(r"ufPriority\( uint32_t x \) \{ return x \* (\d+)u; \}", hdr).group(1) == str(pc.UF_MULTIPLIER)


@pytest.mark.parametrize("n", [300, 4099])
@pytest.mark.parametrize("family", pc.GRAPH_FAMILIES)
def test_graph_families_have_their_closed_form_count(family, n):
    knn, count = pc.graph_table(family, n)
    assert knn.shape == (n, pc.K) and knn.dtype == np.uint32 and knn.max() < n
    ones, zeros = np.ones(n, np.uint8), np.zeros(n, np.uint8)
    a, b = pc.eligible_edges(knn, ones, zeros)
    label = pc.components(n, a, b)
    assert len(np.unique(label)) == count
    assert np.array_equal(label, pc.components_by_sweeps(n, a, b))
    assert np.array_equal(label[label], label) and (label <= np.arange(n)).all()
    if family == "one_way":
        assert len(a) == 0
    if family == "twice":
        assert (knn[:-1, 0] == knn[:-1, 2]).all()                # a neighbour listed twice in a row
    # cut by holes and planes: the two references agree, and no component crosses a plane or holds a hole
    _, partition, raw, cut_label, comps = pc.graph_case(family, n, True)
    ca, cb = pc.eligible_edges(knn, raw, partition)
    assert np.array_equal(cut_label, pc.components_by_sweeps(n, ca, cb))
    assert (partition[cut_label] == partition).all() and (cut_label[raw == 0] == np.flatnonzero(raw == 0)).all()
    assert comps >= min(count, int(raw.sum())) and 0 < (raw == 0).sum() < n // 4
    assert pc.same_partition(cut_label, cut_label, np.flatnonzero(raw))


def test_same_partition_tells_partitions_apart():
    label = np.array([0, 0, 2, 2, 4])
    assert pc.same_partition(label, np.array([1, 1, 3, 3, 4]))
    assert not pc.same_partition(label, np.array([1, 1, 3, 2, 4]))     # a component split
    assert not pc.same_partition(label, np.array([1, 1, 1, 1, 4]))     # two merged
    assert not pc.same_partition(label, np.array([1, 1, 3, 3, 5]))     # a root outside
    assert pc.same_partition(label, np.array([9, 9, 3, 3, 9]), members=[2, 3])


@pytest.mark.parametrize("family", pc.EDGE_FAMILIES)
def test_edge_families_have_their_closed_form_count(family):
    a, b, count = pc.edge_list(family)
    assert a.min() >= 0 and max(a.max(), b.max()) < pc.UF_N and len(a) == len(b)
    label = pc.components(pc.UF_N, a, b)
    assert np.array_equal(label, pc.components_by_sweeps(pc.UF_N, a, b))
    if count is not None:
        assert len(np.unique(label)) == count
    assert {"star": pc.UF_N - 1, "repeated": 4096, "loops": pc.UF_N, "path": pc.UF_N - 1, "path_priority": pc.UF_N - 1,
            "random": 2 * pc.UF_N, "cliques": 190000}[family] == len(a)


def test_initial_forest_obeys_the_headers_rule():
    sign = pc.hidden_signs()
    parent, parity = pc.initial_forest("hooked", sign=sign)
    assert pc.links_fall_in_priority(parent) and (parent != np.arange(pc.UF_N)).sum() > pc.UF_N // 3
    assert np.array_equal(parity, sign ^ sign[parent])
    assert not pc.links_fall_in_priority(np.array([1, 0]))             # a cycle cannot fall both ways
    ident, zero = pc.initial_forest("identity")
    assert np.array_equal(ident, np.arange(pc.UF_N)) and not zero.any()
    words = pc.forest_words(parent, parity, True)
    assert np.array_equal(pc.word_parents(words, True), parent) and np.array_equal(words & 1, parity)
    # the parity check accepts the truth and refuses one wrong bit
    *_, label = pc.edge_case("path", "hooked")
    rp = sign ^ sign[label]
    assert pc.parity_consistent(label, rp, sign)
    rp[12345] ^= 1
    assert not pc.parity_consistent(label, rp, sign)


def test_sort_lists_cover_the_lengths_and_tie_patterns():
    pairs, offsets = pc.sort_lists()
    lengths = np.diff(offsets.astype(np.int64))
    assert len(lengths) == 20000 and set(lengths.tolist()) == set(range(18)) | {31, 32, 33, 100, 1000, 5000}
    assert (lengths == 1000).sum() == len(pc.SORT_LONG_KEYS) == 6 and (lengths == 5000).sum() == 6
    for l in (17, 21, 19999):
        assert pairs[offsets[l]:offsets[l + 1], 1].tolist() == list(range(lengths[l]))   # payload = position
    # the host twin is the real std::sort: sorted, a permutation of its input list by list, and unstable as libstdc++ is
    got = lib.selftest_std_sort(pairs, offsets)
    unstable = 0
    for l in list(range(0, 20000, 97)) + list(range(19988, 20000)):
        lo, hi = int(offsets[l]), int(offsets[l + 1])
        assert (np.diff(got[lo:hi, 0].astype(np.int64)) >= 0).all()
        assert sorted(map(tuple, got[lo:hi].tolist())) == sorted(map(tuple, pairs[lo:hi].tolist()))
        stable = pairs[lo:hi][np.argsort(pairs[lo:hi, 0], kind="stable")]
        unstable += not np.array_equal(stable, got[lo:hi])
    assert unstable > 0
    with pytest.raises(T.Tmc2Error):
        lib.selftest_std_sort(pairs, offsets[:-1])


def test_selftest_entries_refuse_bad_arguments_without_a_device():
    L = T.load_library()
    invalid = int(re.search(r"#define TMC2_E_INVALID (-?\d+)", open(os.path.join(ROOT, "include", "tmc2hip.h")).read()).group(1))
    p = C.c_void_p(4096)                                              # never dereferenced: every call below stops at its arguments
    assert L.tmc2_selftest_scan(None, p, p, 8, None, None, None, 0, 0) == invalid
    assert L.tmc2_selftest_fill(None, p, 1) == invalid
    assert L.tmc2_selftest_work_map(None, 8, 64, 8, 0, p, p) == invalid
    assert L.tmc2_selftest_components(None, p, p, p, None, 8, p, p) == invalid
    assert L.tmc2_selftest_union_find(None, 0, p, 8, p, 1, 1, 0, p, p, p) == invalid
    assert L.tmc2_selftest_cand_sort(None, p, p, 1, p) == invalid
    assert L.tmc2_selftest_std_sort(None, None, 0) == invalid
    assert b"selftest_std_sort" in L.tmc2_last_error()
    falling = np.array([0, 2, 1], np.uint32)
    pairs = np.zeros((2, 2), np.uint32)
    assert L.tmc2_selftest_std_sort(pairs.ctypes.data_as(C.c_void_p), falling.ctypes.data_as(C.c_void_p), 2) == invalid


def test_marked_cells_reference_is_the_loop():
    """the vectorised reference against a set filled point by point, cell by cell; the clouds hold what their names promise"""
    for w, grid_size in pc.CELL_GRIDS:
        half, disth, th = pc.cell_geometry(w, grid_size)
        for kind in pc.CELL_CLOUDS:
            for m in (1, 65, 4097) if w < 35 else (65,):
                xyz4, btype = pc.cell_cloud(kind, m, w, grid_size)
                bits, rank, slot = pc.marked_cells_reference(xyz4, btype, w, grid_size)
                keys = set()
                for (x, y, z, _), t in zip(xyz4.tolist(), btype.tolist()):
                    if t != 1 or min(x, y, z) < disth or max(x, y, z) + disth >= th:
                        continue
                    lo = [c // grid_size - (1 if c % grid_size < half else 0) for c in (x, y, z)]
                    keys |= {((lo[2] + dz) * w + lo[1] + dy) * w + lo[0] + dx for dz in (0, 1) for dy in (0, 1) for dx in (0, 1)}
                what = (w, grid_size, kind, m)
                assert all(0 <= k < w ** 3 for k in keys), what
                order = sorted(keys)
                assert np.flatnonzero(slot != pc.NO_SLOT).tolist() == order and slot[order].tolist() == list(range(len(order))), what
                assert len(bits) == len(rank) == (w ** 3 + 31) // 32 and bits.dtype == rank.dtype == slot.dtype == np.uint32, what
                assert [k for k in range(len(bits) * 32) if bits[k >> 5] >> (k & 31) & 1] == order, what
                assert rank.tolist() == [sum(1 for k in order if k < 32 * i) for i in range(len(rank))], what
                if kind == "near_faces":
                    assert not keys and not bits.any(), what
                if kind == "one_cell":
                    assert len({tuple(c) for c in (xyz4[:, :3] // grid_size).tolist()}) == 1 and 8 <= len(keys) <= 27, what
                if kind == "word_ends":
                    assert any(k % 32 == 0 for k in keys) or any(k % 32 == 31 for k in keys), what
                if kind == "random" and m == 4097:
                    assert set(btype.tolist()) == {0, 1, 3} and keys and (xyz4[:, :3] < 0).any() and (xyz4[:, :3] >= th).any(), what
    # both ends of a word, over all sizes of one grid; a type-1 point near a face in every near_faces cloud of some size
    ends = set()
    for m in pc.CELL_POINTS:
        ends |= {int(k) % 32 for k in np.flatnonzero(pc.marked_cells_reference(*pc.cell_cloud("word_ends", m, 11, 6), 11, 6)[2] != pc.NO_SLOT)}
    assert {0, 31} <= ends
    assert all((pc.cell_cloud("near_faces", m, 4, 4)[1] == 1).any() for m in (63, 64, 65, 4097))
    assert [w ** 3 % 32 for w, _ in pc.CELL_GRIDS] == [27, 0, 19, 27, 27]


def test_marked_cells_entry_refuses_bad_arguments_without_a_device():
    L = T.load_library()
    invalid = int(re.search(r"#define TMC2_E_INVALID (-?\d+)", open(os.path.join(ROOT, "include", "tmc2hip.h")).read()).group(1))
    p, cells = C.c_void_p(4096), C.c_uint32(0)                      # never dereferenced: every call below stops at its arguments
    assert L.tmc2_selftest_marked_cells(None, p, p, 8, 4, 0, 64, C.byref(cells), p, p, p, 1, p) == invalid
    assert b"selftest_marked_cells" in L.tmc2_last_error()
    for grid_size, bits, max_coord in ((1, 0, 64), (66, 0, 640), (3, 0, 64), (4, 15, 0), (4, 0, 40000), (4, 0, -1)):
        assert L.tmc2_selftest_marked_cells(p, p, p, 8, grid_size, bits, max_coord, C.byref(cells), p, p, p, 1, p) == invalid
    for grid_size, bits, max_coord in ((2, 14, 0), (4, 0, 0), (16, 3, 0)):       # more than 2^31 cells, none, none
        assert L.tmc2_selftest_marked_cells(p, p, p, 8, grid_size, bits, max_coord, C.byref(cells), p, p, p, 1, p) == invalid
        assert b"cells" in L.tmc2_last_error()


# ---- the cross-lane idioms of csrc/wave.h ------------------------------------------------------------------------------------
def test_wave_inputs_hold_what_the_cases_need():
    a = pc.wave_u32(64).reshape(len(pc.WAVE_U32_PATTERNS), 4, 64)
    assert not a[0].any() and (a[1] == 1).all() and (a[3] == 0xFFFFFFFF).all() and a[2, 3].tolist() == list(range(3000, 3064))
    for row, place in ((4, 0), (5, 63), (6, 32)):
        assert (np.count_nonzero(a[row], axis=1) == 1).all() and a[row, :, place].all() and len(set(a[row, :, place].tolist())) == 4
    assert len({w.tobytes() for w in a[7]}) == 4
    e = pc.wave_i32(True).reshape(-1, 64)
    assert e.dtype == np.int32 and all(w.min() == -(1 << 31) and w.max() == (1 << 31) - 1 for w in e) and set(e[0].tolist()) == {-(1 << 31), (1 << 31) - 1}
    s = pc.wave_i32(False)
    assert (s < 0).any() and (s > 0).any() and np.abs(s.astype(np.int64)).max() * 64 < 1 << 31
    d = pc.wave_f64()
    ex = np.frexp(np.abs(d))[1] - 1
    assert d.dtype == np.float64 and ex.min() <= -38 and ex.max() >= 38 and -40 <= ex.min() and ex.max() <= 40 and (d < 0).any() and (d > 0).any()
    p = pc.wave_predicates().reshape(len(pc.WAVE_PREDICATES), 4, 64)
    assert p.sum(axis=2).tolist()[:5] == [[0] * 4, [64] * 4, [32] * 4, [1] * 4, [1] * 4] and p[2, 0, 0] and p[2, 1, 1] and p[4, 0, 63]
    assert len(set(p[5].sum(axis=1).tolist())) > 1


def test_wave_references_are_the_plain_loops():
    """integers: the shuffle loop and the butterfly give the cumsum and the one sum / min / max of the group on every lane; float64:
    lane by lane in Python floats, the adds in the order of the loop -- and that order shows (not the left-to-right sum)"""
    for width in (64, 16):
        for a in (pc.wave_u32(64), pc.wave_i32(False), pc.wave_i32(True)):
            g = a.reshape(-1, width)
            if a.dtype == np.uint32 or np.abs(a.astype(np.int64)).max() < 1 << 24:
                assert np.array_equal(pc.wave_scan_reference(a, width), np.cumsum(g, axis=1, dtype=a.dtype).reshape(-1))
                assert np.array_equal(pc.wave_reduce_reference(a, np.add, width), np.repeat(g.sum(axis=1, dtype=a.dtype), width))
            assert np.array_equal(pc.wave_reduce_reference(a, np.minimum, width), np.repeat(g.min(axis=1), width))
            assert np.array_equal(pc.wave_reduce_reference(a, np.maximum, width), np.repeat(g.max(axis=1), width))
    d = pc.wave_f64(1)[:64]
    v = d.tolist()
    for off in (1, 2, 4, 8, 16, 32):
        v = [v[i] + v[i - off] if i >= off else v[i] for i in range(64)]
    assert pc.wave_scan_reference(d).view(np.uint64).tolist() == np.array(v).view(np.uint64).tolist()
    b = d.tolist()
    for off in (32, 16, 8, 4, 2, 1):
        b = [b[i] + b[i ^ off] for i in range(64)]
    got = pc.wave_reduce_reference(d, np.add)
    assert got.view(np.uint64).tolist() == np.array(b).view(np.uint64).tolist() and len(set(got.view(np.uint64).tolist())) == 1
    full = pc.wave_f64()
    left_to_right = np.array([sum(w.tolist()) for w in full.reshape(-1, 64)])
    assert (pc.wave_reduce_reference(full, np.add)[::64].view(np.uint64) != left_to_right.view(np.uint64)).any()


def test_wave_compaction_sort_and_block_scan_references():
    pred = pc.wave_predicates()
    out, count = pc.wave_compact_reference(pred)
    for w, (p, o, c) in enumerate(zip(pred.reshape(-1, 64).tolist(), out.reshape(-1, 64).tolist(), count.reshape(-1, 64).tolist())):
        lanes = [i for i in range(64) if p[i]]
        assert o == lanes + [pc.WAVE_NO_LANE] * (64 - len(lanes)) and c == [len(lanes)] * 64, w
    for length in pc.WAVE_SORT_LENGTHS:
        lists = pc.wave_sort_lists(length).reshape(len(pc.WAVE_SORT_KINDS), length)
        assert len(set(lists[0].tolist())) <= 7 and (np.diff(lists[2].astype(np.int64)) >= 0).all() and (np.diff(lists[3].astype(np.int64)) <= 0).all()
        valid = length - length // 4 - 3
        assert valid & (valid - 1) and (lists[1, valid:] == 0xFFFFFFFF).all() and (lists[1, :valid] == 0xFFFFFFFF).sum() >= 1
    for waves in pc.WAVE_BLOCK_WAVES:
        a = pc.wave_u32(64 * waves, groups=1)
        before, total = pc.wave_block_scan_reference(a, waves)
        for g, b, t in zip(a.reshape(-1, 64 * waves), before.reshape(-1, 64 * waves), total.reshape(-1, 64 * waves)):
            want, ref_total = pc.scan_reference(g)
            assert np.array_equal(b, want) and (t == ref_total).all(), waves


def test_wave_entry_refuses_bad_arguments_without_a_device():
    L = T.load_library()
    invalid = int(re.search(r"#define TMC2_E_INVALID (-?\d+)", open(os.path.join(ROOT, "include", "tmc2hip.h")).read()).group(1))
    p = C.c_void_p(4096)                                              # never dereferenced: every call below stops at its arguments
    ops = pc.WAVE_OPS
    assert L.tmc2_selftest_wave(None, ops["scan"], 0, p, p, None, 256) == invalid
    assert b"selftest_wave" in L.tmc2_last_error()
    for op, param, n, aux in ((-1, 0, 256, p), (9, 0, 256, p), (ops["sum"], 3, 256, None), (ops["min"], 0, 255, None), (ops["max"], 0, 0, None),
                              (ops["compact"], 0, 256, None), (ops["compact"], 0, 64, p), (ops["sort"], 32, 64, None), (ops["sort"], 96, 96, None),
                              (ops["sort"], 16384, 16384, None), (ops["sort"], 128, 192, None), (ops["block_scan"], 3, 192, p),
                              (ops["block_scan"], 4, 256, None), (ops["block_scan"], 16, 512, p), (ops["scan"], 0, (1 << 24) + 256, None)):
        assert L.tmc2_selftest_wave(p, op, param, p, p, aux, n) == invalid, (op, param, n)
    assert L.tmc2_selftest_wave(p, ops["scan"], 0, None, p, None, 256) == invalid and L.tmc2_selftest_wave(p, ops["scan"], 0, p, None, None, 256) == invalid
