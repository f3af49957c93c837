"""Normal orientation (S3) on the device over hand-built normal fields (orientation_cases.py): the parity union-find, the pair
table, the compact-graph scatter, the host walk over what they produce, the threshold ladder, the point-level fallback and the
majority flip -- each case set with `set_normals`, oriented with `normals_orient()` and compared bit for bit (signed zeros
included) with the oracle's growth.  The stage counters say which path ran; what they must show comes from the plain classifier
in orientation_cases.py (test_orientation_cases.py checks, without a GPU, that every figure waited for here occurs)."""
import numpy as np
import pytest

import orientation_cases as oc

pytestmark = pytest.mark.gpu

NAMES = oc.case_names()
TAUS = ["0.0", "0.5", "0.9", "0.9999", "1.0", "1.5", "1.6", "4"]
TAU_CASES = ["pca", "noisy", "palette", "random", "islands", "one_way_conflict", "mutual_conflict"]
HOOK_CASES = ["pca", "palette", "random", "noisy", "islands", "moebius_short"]
HOOKS = [("ORIENT_PAIRS", "4"), ("ORIENT_PAIRS", "8"), ("ORIENT_SPEC", "64,16"), ("ORIENT_SPEC", "1,2"), ("ORIENT_ORDER", "input"),
         ("ORIENT_ORDER", "chunk"), ("ORIENT_ORDER", "tree"), ("ORIENT_NO_CONTRACTION", "1"), ("UF_CHECK", "1"), ("UF_PRECHECK", "0"),
         ("UF_SCOPE", "agent")]
COUNTERS = ("orient_contract", "orient_tau_retry", "orient_normals_regrowth", "orient_pair_table_overflow", "orient_exact_size_repeat")


@pytest.fixture(scope="module")
def cases(oracle):
    return oc.all_cases(oracle)


def orient(gpu_ctx, c, what):
    """the case through the device: its own k-NN lists (they must be the oracle's), the case's field, one orientation.  Returns
    the stage counters; asserts the bits."""
    fr = gpu_ctx.frame(c.xyz)
    fr.normals_compute_normals(16)
    assert np.array_equal(fr.get_adjacency(16), c.knn), "k-NN lists differ from the oracle"
    fr.set_normals(c.normals)
    gpu_ctx.stage_reset()
    fr.normals_orient()
    calls = gpu_ctx.stage_calls()
    got = {k: calls.get(k, 0) for k in COUNTERS}
    print("ORIENT %s n=%d %s" % (what, len(c.xyz), " ".join("%s=%d" % (k[7:], v) for k, v in got.items())))
    wrong = (fr.get_normals().view(np.uint64) != c.expected.view(np.uint64)).any(1)
    assert not wrong.any(), "%d of %d normals differ from the oracle, first at point %d" % (wrong.sum(), len(wrong), np.argmax(wrong))
    return got


def assert_path(got, path):
    retries, regrowth = path
    assert (got["orient_contract"], got["orient_tau_retry"], got["orient_normals_regrowth"]) == (retries + 1, retries, regrowth)


@pytest.mark.parametrize("name", NAMES)
def test_gpu_orientation_case(gpu_ctx, cases, name):
    c = cases[name]
    got = orient(gpu_ctx, c, name)
    assert c.path() is not None
    assert_path(got, c.path())
    assert got["orient_pair_table_overflow"] == 0 and got["orient_exact_size_repeat"] == 0   # (2^20 pairs, 384 K edges: room for any case here)


@pytest.mark.parametrize("tau", TAUS)
@pytest.mark.parametrize("name", TAU_CASES)
def test_gpu_orientation_first_threshold(gpu_ctx, ctx_options, cases, name, tau):
    """ORIENT_TAU from "every edge is strong" to "none is": the ladder starts there, and above 1.5 the hook switches the contraction
    off (no contraction, no retry, and the point-level walk is no fallback then)."""
    c = cases[name]
    ctx_options.setenv("TMC2_ORIENT_TAU", tau)
    got = orient(gpu_ctx, c, "%s ORIENT_TAU=%s" % (name, tau))
    if float(tau) > oc.NO_CONTRACTION_ABOVE:
        assert (got["orient_contract"], got["orient_tau_retry"], got["orient_normals_regrowth"]) == (0, 0, 0)
    elif c.path(float(tau)) is not None:
        assert_path(got, c.path(float(tau)))


@pytest.mark.parametrize("hook,value", HOOKS)
@pytest.mark.parametrize("name", HOOK_CASES)
def test_gpu_orientation_hooks(gpu_ctx, ctx_options, cases, name, hook, value):
    """The forms of the device passes: a pair table too small for the frame (the walk gets every cross edge), speculative room too
    small (the scatter is repeated with exact sizes), the three pass orders, the point-level walk alone, the union-find's debug
    check, its unions without the stale-view shortcut and with agent-scope loads -- same bits, and the same path."""
    c = cases[name]
    ctx_options.setenv("TMC2_" + hook, value)
    got = orient(gpu_ctx, c, "%s %s=%s" % (name, hook, value))
    if hook == "ORIENT_NO_CONTRACTION":
        assert (got["orient_contract"], got["orient_tau_retry"], got["orient_normals_regrowth"]) == (0, 0, 0)
        return
    assert_path(got, c.path())
    tau = c.final_tau()                                              # the rung whose compact graph reaches the host
    if hook == "ORIENT_PAIRS" and tau is not None and c.cross_pairs(tau) > (1 << int(value)):
        assert got["orient_pair_table_overflow"] == 1
    if hook == "ORIENT_SPEC" and tau is not None:
        clusters, edges = c.compact_size(tau)
        room_edges, room_records = (int(x) for x in value.split(","))
        assert got["orient_exact_size_repeat"] == int(edges > room_edges or clusters + 1 > room_records)
        # (under this hook the stage table also carries the size of the compact graph: per pair of clusters ALL the light edges
        #  that tie at the best weight and one strong edge per sign, no more and no fewer)
        assert gpu_ctx.stage_ms()["orient_compact_edges"] == edges
