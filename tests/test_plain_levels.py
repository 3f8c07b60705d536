"""The forest walk's plain levels (k_eval_forest, "plain levels"; rdf_set_plain_levels): while every tree slot of a wave is
walking and no fetched node has a leaf or exact flag, the level loop runs without leaf and finished-slot bookkeeping, and
hands over to the general loop at the first level that says otherwise.  The labels are the oracle's, bit for bit, and the
same with the knob at 0 (general loop from level 0) and at 1 in one process -- on forests that stay plain down to level
D-2, that leave the plain path at a planted node only a few lanes of a wave reach, that hold an exact node, a trained
topology, or a last level the last-level table cannot serve; on frames whose waves have inactive lanes; with full groups of
trees and groups with idle slots; in LDS levels and in levels read from the packed table."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

H, W, D, C = 40, 80, 9, 4       # 80 = one ordinary tile column + 16 columns of narrow tiles; 40 rows = two 16-row tiles + 8
TREES = (1, 2, 3, 4, 5, 8)
PLANTED_LEVELS = (0, 2, 3, D - 2)
VARIANTS = ("full",) + tuple(f"leaf{L}" for L in PLANTED_LEVELS) + ("exact", "trained", "no_last_level_table")


@pytest.fixture(scope="module")
def depth(rdf):
    """Two dense frames: invalid pixels (0 and 65535) scattered over the first, so that waves run with inactive lanes; two
    whole rows of the second invalid."""
    d = rdf.synth.frames(["dense", "dense"], 7100, H, W)
    rng = np.random.default_rng(71)
    holes = rng.random((H, W))
    d[0][holes < 0.15] = 0
    d[0][holes > 0.85] = 65535
    d[1][13, :] = 0
    d[1][30, :] = 65535
    return d


def _reaches(oracle, depth, forest, tree, level):
    """Which pixels' walks of `tree` end on `level`: the oracle's per-pixel visit counts (a walk that ends there read
    level + 1 records).  Returns that mask and the mask of the evaluated pixels."""
    lengths = oracle.walk_lengths(depth, forest)[..., tree]
    return lengths == level + 1, lengths > 0


def _plant_leaf(rdf, oracle, depth, T, level):
    """A full forest in which ONE side of ONE node of `level` in one tree is a leaf, picked so that some wave (the 64 pixels
    of a row of the ordinary tile column) has a lane that reaches it and a lane that walks on, and as few lanes reach it as
    that allows (the search stops at 32 pixels of the batch): the wave leaves the plain path there while most of its lanes
    keep walking."""
    full = rdf.synth.forest(T, D, C, "full", first_tree=300 + T)
    rng = np.random.default_rng(level)
    best = None
    for tree in reversed(range(T)):
        for node in range((1 << level) - 1, (1 << (level + 1)) - 1):
            for side in (0, 1):
                f = full.copy()
                f[tree, node, 5 + side] = 0.0       # floor != -1: this side is a leaf
                f[tree, node, 7 + side * C:7 + (side + 1) * C] = rng.integers(0, 257, C).astype(np.float32) / 256.0
                hit, evaluated = _reaches(oracle, depth, f, tree, level)
                wave_hit, wave_on = hit[:, :, :64], (evaluated & ~hit)[:, :, :64]
                split = (wave_hit.any(axis=2) & wave_on.any(axis=2)).any()
                if split and (best is None or hit.sum() < best[0]):
                    best = (int(hit.sum()), f, tree)
                    if best[0] <= 32:
                        return f, tree
    assert best is not None, f"no node of level {level} splits a wave: the case would test nothing"
    return best[1], best[2]


def _forest(variant, T, rdf, oracle, depth):
    if variant.startswith("leaf"):
        level = int(variant[4:])
        forest, tree = _plant_leaf(rdf, oracle, depth, T, level)
        # the condition on the inputs, from the oracle: a pixel reaches the planted leaf, a pixel of the same wave does not
        hit, evaluated = _reaches(oracle, depth, forest, tree, level)
        rows = hit[:, :, :64].any(axis=2) & (evaluated & ~hit)[:, :, :64].any(axis=2)
        assert rows.any() and hit.sum() >= 1
        return forest
    if variant == "trained":
        return rdf.synth.forest(T, D, C, "trained", first_tree=500 + T)
    forest = rdf.synth.forest(T, D, C, "full", first_tree=300 + T)
    if variant == "exact":
        walked = oracle.distinct_nodes_per_level(depth, forest)[:, 1] == 2          # trees whose level 1 is walked on both nodes
        assert walked.any()
        forest[int(np.nonzero(walked)[0][-1]), 2, 0] = 3.0e6        # level 1, a numerator >= 2^21: the record is flagged exact
    if variant == "no_last_level_table":
        forest[0, (1 << (D - 1)) - 1:, 5] = -1.0        # "continue" on level D-1: the loop runs all D levels
    return forest


def _eval(rdf, ev, f, d, prefill, filt=None, fcls=None):
    out = rdf.DeviceArray((d.shape[0], H, W), np.uint16).fill(prefill)
    ev.get_labels_forest(f, d, out, 1, filt, fcls)
    return out.get()


def _both_knobs(lib, run, want, what):
    got = {}
    for knob in (0, 1):
        lib.rdf_set_plain_levels(knob)
        got[knob] = run()
        assert np.array_equal(got[knob], want), (what, "plain levels", knob, int((got[knob] != want).sum()))
    assert np.array_equal(got[0], got[1]), what


@pytest.fixture()
def knobs(gpu_runtime):
    lib = gpu_runtime.lib
    yield lib
    lib.rdf_set_plain_levels(-1)
    lib.rdf_set_block_threads(0)
    lib.rdf_set_rows_per_wave(0)
    lib.rdf_set_lds_levels(-1)
    lib.rdf_set_group(0)
    lib.rdf_set_deep_from(-1)


def _throughput_geometry(lib):
    lib.rdf_set_block_threads(512)      # the kernels of a launch that fills the chip, on two small frames
    lib.rdf_set_rows_per_wave(2)        # 16-row tiles: two tile rows and a partial one
    lib.rdf_set_lds_levels(3)           # plain levels in LDS and in the packed table's records


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("T", TREES)
def test_labels_are_the_oracles_with_and_without_plain_levels(T, variant, rdf, oracle, depth, knobs, gpu_runtime):
    lib = knobs
    forest = _forest(variant, T, rdf, oracle, depth)
    want = oracle.eval_forest(depth, forest, np.full((2, H, W), 65535, np.uint16))
    ev = rdf.DecisionTreeEvaluator(use_packed=True)
    f, d = rdf.DecisionForest.from_numpy(forest), rdf.to_device(depth)
    _throughput_geometry(lib)
    # trees per lane by forest size (1, 2, 3 or 4: T = 5 ends on a group with three idle slots), and four-wide for the
    # small forests too (their one group has idle slots)
    for group in ((0, 4) if T < 4 else (0,)):
        lib.rdf_set_group(group)
        _both_knobs(lib, lambda: _eval(rdf, ev, f, d, 65535), want, (variant, T, "512 threads", group))
    lib.rdf_set_group(0)
    # the geometry a small launch takes by itself, once
    lib.rdf_set_block_threads(0)
    lib.rdf_set_rows_per_wave(0)
    _both_knobs(lib, lambda: _eval(rdf, ev, f, d[0:1], 65535), want[0:1], (variant, T, "default geometry"))


@pytest.mark.parametrize("topology", ["full", "trained"])
def test_filtered_and_deep_launches_do_not_depend_on_the_knob(topology, rdf, oracle, depth, knobs, gpu_runtime):
    lib = knobs
    forest = rdf.synth.forest(4, D, C, topology, first_tree=640)
    filt = (np.arange(2 * H * W).reshape(2, H, W) % 3).astype(np.uint16)
    want = oracle.eval_forest(depth, forest, np.full((2, H, W), 65535, np.uint16))
    want_f = oracle.eval_forest(depth, forest, np.full((2, H, W), 7, np.uint16), 1, filt, 1)
    ev = rdf.DecisionTreeEvaluator(use_packed=True)
    f, d, fd = rdf.DecisionForest.from_numpy(forest), rdf.to_device(depth), rdf.to_device(filt)
    _throughput_geometry(lib)
    _both_knobs(lib, lambda: _eval(rdf, ev, f, d, 7, fd, 1), want_f, (topology, "pixel list"))
    lib.rdf_set_deep_from(4)
    _both_knobs(lib, lambda: _eval(rdf, ev, f, d, 65535), want, (topology, "deep blocks"))
