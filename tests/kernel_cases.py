"""One oracle-compared launch per k_eval_forest instantiation, made by rule (no GPU needed here).

kForestKernels in 3d-beats_amd/csrc/rdf_launch_plan.hpp lists the instantiations librdf_hip.so has; `keys()` parses that
block, so the list stays in one place.  `case_for(key)` gives the request (entry point, forests, filter) and the knob settings
meant to reach that key through the C ABI; a key no rule covers raises, so a kernel added to the list gets a case or a loud
error.  `check_case` holds a case's own preconditions (trees and classes agree with the key's width and `cmax`, depth inside
the deep blocks' limits, label maps small enough for tree waves): what has to be true of the CASE before a failure on the GPU
may be read as a failure of the kernel or of the selection.  tests/test_kernel_coverage.py runs the cases."""
import os
import re
from collections import namedtuple

import numpy as np

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "3d-beats_amd", "csrc", "rdf_launch_plan.hpp")

FIELDS = ("block", "packed", "cmax", "stats", "group", "compact", "nl", "tw", "deep")     # struct KernelKey, in its order
Key = namedtuple("Key", FIELDS)

# ---- the frames and the two launches every case makes ----
FRAME_KINDS, FRAME_SEED, FRAME_H, FRAME_W = ["dense", "live"], 6500, 37, 131
# labels_reduce, scale factor, pre-fill.  131 = 2 x 64 + 3 label columns: a narrow-tile column (fold 4) and a ragged last tile
# row; at labels_reduce 2 the label map is 18 x 65, again with a one-pixel narrow column.
Launch = namedtuple("Launch", "reduce scale prefill")
LAUNCHES = (Launch(1, 1.0, 65535), Launch(2, 0.5, 0))
FILTER_CLASS = 1            # filtered cases: a random filter map over {0, 1, 2}, evaluated where it holds 1
TW_MAX_LABEL_PIXELS = 131072
DEPTH = 10                  # every forest but the deep ones
DEEP_DEPTH, DEEP_FROM = 11, 4
DEEP_CALIBRATION = (4, 120, 212)    # frames the balanced topology takes its medians from (synth.calibration_frames)

ForestSpec = namedtuple("ForestSpec", "trees depth classes topology first", defaults=(0,))     # (first: synth's first_tree)
# knobs: what rdf_set_block_threads / rdf_set_tree_waves / rdf_set_deep_from / rdf_set_group get (their "unset" otherwise);
# forests: one ForestSpec (several for a layered stack, layer i > 0 filtering on layer i - 1's class LAYER_FILTER_CLASS[i])
Variant = namedtuple("Variant", "knobs forests filtered")
# entry: "packed" rdf_eval_forest_packed, "reference" rdf_eval_forest (DecisionTreeEvaluator with and without use_packed),
# "stats" rdf_eval_forest_stats, "packed_stats" rdf_eval_forest_packed_stats, "layers" LayeredDecisionForest.run
Case = namedtuple("Case", "key entry variants")
LAYER_FILTER_CLASS = (None, 2, 1)

UNSET = {"block": 0, "tree_waves": -1, "deep_from": -1, "group": 0}


def keys(path=HEADER):
    """The entries of kForestKernels, in the list's order."""
    src = open(path).read()
    m = re.search(r"constexpr\s+KernelKey\s+kForestKernels\[\]\s*=\s*\{(.*?)\n\};", src, re.S)
    if m is None:
        raise ValueError(f"no kForestKernels block in {path}")
    body = re.sub(r"//[^\n]*", "", m.group(1))
    out = []
    for entry in re.findall(r"\{([^{}]*)\}", body):
        words = [w.strip() for w in entry.split(",")]
        if len(words) != len(FIELDS):
            raise ValueError(f"kForestKernels entry {{{entry}}} has {len(words)} fields, KernelKey has {len(FIELDS)}")
        out.append(Key(*[{"true": True, "false": False}[w] if w in ("true", "false") else int(w) for w in words]))
    if not out or len(set(out)) != len(out):
        raise ValueError(f"kForestKernels in {path}: {len(out)} entries, {len(set(out))} distinct")
    return out


def key_id(key):
    """b512-packed-c8-g3-deep"""
    parts = [f"b{key.block}", "packed" if key.packed else "ref", f"c{key.cmax}", f"g{key.group}"]
    parts += [name for name, on in (("stats", key.stats), ("compact", key.compact), (f"nl{key.nl}", key.nl > 1), ("tw", key.tw),
                                    ("deep", key.deep)) if on]
    return "-".join(parts)


def key_fields(key):
    """The nine fields as rdf_debug_kernel_key returns them (bools as 0 / 1)."""
    return [int(v) for v in key]


# ---- the rules ----
# trees that make a forest take the `group`-wide kernel by its size (group_for), per workgroup size: 6 trees are two passes of
# the 3-wide kernel, 5 a second pass of the 4-wide one with three idle slots
PACKED_TREES = {256: {1: 1, 2: 2, 3: 6, 4: 5}, 512: {1: 1, 2: 2, 3: 3, 4: 8}}
PACKED_TREES_C16 = {1: 1, 4: 7}             # the sixteen-class kernels exist one- and four-wide only
PACKED_CLASSES = {256: {4: 3, 8: 5, 16: 9}, 512: {4: 4, 8: 8, 16: 16}}
COMPACT_TREES = 4
REFERENCE_TREES = {1: 1, 4: 5}
REFERENCE_CLASSES = {256: {4: 4, 16: 5}, 512: {4: 4, 16: 17}}
REFERENCE_FILTERED = (512, 4)               # the (block, width) that runs filtered: the per-lane early-outs
# deep blocks: a single tree walks the two-wide kernel with one slot idle
DEEP_TREES = {256: {2: 1, 3: 3, 4: 4}, 512: {2: 2, 3: 6, 4: 5}}
DEEP_CLASSES = {4: 3, 8: 7}
TW_TREES = (2, 3, 4)                        # at 3 a workgroup holds two rows and leaves two waves without a tree
TW_CLASSES = {4: 4, 8: 6}
# the layers of a stack as (trees, classes); every layer has 2 to 4 trees (tree waves can take it), cmax 8: one has 5 to 8 classes
LAYER_STACKS = {4: ((3, 4), (4, 3), (2, 4)), 8: ((3, 4), (4, 6), (2, 8))}


def _no_rule(key, why):
    return ValueError(f"tests/kernel_cases.py has no rule for kForestKernels entry {key_id(key)} {tuple(key)}: {why}")


def _knobs(**set_):
    return dict(UNSET, **set_)


def _single(key, entry, knobs, trees, depth, classes, topology="trained", filtered=False):
    return Case(key, entry, (Variant(knobs, (ForestSpec(trees, depth, classes, topology),), filtered),))


def _layers_case(key):
    if not (key.packed and not key.stats and not key.compact and not key.deep and key.nl in (2, 3) and key.cmax in LAYER_STACKS):
        raise _no_rule(key, "layers in one launch are packed, 2 or 3 layers, 4 or 8 classes")
    stack = [ForestSpec(t, DEPTH, c, "trained", 20 * i) for i, (t, c) in enumerate(LAYER_STACKS[key.cmax][:key.nl])]
    if key.tw:
        if (key.block, key.group) != (512, 1):
            raise _no_rule(key, "tree waves are 512 threads, one tree a lane")
        return Case(key, "layers", (Variant(_knobs(), tuple(stack), True),))
    if (key.block, key.group) != (256, 4):
        raise _no_rule(key, "the trees-in-a-lane form is 256 threads, four wide")
    # reached once with tree waves switched off, and once by a layer of one tree: layered_run then plans a second time.  (The
    # FIRST layer: a later layer is compared with the first one's tiles while that one is still planned as tree waves, so a
    # stack whose first layer can take tree waves and a later one cannot is evaluated layer by layer.)
    one_tree = list(stack)
    one_tree[0] = one_tree[0]._replace(trees=1)
    return Case(key, "layers", (Variant(_knobs(tree_waves=0), tuple(stack), True), Variant(_knobs(), tuple(one_tree), True)))


def _tree_wave_case(key):
    if not (key.packed and not key.stats and not key.compact and not key.deep and (key.block, key.group) == (512, 1)
            and key.cmax in TW_CLASSES):
        raise _no_rule(key, "tree waves are packed, 512 threads, one tree a lane, 4 or 8 classes")
    # (block knob unset: tree waves are chosen for launches that would take 256 threads)
    return Case(key, "packed", tuple(Variant(_knobs(), (ForestSpec(t, DEPTH, TW_CLASSES[key.cmax], "trained"),), False)
                                     for t in TW_TREES))


def _stats_case(key):
    if key.compact or key.group != 4 or key.cmax != 4:
        raise _no_rule(key, "the counting kernels are four wide, classes four at a time, no pixel list")
    if not key.packed:
        if key.block != 256 or key.deep:
            raise _no_rule(key, "rdf_eval_forest_stats launches 256 threads")
        return _single(key, "stats", _knobs(tree_waves=0), 4, DEPTH, 6)
    if key.deep:
        return _single(key, "packed_stats", _knobs(block=key.block, tree_waves=0, deep_from=DEEP_FROM), 4, DEEP_DEPTH, 4, "balanced")
    return _single(key, "packed_stats", _knobs(block=key.block, tree_waves=0, deep_from=0), 4, DEPTH, 4)


def _deep_case(key):
    if not key.packed or key.cmax not in DEEP_CLASSES:
        raise _no_rule(key, "deep blocks serve packed forests of up to eight classes")
    knobs = _knobs(block=key.block, tree_waves=0, deep_from=DEEP_FROM)
    if key.compact:
        if key.group != 4:
            raise _no_rule(key, "the pixel-list kernels are four wide")
        return _single(key, "packed", knobs, COMPACT_TREES, DEEP_DEPTH, DEEP_CLASSES[key.cmax], "balanced", True)
    if key.group not in DEEP_TREES[key.block]:
        raise _no_rule(key, "no forest size takes this width")
    return _single(key, "packed", knobs, DEEP_TREES[key.block][key.group], DEEP_DEPTH, DEEP_CLASSES[key.cmax], "balanced")


def _reference_case(key):
    if key.compact or key.group not in REFERENCE_TREES or key.cmax not in REFERENCE_CLASSES[key.block]:
        raise _no_rule(key, "the reference layout is walked one or four wide, 4 or 16 classes, without a pixel list")
    return _single(key, "reference", _knobs(block=key.block, tree_waves=0), REFERENCE_TREES[key.group], DEPTH,
                   REFERENCE_CLASSES[key.block][key.cmax], filtered=(key.block, key.group) == REFERENCE_FILTERED)


def _packed_case(key):
    if key.cmax not in PACKED_CLASSES[key.block]:
        raise _no_rule(key, "packed forests keep 4, 8 or 16 classes in registers")
    knobs = _knobs(block=key.block, tree_waves=0)
    classes = PACKED_CLASSES[key.block][key.cmax]
    if key.compact:
        if key.group != 4:
            raise _no_rule(key, "the pixel-list kernels are four wide")
        return _single(key, "packed", knobs, COMPACT_TREES, DEPTH, classes, filtered=True)
    trees = PACKED_TREES_C16 if key.cmax == 16 else PACKED_TREES[key.block]
    if key.group not in trees:
        raise _no_rule(key, "no forest size takes this width")
    return _single(key, "packed", knobs, trees[key.group], DEPTH, classes)


def case_for(key):
    """The request and the knob settings meant to reach `key`."""
    key = Key(*key)
    if key.block not in (256, 512) or key.nl not in (1, 2, 3):
        raise _no_rule(key, "workgroups of 256 or 512 threads, one to three argument sets")
    if key.nl > 1:
        return _layers_case(key)
    if key.tw:
        return _tree_wave_case(key)
    if key.stats:
        return _stats_case(key)
    if key.deep:
        return _deep_case(key)
    if not key.packed:
        return _reference_case(key)
    return _packed_case(key)


def extra_cases():
    """Kernels already counted, reached through other loops: rdf_set_group makes the width differ from the forest's natural one
    (two trees four wide; five trees two wide: three passes, the last half idle; three trees one after the other)."""
    out = []
    for trees, group in ((2, 4), (5, 2), (3, 1)):
        key = Key(256, True, 4, False, group, False, 1, False, False)
        out.append(_single(key, "packed", _knobs(block=256, tree_waves=0, group=group), trees, DEPTH, 4))
    return out


def extra_id(case):
    return f"{key_id(case.key)}-T{case.variants[0].forests[0].trees}"


def launches_expected(case):
    return len(case.variants) * len(LAUNCHES)


# ---- a case's own preconditions ----
def natural_width(trees):
    """Trees a lane walks interleaved when nothing forces a width (group_for)."""
    return 1 if trees == 1 else 2 if trees == 2 else 3 if trees in (3, 6) else 4


def width_taken(trees, classes, packed, deep, compact, forced=0):
    """... and the width of the kernel such a forest is given (select_kernel)."""
    g = forced if forced > 0 else natural_width(trees)
    if compact:
        return 4
    if not packed:
        return 1 if g == 1 else 4
    if deep:
        return 2 if g <= 2 else g
    return g if g == 1 or (g in (2, 3) and classes <= 8) else 4


def classes_kept(classes, packed, deep):
    """`cmax` of the kernel a forest of `classes` classes is given."""
    if deep:
        return 4 if classes <= 4 else 8
    if not packed:
        return 4 if classes <= 4 else 16
    return 4 if classes <= 4 else 8 if classes <= 8 else 16


def label_shape(launch, n=len(FRAME_KINDS)):
    return (n, FRAME_H // launch.reduce, FRAME_W // launch.reduce)


def check_case(case, known):
    """Raises AssertionError naming what is wrong with the case itself."""
    key, what = case.key, key_id(case.key)
    assert key in known, f"{what}: not an entry of kForestKernels"
    assert case.variants, f"{what}: a case without a launch"
    assert case.entry in ("packed", "reference", "stats", "packed_stats", "layers"), (what, case.entry)
    assert (case.entry in ("stats", "packed_stats")) == key.stats and (case.entry == "layers") == (key.nl > 1), (what, case.entry)
    assert (case.entry in ("reference", "stats")) == (not key.packed), (what, case.entry)
    for v in case.variants:
        k = v.knobs
        assert set(k) == set(UNSET), (what, k)
        assert len(v.forests) == key.nl, f"{what}: {len(v.forests)} forests for {key.nl} argument sets"
        for launch in LAUNCHES:
            # small launches: the workgroup size is the knob's, and the label map has a narrow column
            n, hl, wl = label_shape(launch, 1 if key.nl > 1 else len(FRAME_KINDS))
            assert wl > 64 and 0 < wl % 64 <= 16 and hl % 4 != 0, (what, hl, wl)
            if key.tw:
                assert n * hl * wl <= TW_MAX_LABEL_PIXELS, f"{what}: {n * hl * wl} label pixels are too many for tree waves"
        for f in v.forests:
            assert f.trees >= 1 and 1 <= f.depth <= 27 and f.classes >= 2, (what, f)
            if key.deep:
                assert f.topology == "balanced" and 5 <= f.depth <= 24 and f.classes <= 8, f"{what}: {f} cannot have deep blocks"
                assert 0 < k["deep_from"] <= f.depth - (2 if f.classes <= 4 else 1), (what, k)
            else:
                assert k["deep_from"] <= 0 or case.entry != "packed_stats", (what, k)
        if key.tw:
            assert k["block"] == 0 and k["tree_waves"] != 0, f"{what}: tree waves need the block and tree-wave knobs unset"
            assert all(2 <= f.trees <= 4 and f.classes <= 8 for f in v.forests), (what, v.forests)
            assert not v.filtered or key.nl > 1, what
        elif key.nl > 1:
            assert k["block"] == 0, (what, k)
            assert k["tree_waves"] == 0 or any(not 2 <= f.trees <= 4 for f in v.forests), f"{what}: every layer can take tree waves"
        else:
            assert k["tree_waves"] == 0, f"{what}: forests of 2 to 4 trees would go to tree waves"
            assert key.stats and not key.packed or k["block"] == key.block, (what, k)
        if key.nl > 1:
            assert max(classes_kept(f.classes, True, False) for f in v.forests) == key.cmax, (what, v.forests)
            assert all(f.classes <= 8 and f.classes > LAYER_FILTER_CLASS[i + 1] for i, f in enumerate(v.forests[:-1])), (what, v.forests)
            continue
        f = v.forests[0]
        if key.stats:
            assert f.classes <= 4 or not key.packed, f"{what}: the packed counting kernels keep four classes"
            continue
        assert classes_kept(f.classes, key.packed, key.deep) == key.cmax, f"{what}: {f.classes} classes do not take cmax {key.cmax}"
        assert v.filtered == key.compact or not key.packed, f"{what}: a filtered packed launch lists its pixels"
        if not key.tw:
            got = width_taken(f.trees, f.classes, key.packed, key.deep, key.compact, k["group"])
            assert got == key.group, f"{what}: {f.trees} trees take the {got}-wide kernel"


# ---- the inputs, the same for every test that asks ----
_cache = {}


def frames(synth):
    if "frames" not in _cache:
        _cache["frames"] = synth.frames(FRAME_KINDS, FRAME_SEED, FRAME_H, FRAME_W)
        _cache["frames"].setflags(write=False)
    return _cache["frames"].copy()          # (the cached one stays as it is)


def filter_map(launch):
    """uint16 over {0, 1, 2}, one per launch shape."""
    k = ("filter", launch)
    if k not in _cache:
        _cache[k] = np.random.default_rng(FRAME_SEED + launch.reduce).integers(0, 3, size=label_shape(launch)).astype(np.uint16)
        _cache[k].setflags(write=False)
    return _cache[k].copy()


def forest(synth, spec):
    """synth.forest for `spec`: the first `trees` trees of one forest per (depth, classes, topology, first tree)."""
    k = ("forest", spec.depth, spec.classes, spec.topology, spec.first)
    if k not in _cache or _cache[k].shape[0] < spec.trees:
        most = max(8, spec.trees)
        calib = synth.calibration_frames(*DEEP_CALIBRATION) if spec.topology == "balanced" else None
        _cache[k] = synth.forest(most if spec.topology != "balanced" else max(6, spec.trees), spec.depth, spec.classes, spec.topology,
                                 spec.first, calib=calib)
        _cache[k].setflags(write=False)
    return _cache[k][:spec.trees].copy()


def stack_conditions(classes):
    """The conditions table of a stack whose layer i > 0 filters on layer i - 1's class LAYER_FILTER_CLASS[i]: that label
    leads on to the next layer's rows, every other label 1 .. C - 1 is final with an id of its own.  Returns (rows, ids)."""
    rows, next_id, off = [], 1, 0
    for i, c in enumerate(classes):
        off += c - 1
        for label in range(1, c):
            if i + 1 < len(classes) and label == LAYER_FILTER_CLASS[i + 1]:
                rows.append([1, off])
            else:
                rows.append([0, next_id])
                next_id += 1
    return rows, next_id - 1
