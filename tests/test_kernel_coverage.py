"""Every k_eval_forest instantiation of librdf_hip.so is launched once through the C ABI, compared with the oracle bit for bit,
and PROVEN to be the kernel that ran: the library counts its launches per entry of kForestKernels
(rdf_debug_kernel_launches), and after a case exactly its own kernel has been counted, exactly as often as the case launched.
tests/kernel_cases.py makes the cases by rule from the list in rdf_launch_plan.hpp; the tests of its rules need no GPU.
Labels and counters are integers and compared exactly.  (The 70 GPU tests of this module take 4 s together on an MI355X.)"""
import ctypes

import numpy as np
import pytest

import kernel_cases as kc

KEYS = kc.keys()
EXTRA = kc.extra_cases()

# every rdf_set_* knob and the value that means "nothing set"
KNOBS_AT_REST = {"lds_budget_bytes": 0, "block_threads": 0, "scheduler": -1, "compaction": -1, "halo": -1, "group": 0,
                 "layers_one_launch": -1, "lds_levels": -1, "tree_waves": -1, "stage_vec": -1, "rows_per_wave": 0, "force_exact": 0,
                 "last_level_table": -1, "deep_from": -1, "fold": -1, "plain_levels": -1}


# ---- the rules (no GPU) ----
def test_the_parsed_list_is_the_headers():
    assert len(KEYS) == 65 and len({kc.key_id(k) for k in KEYS}) == len(KEYS)
    src = open(kc.HEADER).read()
    assert f"({len(KEYS)} kernels;" in src                      # (the comment above the list counts them too)
    assert KEYS[0] == kc.Key(256, True, 4, False, 1, False, 1, False, False)
    assert KEYS[-1] == kc.Key(256, True, 8, False, 4, False, 3, False, False)


@pytest.mark.parametrize("key", KEYS, ids=kc.key_id)
def test_every_key_has_a_case_whose_preconditions_hold(key):
    case = kc.case_for(key)
    assert case.key == key
    kc.check_case(case, KEYS)
    assert kc.launches_expected(case) == len(kc.LAUNCHES) * len(case.variants) >= 2


def test_no_case_names_a_key_outside_the_list():
    for case in [kc.case_for(k) for k in KEYS] + EXTRA:
        assert case.key in KEYS, case.key
    for case in EXTRA:
        kc.check_case(case, KEYS)
        v = case.variants[0]
        assert v.knobs["group"] != kc.natural_width(v.forests[0].trees)       # another loop than the forest's own case runs
    # a kernel added to the list without a rule is a loud error, and so is a case whose forest does not fit its key
    for unknown in (kc.Key(768, True, 4, False, 4, False, 1, False, False), kc.Key(256, True, 16, False, 2, False, 1, False, False),
                    kc.Key(256, True, 16, False, 4, False, 1, False, True), kc.Key(512, False, 8, False, 4, False, 1, False, False),
                    kc.Key(256, True, 4, False, 4, False, 4, False, False)):
        assert unknown not in KEYS
        with pytest.raises(ValueError, match="no rule"):
            kc.case_for(unknown)
    wrong = kc.case_for(kc.Key(256, True, 4, False, 3, False, 1, False, False))
    bad = wrong._replace(variants=(wrong.variants[0]._replace(forests=(wrong.variants[0].forests[0]._replace(trees=5),)),))
    with pytest.raises(AssertionError, match="4-wide"):
        kc.check_case(bad, KEYS)


# ---- on the GPU ----
@pytest.fixture()
def lib(gpu_runtime):
    """The library with every knob at rest, before and after."""
    lib = gpu_runtime.lib

    def rest():
        for name, value in KNOBS_AT_REST.items():
            getattr(lib, "rdf_set_" + name)(value)
    rest()
    try:
        yield lib
    finally:
        rest()


@pytest.fixture(scope="module")
def evs(rdf, gpu_runtime):
    return {"packed": rdf.DecisionTreeEvaluator(use_packed=True), "reference": rdf.DecisionTreeEvaluator(use_packed=False)}


def _counters(lib, reset=0):
    out = (ctypes.c_ulonglong * len(KEYS))()
    assert lib.rdf_debug_kernel_launches(out, len(KEYS), reset) == len(KEYS)
    return [int(v) for v in out]


def _set_knobs(lib, knobs):
    lib.rdf_set_block_threads(knobs["block"])
    lib.rdf_set_tree_waves(knobs["tree_waves"])
    lib.rdf_set_deep_from(knobs["deep_from"])
    lib.rdf_set_group(knobs["group"])


def _blocks_can_serve(rdf, gpu_runtime, f, forest_np, scale, what):
    """The case is wrong, not the kernel, if the table's deep blocks cannot serve the forest: no node needs the exact numerators
    (rdf_forest_info), every node of the last level is a plain two-leaf node."""
    exact = ctypes.c_int(-1)
    rc = gpu_runtime.lib.rdf_forest_info(f.packed(scale).ptr, int(f.num_trees), int(f.max_depth), int(f.num_classes), gpu_runtime.stream(),
                                         None, ctypes.byref(exact), None)
    assert rc == 0 and exact.value == 0, f"the case is wrong ({what}): {exact.value} nodes need the exact numerators (rc {rc})"
    last = forest_np[:, (1 << (f.max_depth - 1)) - 1:, 5:7]
    assert (last == 0.0).all(), f"the case is wrong ({what}): a node of the last level is not a plain two-leaf node"


def _run_forest(case, v, rdf, gpu_runtime, evs, oracle):
    """Both launches of a variant.  Returns [(what, got, want), ...]; nothing is compared yet."""
    lib, synth = gpu_runtime.lib, rdf.synth
    depth_np = kc.frames(synth)
    spec = v.forests[0]
    forest_np = kc.forest(synth, spec)
    f = rdf.DecisionForest.from_numpy(forest_np)
    depth = rdf.to_device(depth_np)
    n, h, w = depth_np.shape
    out = []
    for launch in kc.LAUNCHES:
        what = (kc.key_id(case.key), tuple(spec), launch)
        filt = kc.filter_map(launch) if v.filtered else None
        fcls = kc.FILTER_CLASS if v.filtered else None
        want = np.full(kc.label_shape(launch), launch.prefill, np.uint16)
        st = np.zeros(3, np.uint64)
        oracle.eval_forest(depth_np, forest_np, want, launch.reduce, filt, fcls, launch.scale, stats=st)
        assert 0 < int(st[0]) < want.size, what                     # (some pixels evaluated, some left alone)
        if case.key.deep:
            _blocks_can_serve(rdf, gpu_runtime, f, forest_np, launch.scale, what)
        labels = rdf.DeviceArray(want.shape, np.uint16).fill(launch.prefill)
        if case.entry in ("packed", "reference"):
            evs[case.entry].get_labels_forest(f, depth, labels, launch.reduce, rdf.to_device(filt) if v.filtered else None, fcls,
                                              launch.scale)
            out.append((what, labels.get(), want))
            continue
        wide = case.entry == "packed_stats"
        counters = rdf.DeviceArray((8 if wide else 3,), np.uint64).fill(0)
        if wide:
            rc = lib.rdf_eval_forest_packed_stats(depth.ptr, n, w, h, f.packed(launch.scale).ptr, f.forest_cu.ptr, spec.trees, spec.depth,
                                                  spec.classes, labels.ptr, launch.reduce, counters.ptr, gpu_runtime.stream())
        else:
            rc = lib.rdf_eval_forest_stats(depth.ptr, n, w, h, f.forest_cu.ptr, spec.trees, spec.depth, spec.classes, None, -1, labels.ptr,
                                           launch.reduce, launch.scale, counters.ptr, gpu_runtime.stream())
        assert rc == 0, (what, rc)
        out.append((what, labels.get(), want))
        out.append((what + ("pixels, visits, leaves",), counters.get()[0:3].astype(np.uint64), st))
    return out


def _run_layers(case, v, rdf, gpu_runtime, oracle):
    """One frame through LayeredDecisionForest.run, at both launch shapes: every layer image and the composite."""
    synth = rdf.synth
    forests = [kc.forest(synth, s) for s in v.forests]
    cond, n_ids = kc.stack_conditions([s.classes for s in v.forests])
    layers = [{"model": rdf.DecisionForest.from_numpy(forests[0])}]
    for i in range(1, len(forests)):
        layers.append({"model": rdf.DecisionForest.from_numpy(forests[i]), "filter_model": i - 1,
                       "filter_model_class": kc.LAYER_FILTER_CLASS[i]})
    cfg = {"layers": layers, "conditions": cond, "label_colors": [[1, 2, 3, 255]] * n_ids}
    out = []
    for k, launch in enumerate(kc.LAUNCHES):
        what = (kc.key_id(case.key), tuple(tuple(s) for s in v.forests), launch)
        frame = kc.frames(synth)[k:k + 1]                   # the dense frame at full resolution, the live one at labels_reduce 2
        shape = kc.label_shape(launch, 1)
        want = []
        for i, forest_np in enumerate(forests):
            img = np.full(shape, 65535, np.uint16)
            oracle.eval_forest(frame, forest_np, img, launch.reduce, want[i - 1] if i else None, kc.LAYER_FILTER_CLASS[i], launch.scale)
            want.append(img)
        comp = np.full(shape, 65535, np.uint16)
        assert oracle.composite([img[0] for img in want], np.array(cond, np.int32), comp) == 0, what
        if k == 0:      # (the dense frame: every layer labels some pixels, and the composite holds final ids of the last layer)
            assert all((img != 65535).any() for img in want) and int(comp[comp != 65535].max()) > n_ids - v.forests[-1].classes + 1, what
        lf = rdf.LayeredDecisionForest(cfg, (kc.FRAME_H, kc.FRAME_W), launch.reduce)
        depth = rdf.GpuBuffer((kc.FRAME_H, kc.FRAME_W), np.uint16)
        labels = rdf.GpuBuffer(shape[1:], np.uint16)
        depth.cu().set(frame[0])
        labels.cu().fill(4242)
        lf.run(depth, labels, launch.scale)
        for i, img in enumerate(want):
            out.append((what + (f"layer {i}",), lf.label_images[i].cu().get(), img[0]))
        out.append((what + ("composite",), labels.cu().get(), comp[0]))
        out.append((what + ("invalid composite walks",), np.array(lf.eval.composite_bad_pixels()), np.array(0)))
    return out


def _run_case(case, lib, rdf, gpu_runtime, evs, oracle):
    _counters(lib, reset=1)
    results = []
    for v in case.variants:
        _set_knobs(lib, v.knobs)
        if case.entry == "layers":
            results += _run_layers(case, v, rdf, gpu_runtime, oracle)
        else:
            results += _run_forest(case, v, rdf, gpu_runtime, evs, oracle)
    # which kernel ran comes first, so that a routing error reads as one: this kernel as often as the case launched, no other
    counted = {kc.key_id(k): c for k, c in zip(KEYS, _counters(lib)) if c}
    differ = sum(not np.array_equal(got, want) for _, got, want in results)
    assert counted == {kc.key_id(case.key): kc.launches_expected(case)}, \
        f"launched {counted} ({differ} of {len(results)} results differ from the oracle's)"
    for what, got, want in results:
        assert np.array_equal(got, want), (what, f"{int((np.asarray(got) != np.asarray(want)).sum())} of {np.asarray(want).size} differ")


@pytest.mark.gpu
def test_the_library_names_the_kernels_of_the_list(lib):
    assert lib.rdf_debug_kernel_launches(None, 0, 0) == len(KEYS)
    for i, key in enumerate(KEYS):
        got = (ctypes.c_int * 9)(*([-7] * 9))
        assert lib.rdf_debug_kernel_key(i, got) == 0
        assert list(got) == kc.key_fields(key), (i, kc.key_id(key), list(got))
    untouched = (ctypes.c_int * 9)(*([-7] * 9))
    for outside in (-1, len(KEYS), 1 << 20):
        assert lib.rdf_debug_kernel_key(outside, untouched) == -1           # RDF_ERR_BAD_ARG
    assert list(untouched) == [-7] * 9
    # fewer entries asked for than there are: only those are written
    few = (ctypes.c_ulonglong * 4)(*([99] * 4))
    assert lib.rdf_debug_kernel_launches(few, 3, 1) == len(KEYS) and few[3] == 99


@pytest.mark.gpu
@pytest.mark.parametrize("key", KEYS, ids=kc.key_id)
def test_each_kernel_is_reached_and_gives_the_oracles_labels(key, lib, rdf, gpu_runtime, evs, oracle):
    _run_case(kc.case_for(key), lib, rdf, gpu_runtime, evs, oracle)


@pytest.mark.gpu
@pytest.mark.parametrize("case", EXTRA, ids=kc.extra_id)
def test_a_forced_width_reaches_the_kernel_of_that_width(case, lib, rdf, gpu_runtime, evs, oracle):
    _run_case(case, lib, rdf, gpu_runtime, evs, oracle)


@pytest.mark.gpu
def test_counters_count_calls_that_launched(lib, rdf, gpu_runtime, oracle):
    """Two launches of one kernel count as 2, a reset clears, a call refused with RDF_ERR_BAD_ARG counts nothing."""
    synth = rdf.synth
    key = kc.Key(256, True, 4, True, 4, False, 1, False, False)
    at = KEYS.index(key)
    depth_np = kc.frames(synth)
    n, h, w = depth_np.shape
    depth = rdf.to_device(depth_np)
    labels = rdf.DeviceArray(depth_np.shape, np.uint16).fill(65535)
    st8 = rdf.DeviceArray((8,), np.uint64).fill(0)
    lib.rdf_set_block_threads(256)

    def call(classes):
        f = rdf.DecisionForest.from_numpy(kc.forest(synth, kc.ForestSpec(4, kc.DEPTH, classes, "trained")))
        return lib.rdf_eval_forest_packed_stats(depth.ptr, n, w, h, f.packed(1.0).ptr, f.forest_cu.ptr, 4, kc.DEPTH, classes, labels.ptr, 1,
                                                st8.ptr, gpu_runtime.stream())
    _counters(lib, reset=1)
    assert _counters(lib) == [0] * len(KEYS)
    assert call(4) == 0 and call(4) == 0
    want = [0] * len(KEYS)
    want[at] = 2
    assert _counters(lib) == want
    assert call(5) == -1                                        # RDF_ERR_BAD_ARG: the packed counting kernels keep four classes
    assert _counters(lib) == want
    assert _counters(lib, reset=1) == want                      # (a reset returns what it clears)
    assert _counters(lib) == [0] * len(KEYS)
    assert lib.rdf_debug_kernel_launches(None, 0, 1) == len(KEYS)
    labels.get()
