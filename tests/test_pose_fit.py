"""The pose fit (librdf_labels.so: rdf_pose_cost, rdf_pose_propose, rdf_pose_select, rdf_pose_fit; PoseFitter) against the
restatement in tests/pose_fit_numpy.py.  The CPU tests pin the restatement to answers worked by hand from rules C, P, K and S
in include/rdf_labels.h and to HandModel's own kinematics; every GPU comparison is bit for bit, with no case left out."""
import ctypes
import importlib
import os

import numpy as np
import pytest

import hand_scene_numpy as hs
import pose_fit_cases as pc
import pose_fit_numpy as pf
from abi_helpers import declared

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rdf_labels.h")
NEW_SYMBOLS = ("rdf_pose_cost", "rdf_pose_propose", "rdf_pose_select", "rdf_pose_fit_workspace_bytes", "rdf_pose_fit")


def _mods():
    return (importlib.import_module("3d-beats_amd.hand_model"), importlib.import_module("3d-beats_amd.hand_scene"),
            importlib.import_module("3d-beats_amd.pose_fit"))


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


# ------------------------------------------------------------------ CPU: rule C ---------------------------------------------
def test_rule_c_by_hand_on_a_4x3_frame():
    #            x = 0            1              2                3
    depth = np.array([[0, 1000, 1000, 1000],           # y = 0: missing data | hand, drawn | hand, not drawn | not hand, drawn
                      [1000, 1000, 1000, 1000],         # y = 1: not hand, not drawn | label 65535 | label 64 | hand, other label
                      [500, 0, 65535, 1]], np.uint16)   # y = 2: hand, deeper | missing data, hand | the two largest differences
    labels = np.array([[3, 3, 3, 0],
                       [0, 65535, 64, 2],
                       [1, 1, 1, 7]], np.uint16)
    cand_d = np.array([[[900, 990, 0, 700],
                        [0, 800, 800, 1010],
                        [520, 400, 1, 65535]]], np.uint16)
    cand_l = np.array([[[3, 3, 0, 1],
                        [0, 2, 2, 3],
                        [1, 1, 5, 7]]], np.uint16)
    t = pf.cost_terms(depth, labels, 1, (0, 0, 4, 3), cand_d, cand_l, 0xFE)
    # missing: (2, 0).  extra: (3, 0), and (1, 1), (2, 1) whose labels 65535 and 64 are no hand -- each once, as the
    # reference's second test falls through to a third that cannot hold.  label: (3, 1) (3 over 2) and (2, 2) (5 over 1).
    # sq: 10^2 at (1, 0), 10^2 at (3, 1), 20^2 at (0, 2), 65534^2 twice at (2, 2) and (3, 2); the d0 == 0 pixels (0, 0)
    # and (1, 2) are free although something is drawn over them.
    assert t.tolist() == [[1, 3, 2, 100 + 100 + 400 + 2 * 65534 ** 2]]
    assert 2 * 65534 ** 2 > 1 << 32
    assert pf.cost(t, 10000, 0) == [40000 + 600 + 2 * 65534 ** 2] and pf.cost(t, 10000, 7) == [40014 + 600 + 2 * 65534 ** 2]
    # one bit in the mask: only label 3 is hand, so (3, 1), (0, 2), (2, 2), (3, 2) become extra
    t3 = pf.cost_terms(depth, labels, 1, (0, 0, 4, 3), cand_d, cand_l, 1 << 3)
    assert t3.tolist() == [[1, 7, 0, 100]]
    # fit_mesh.cu: BOUNDARY_MISMATCH_COST = 100 per mismatch, 0.01 * diff * diff; the integer cost is 100 times that
    fit = _mods()[2]
    assert pf.reference_cost(t3[0]) == fit.reference_cost(t3[0]) == 100. * 8 + 0.01 * 100
    assert pf.cost(t3, 10000, 0)[0] == round(100 * fit.reference_cost(t3[0]))
    # a window: rendered pixel (i, j) sits over observed pixel (x0 + i, y0 + j)
    tw = pf.cost_terms(depth, labels, 1, (1, 0, 2, 2), cand_d[:, :2, 1:3], cand_l[:, :2, 1:3], 0xFE)
    assert tw.tolist() == [[1, 2, 0, 100]]


def test_rule_c_reads_a_reduced_label_map_with_its_last_row_and_column_repeated():
    # 5 x 3 depth pixels, r = 2: labels [1][2]; depth column 4 reads label column min(4 // 2, 1) = 1, row 2 reads row 0
    got = pf.observed_labels(np.array([[4, 9]], np.uint16), 5, 3, 2)
    assert got.tolist() == [[4, 4, 9, 9, 9]] * 3
    depth = np.full((3, 5), 100, np.uint16)
    cand = np.zeros((1, 3, 5), np.uint16)
    cand[0, 2, 4] = cand[0, 0, 0] = 90
    # mask = label 9 only: (4, 2) is hand and drawn, (0, 0) is extra, the other eight label-9 pixels are missing
    t = pf.cost_terms(depth, np.array([[4, 9]], np.uint16), 2, (0, 0, 5, 3), cand, np.full((1, 3, 5), 9, np.uint16), 1 << 9)
    assert t.tolist() == [[8, 1, 0, 100]]


def test_the_gpu_cost_cases_reach_every_branch():
    for W, H in pc.COST_FRAMES:
        for r in (1, 2):
            c = pc.cost_case(W, H, r)
            assert W % 2 == 1 or H % 2 == 0 and (W // r) * r <= W       # (33 x 17 is odd in both)
            assert len(c["runs"]) == len(pc.cost_windows(W, H)) * len(pc.COST_K)
            whole = [run for run in c["runs"] if run["window"] == (0, 0, W, H) and run["K"] == 65][0]
            assert (whole["terms"] > 0).all() and (whole["terms"][:, 3] > 1 << 32).all()
            assert {run["window"][2] for run in c["runs"]} >= {1, 7, 8, 33}
            assert any(run["window"][0] % 2 == 1 for run in c["runs"])
    assert 200 * 70 // 8 > 256          # more than one workgroup's groups per candidate


def _cost_plan(n_px, K):
    """The three plan lines of launch_cost: (sets, chunk, workgroups per candidate)."""
    sets = (n_px // 8 + 255) // 256
    chunk = min(max(sets * K // 1024, 1), 16)
    return sets, chunk, (sets + chunk - 1) // chunk if sets else 1


def _groups(n_px, offset, k):
    """The full groups of eight of candidate k, whose image starts offset + k * n_px elements into a 16-byte aligned array."""
    head = min(((16 - 2 * (offset + k * n_px) % 16) % 16) // 2, n_px)
    return (n_px - head) // 8


def test_the_chunked_cost_cases_make_the_trips_they_claim():
    for name, ((W, H), window, K, rs, offsets, plan) in pc.CHUNK_CASES.items():
        x0, y0, ww, wh = window
        n_px = ww * wh
        sets, chunk, gx = _cost_plan(n_px, K)
        assert (sets, chunk, gx) == plan and 1 < chunk < 16, name
        assert x0 + ww <= W and y0 + wh <= H and 2e6 < K * n_px < 6e6, name
        assert offsets[0] % 2 == 1 and offsets[1] % 2 == 1 and offsets[0] != offsets[1], name
        # the odd offset moves at most one group from the full groups to the head
        groups = {_groups(n_px, offsets[0], k) for k in range(K)}
        assert groups <= {n_px // 8 - 1, n_px // 8} and n_px // 8 - 1 in groups, name
        last = [[min(max(g - ((gx - 1) * chunk + trip) * 256, 0), 256) for trip in range(chunk)] for g in sorted(groups)]
        if name == "the benchmarked plan":
            assert K == 64 and (ww, wh) == (256, 256) and rs == (1, 2)          # what profiles/pose_fit_bench.json measures
            assert all(trips[0] == 256 and 192 < trips[1] <= 256 for trips in last), last   # every workgroup's second trip works
        elif name == "sets no multiple of chunk":
            assert sets % chunk and all(trips[0] == 256 and 64 < trips[1] < 128 and trips[2] == 0 for trips in last), last
            assert (offsets[1] - offsets[0]) % 8 == 0                           # the labels are loaded as vectors
        else:
            assert K == pc.MAX_CANDIDATES and all(0 < trips[0] < 256 and trips[1:] == [0, 0, 0] for trips in last), last
            assert len({(16 - 2 * (offsets[0] + k * n_px) % 16) % 16 for k in range(K)}) == 8       # every head length
        for r in rs:
            c = pc.chunk_cost_case(name, r)
            assert c["terms"].shape == (K, 4) and (c["terms"] > 0).all() and (c["base"] > 0).all(), (name, r)
            assert c["depth"].shape == (H, W) and c["labels"].shape == (H // r, W // r)
    # the chunk is the same whichever way the sets are counted; cost_case never reaches a second trip
    assert all(_cost_plan(w[2] * w[3], K)[1] == 1 for W, H in pc.COST_FRAMES for w in pc.cost_windows(W, H) for K in pc.COST_K)
    assert _cost_plan(96 * 72, 16)[1] == 1 and _cost_plan(95 * 71, pc.K_ODD)[1] == 1


# ------------------------------------------------------------------ CPU: rule P ---------------------------------------------
def test_rule_p_draws_are_exact_and_centred():
    n = np.array([pf.draw(pf.candidate_hash(11, g, k), j) for g in range(20) for k in range(25) for j in range(20)])
    assert len(n) == 10 ** 4 and n.dtype == np.float64
    assert (np.abs(n) < 2.).all() and np.array_equal(n * 65536., np.rint(n * 65536.))        # multiples of 2^-16
    assert abs(n.mean()) < 0.03 and 0.5 < n.std() < 0.65             # four uniform 16-bit halves: sigma = sqrt(1 / 3)
    assert pf.mix1(0) == 0 and pf.mix1(1) == 0x688990C0
    h = pf.candidate_hash(5, 2, 3)
    assert h == pf.mix1(pf.mix1(5 + 2 * 0x9E3779B9) ^ 3)


def test_rule_p_moves_one_group_clamps_and_anneals():
    hm, _, fit = _mods()
    model = hm.HandModel()
    inc = pc.true_pose(model)
    sigma = fit.pose_vector(fit.DEFAULT_SIGMA, 10.)
    assert sigma[:6].tolist() == [80., 80., 80., 0.08, 0.08, 0.08] and sigma[6:10].tolist() == [0.05, 0.12, 0.12, 0.12]
    lo, hi = fit.pose_ranges(None, 10.)
    K = 64
    poses = pf.propose(inc, 9, 0, K, sigma, lo, hi, 8)
    groups = set()
    for k in range(K):
        h = pf.candidate_hash(9, 0, k)
        moved = set(pf.GROUPS[h & 7])
        groups.add(h & 7)
        others = [j for j in range(26) if j not in moved]
        assert np.array_equal(_bits(poses[k, others]), _bits(inc[others])), k          # copied, bit for bit
        for j in moved:
            assert poses[k, j] == inc[j] + (sigma[j] * 1.) * pf.draw(h, j)
    assert groups == set(range(8))
    assert pf.GROUPS[0] == (0, 1, 2) and pf.GROUPS[1] == (3, 4, 5) and pf.GROUPS[2] == (6, 7, 8, 9) and pf.GROUPS[6] == (22, 23, 24, 25)
    assert pf.GROUPS[7] == tuple(range(26))
    # clamping at both ends: a range narrower than the draws
    tight_lo, tight_hi = inc - 0.25 * sigma, inc + 0.25 * sigma
    tight = pf.propose(inc, 9, 0, K, sigma, tight_lo, tight_hi, 8)
    assert (tight >= tight_lo).all() and (tight <= tight_hi).all()
    assert (tight == tight_lo).any() and (tight == tight_hi).any() and ((tight > tight_lo) & (tight < tight_hi) & (tight != inc)).any()
    # the first generation of a fresh fit: generation 0 whatever g says, candidate 0 the incumbent itself -- even outside
    # the ranges
    outside = inc.copy()
    outside[0] = hi[0] + 5.
    fresh = pf.propose(outside, 9, 77, K, sigma, lo, hi, 8, fresh_first=True)
    assert np.array_equal(_bits(fresh[0]), _bits(outside))
    assert np.array_equal(fresh[1:, 1:], poses[1:, 1:])
    # the scale halves at the anneal_every boundary, and not before
    assert [float(pf.scale_of(g, 8)) for g in (0, 7, 8, 15, 16, 24)] == [1., 1., 0.5, 0.5, 0.25, 0.125]
    assert pf.scale_of(3, 1) == 0.125 and pf.scale_of(10 ** 6, 1) == 2. ** -1022
    for g, scale in ((7, 1.), (8, 0.5)):
        p = pf.propose(inc, 9, g, 8, sigma, lo, hi, 8)
        for k in range(8):
            h = pf.candidate_hash(9, g, k)
            for j in pf.GROUPS[h & 7]:
                assert p[k, j] == inc[j] + (sigma[j] * scale) * pf.draw(h, j)


# ------------------------------------------------------------------ CPU: rule K ---------------------------------------------
def test_rule_k_is_within_one_fp32_ulp_of_the_hand_models_own_transforms():
    """The two fp64 chains differ by about 1e-12 relative (different association, another sine), far below half an fp32
    ulp: after the cast an entry can differ only where its value straddles a rounding boundary, by one ulp."""
    hm, scene, _ = _mods()
    plane = scene.look_down_plane(5500., 0.15)
    cam = np.linalg.inv(plane)
    worst, differing, total = 0., 0, 0
    for mirrored in (False, True):
        model = hm.HandModel(mirrored=mirrored)
        poses = model.sample_poses(100, np.random.default_rng(21 + mirrored), {"yaw": (-3.1, 3.1), "flexion": (-0.3, 1.8)})
        got = pf.part_tforms(poses, cam[:3].reshape(12), pf.geometry_of(model), mirrored)
        want = model.part_transforms(poses, cam)
        assert got.dtype == np.float32 and got.shape == want.shape == (100, 16, 12)
        ulp = np.spacing(np.maximum(np.abs(got), np.abs(want)))
        err = np.abs(got.astype(np.float64) - want.astype(np.float64)) / ulp
        worst, differing, total = max(worst, float(err.max())), differing + int((got != want).sum()), total + got.size
    print(f"rule K against HandModel.part_transforms: {differing} of {total} entries differ, by at most {worst} ulp")
    assert worst <= 1.
    # the restated sine and cosine against numpy's, on a grid over [-pi, pi] (recorded in DESIGN.md, not asserted: the
    # assertion is the one-ulp bound above)
    x = np.linspace(-np.pi, np.pi, 20001)
    sc = np.array([pf.sincos(v) for v in x])
    print(f"sincos on 20001 points of [-pi, pi]: max |sin - np.sin| = {np.abs(sc[:, 0] - np.sin(x)).max():.3e}, "
          f"max |cos - np.cos| = {np.abs(sc[:, 1] - np.cos(x)).max():.3e}")
    assert np.isnan(pf.sincos(2. ** 21)).all() and np.isnan(pf.sincos(np.nan)).all()


def test_rule_k_mirror_negates_five_entries_of_the_chain():
    hm, scene, _ = _mods()
    model = hm.HandModel()
    pose = pc.true_pose(model)
    pose[[0, 3, 5]] = 0.            # a pose that is its own mirror image, under a camera that is too
    cam = np.linalg.inv(scene.look_down_plane(5500., 0.))[:3].reshape(12)
    right = pf.part_tforms(pose[None], cam, pf.geometry_of(model), False)[0].reshape(16, 3, 4)
    left = pf.part_tforms(pose[None], cam, pf.geometry_of(model), True)[0].reshape(16, 3, 4)
    sign = np.array([[1, -1, -1, -1], [-1, 1, 1, 1], [-1, 1, 1, 1]], np.float32)
    assert np.array_equal(left, right * sign)


# ------------------------------------------------------------------ CPU: rule S ---------------------------------------------
def test_rule_s_ties_strictness_and_the_fresh_acceptance():
    want = {"the lowest cost wins": (1, True), "of equal costs the lowest k": (0, True), "equal to the incumbent is not better": (None, False),
            "one below the incumbent is": (1, True), "nothing better: only g moves": (None, False),
            "a fresh first generation takes the best although it is worse": (1, True), "one candidate": (0, True),
            "130 candidates, a tie across the wave": (6, True), "costs beyond 2^63": (1, True),
            "4096 candidates, the minimum three times": (61, True), "4096 candidates, all equal": (0, True)}
    cases = pc.select_cases()
    assert {c[0] for c in cases} == set(want)
    for name, K, terms, before, wb, wl, fresh in cases:
        state = {k: (v.copy() if hasattr(v, "copy") else v) for k, v in before.items()}
        poses = pc.select_poses(K)
        costs = pf.cost(terms, wb, wl)
        entry = pf.select(state, poses, terms, wb, wl, fresh)
        best, replaced = want[name]
        if replaced:
            assert np.array_equal(state["pose"], poses[best]) and state["cost"] == costs[best] == min(costs), name
            assert np.array_equal(state["terms"], terms[best]) and costs.index(min(costs)) == best, name
        else:
            assert np.array_equal(state["pose"], before["pose"]) and state["cost"] == before["cost"], name
            assert np.array_equal(state["terms"], before["terms"]) and min(costs) >= before["cost"], name
        assert entry == state["cost"], name
        if fresh:
            assert (state["g"], state["accepted"]) == (1, 1) and min(costs) > before["cost"], name
        else:
            assert (state["g"], state["accepted"]) == (before["g"] + 1, before["accepted"] + int(replaced)), name
    assert pf.cost(np.array([[2 ** 31 - 1, 2 ** 31 - 1, 0, 2 ** 62]], np.uint64), 2 ** 32 - 1, 0)[0] < 2 ** 63     # it wrapped
    # the cases at RDF_POSE_MAX_CANDIDATES: a lane of k_pose_select takes k = lane, lane + 64, ...
    by_name = {c[0]: c for c in cases}
    _, K, terms, _, wb, wl, _ = by_name["4096 candidates, the minimum three times"]
    costs = pf.cost(terms, wb, wl)
    at = [k for k in range(K) if costs[k] == min(costs)]
    assert K == pc.MAX_CANDIDATES == 64 * 64 and at == [61, 4032, 4095] and [k % 64 for k in at] == [61, 0, 63]
    _, K, terms, _, wb, wl, _ = by_name["4096 candidates, all equal"]
    assert K == pc.MAX_CANDIDATES and len(set(pf.cost(terms, wb, wl))) == 1


# ------------------------------------------------------------------ CPU: the whole fit --------------------------------------
def test_a_fit_from_the_true_pose_costs_nothing_and_never_moves():
    c, ref = pc.self_fit_case(), pc.self_fit_reference()
    assert c["cfg"]["w_label"] > 0 and ((c["labels"] > 0).sum()) > 400
    assert ref["history"] == [0] * pc.G_SELF
    assert ref["state"]["accepted"] == 1 and ref["state"]["g"] == pc.G_SELF        # the fresh acceptance, and no other
    assert np.array_equal(_bits(ref["state"]["pose"]), _bits(c["pose"])) and not ref["state"]["terms"].any()


def test_a_fit_from_an_offset_start_only_ever_gets_cheaper():
    c, ref = pc.fit_case(), pc.fit_reference()
    assert c["cfg"]["window"] == (13, 9, 96, 72) and c["depth"].shape == (90, 120) and c["cfg"]["K"] == 16
    hand = c["labels"] > 0
    x0, y0, ww, wh = c["cfg"]["window"]
    assert 400 < hand.sum() == hand[y0:y0 + wh, x0:x0 + ww].sum() and (c["depth"] > 0).all()       # the table is behind the hand
    h = ref["history"]
    print(f"restated fit, {int(hand.sum())} hand pixels: history {h}, accepted {ref['state']['accepted']}")
    assert len(h) == pc.G_FIT == 8 and all(b <= a for a, b in zip(h, h[1:]))
    # the start's own cost: candidate 0 of the fresh first generation
    t = pf.part_tforms(c["start"][None], c["cfg"]["cam_from_plane"], c["cfg"]["geometry"], False)
    F = np.float32
    cd, cl, _ = hs.render(ww, wh, *c["mesh"], t, None, F(c["cfg"]["f"]), F(c["cfg"]["ppx"]) - F(x0), F(c["cfg"]["ppy"]) - F(y0), empty_depth=0)
    initial = pf.cost(pf.cost_terms(c["depth"], c["labels"], 1, c["cfg"]["window"], cd, cl, 0xFE), 10000, 0)[0]
    assert h[0] <= initial and h[-1] < initial
    assert ref["state"]["accepted"] >= 1 and ref["state"]["g"] == 8 and ref["state"]["cost"] == h[-1]
    assert ref["after3"]["g"] == 3 and ref["after3"]["cost"] == h[2]
    assert (ref["state"]["pose"] >= c["cfg"]["lo"]).all() and (ref["state"]["pose"] <= c["cfg"]["hi"]).all()


def test_the_odd_window_fit_gives_every_candidate_another_head():
    c, ref = pc.odd_fit_case(), pc.odd_fit_reference()
    x0, y0, ww, wh = c["cfg"]["window"]
    assert (x0, y0, ww, wh) == (13, 9, 95, 71) and c["cfg"]["K"] == 5 and ww * wh == 6745 and x0 + ww <= pc.FRAME_W and y0 + wh <= pc.FRAME_H
    # candidate k's images start k * 6745 * 2 bytes into a 256-byte aligned region: the pixels in front of the first 16-byte
    # boundary are 0, 7, 6, 5 and 4; under the 96 x 72 window every candidate starts on a boundary
    heads = [((16 - (k * ww * wh * 2) % 16) % 16) // 2 for k in range(5)]
    assert heads == [0, 7, 6, 5, 4] and all((k * 96 * 72 * 2) % 16 == 0 for k in range(pc.K_FIT))
    hand = c["labels"] > 0
    assert 400 < hand.sum() == hand[y0:y0 + wh, x0:x0 + ww].sum()
    h = ref["history"]
    print(f"restated fit on the odd window: history {h}, accepted {ref['state']['accepted']}")
    assert len(h) == pc.G_ODD == 2 and h[1] <= h[0] and h[1] > 0 and ref["state"]["g"] == 2 and ref["state"]["accepted"] >= 1
    assert ref["state"]["terms"][3] > 0 and ref["state"]["cost"] == h[1]


# ------------------------------------------------------------------ CPU: the interface --------------------------------------
def _config_struct(cfg, **over):
    fit = _mods()[2]
    s = fit._Config()
    s.candidates, s.mirrored, s.anneal_every, s.seed = cfg["K"], int(cfg["mirrored"]), cfg["anneal_every"], cfg["seed"]
    s.x0, s.y0, s.ww, s.wh = cfg["window"]
    s.w_boundary, s.w_label, s.target_mask = cfg["w_boundary"], cfg["w_label"], cfg["target_mask"]
    s.f, s.ppx, s.ppy, s.zmin, s.zmax = float(cfg["f"]), float(cfg["ppx"]), float(cfg["ppy"]), cfg["zmin"], cfg["zmax"]
    for name in ("sigma", "lo", "hi", "cam_from_plane", "geometry"):
        getattr(s, name)[:] = [float(v) for v in cfg[name]]
    for k, v in over.items():
        if isinstance(v, tuple):
            getattr(s, k)[v[0]] = v[1]
        else:
            setattr(s, k, v)
    return s


def test_the_new_entry_points_reject_bad_and_null_arguments(rdf):
    _lib = importlib.import_module("3d-beats_amd._lib")
    importlib.import_module("3d-beats_amd._build").build()
    names = declared(HEADER)
    for must in NEW_SYMBOLS:
        assert must in names and must in _lib.BINDINGS["labels"][1]
    lib = _lib.load("labels")
    assert lib.rdf_labels_abi_version() == 1            # a pure addition
    text = open(HEADER).read()
    for rule in ("\n * C. The cost", "\n * P. Proposals", "\n * K. Kinematics", "\n * S. Selection"):
        assert rule in text
    ws = lib.rdf_pose_fit_workspace_bytes
    keys = lib.rdf_hand_scene_workspace_bytes(64, 256, 256)
    assert ws(64, 256, 256) >= keys + 64 * (256 * 256 * 4 + 16 * 48 + 26 * 8 + 32) and ws(64, 256, 256) % 256 == 0
    assert ws(0, 8, 8) == 0 and ws(4097, 8, 8) == 0 and ws(4, 0, 8) == 0 and ws(4, 8, 40000) == 0 and ws(1, 1, 1) > 0

    # rejected arguments launch nothing, so they can be checked without a device
    def cost(W=33, H=17, r=1, window=(1, 2, 8, 4), K=3, p=(64, 128, 256, 512, 1024)):
        return lib.rdf_pose_cost(W, H, p[0], p[1], r, *window, K, p[2], p[3], 0xFE, p[4], None)
    assert cost(K=0) == -1 and cost(K=4097) == -1 and cost(r=0) == -1 and cost(W=-1) == -1
    assert cost(window=(26, 2, 8, 4)) == -1 and cost(window=(1, 14, 8, 4)) == -1 and cost(window=(-1, 2, 8, 4)) == -1
    assert cost(window=(1, 2, 0, 4)) == -1 and cost(window=(1, 2, 8, 0)) == -1 and cost(W=3, H=3, r=4, window=(0, 0, 1, 1)) == -1
    assert cost(p=(None, 128, 256, 512, 1024)) == -2 and cost(p=(64, 128, 256, 512, None)) == -2
    assert cost(W=40000, H=17) == -3
    assert cost(p=(65, 128, 256, 512, 1024)) == -1 and cost(p=(64, 128, 256, 512, 1028)) == -1        # misaligned

    cfg = pc.fit_case()["cfg"]

    def propose(s, p=(256, 512, 1024, 2048)):
        return lib.rdf_pose_propose(ctypes.addressof(s) if s is not None else None, p[0], 0, p[1], p[2], p[3], None)
    assert propose(None) == -2 and propose(_config_struct(cfg), p=(None, 512, 1024, 2048)) == -2
    assert propose(_config_struct(cfg), p=(256, 516, 1024, 2048)) == -1
    pi = float(np.pi)
    for over in ({"candidates": 0}, {"candidates": 4097}, {"anneal_every": 0}, {"sigma": (4, -1.)}, {"sigma": (4, float("nan"))},
                 {"lo": (2, float("-inf"))}, {"lo": (7, 2.)}, {"hi": (3, np.nextafter(pi, 4.))}, {"lo": (25, -np.nextafter(pi, 4.))},
                 {"cam_from_plane": (5, float("inf"))}, {"geometry": (29, float("nan"))}):
        assert propose(_config_struct(cfg, **over)) == -1, over
    # a wrist range is a length: it may exceed pi; an angle's range may reach pi exactly
    assert propose(_config_struct(cfg, hi=(3, pi), lo=(3, -pi)), p=(None, 512, 1024, 2048)) == -2

    def select(K=4, p=(64, 128, 256, None)):
        return lib.rdf_pose_select(K, p[0], p[1], 10000, 0, 0, p[2], p[3], None)
    assert select(K=0) == -1 and select(K=4097) == -1 and select(p=(None, 128, 256, None)) == -2 and select(p=(64, 128, None, None)) == -2
    assert select(p=(68, 128, 256, None)) == -1 and select(p=(64, 128, 256, 44)) == -1

    def fit(s, G=1, W=120, H=90, r=1, p=(256, 512, 1024, 4096), mesh=2048, n_tris=1):
        m = [mesh] * 4
        return lib.rdf_pose_fit(G, 1, ctypes.addressof(s) if s is not None else None, p[0], W, H, p[1], p[2], r, 3, m[0], m[1],
                                n_tris, m[2], m[3], p[3], None, None)
    good = _config_struct(cfg)
    assert fit(None) == -2 and fit(good, G=-1) == -1 and fit(good, W=100) == -1 and fit(good, H=80) == -1 and fit(good, r=0) == -1
    assert fit(_config_struct(cfg, x0=-1)) == -1 and fit(_config_struct(cfg, ww=0)) == -1 and fit(_config_struct(cfg, f=0.)) == -1
    assert fit(_config_struct(cfg, zmin=0.)) == -1 and fit(_config_struct(cfg, zmax=40.)) == -1 and fit(_config_struct(cfg, hi=(4, 4.))) == -1
    assert fit(good, G=0, p=(None, None, None, None)) == 0                  # no generations: nothing to do
    assert fit(good, p=(None, 512, 1024, 4096)) == -2 and fit(good, p=(256, 512, 1024, None)) == -2 and fit(good, mesh=None) == -2
    assert fit(good, p=(260, 512, 1024, 4096)) == -1 and fit(good, p=(256, 512, 1024, 4104)) == -1
    assert fit(good, W=40000, H=90) == -3


def test_pose_fitter_checks_its_arguments_on_the_host(rdf):
    hm, scene, fit = _mods()
    plane = scene.look_down_plane(5500., 0.1)
    ok = dict(depth_dims=(90, 120), intrinsics=pc.CAM, plane=plane)
    f = rdf.PoseFitter(**ok)
    assert f.window == (0, 0, 120, 90) and f.candidates == 64 and f.target_mask == 0xFE and f.w_boundary == 10000 and f.w_label == 0
    assert f.anneal_every == 8 and not f.model.is_mirrored and rdf.PoseFitter(mirrored=True, **ok).model.is_mirrored
    assert "PoseFitter" in rdf.__all__ and "unmeasured on real data" in rdf.PoseFitter.__init__.__doc__
    assert f.workspace_bytes() == f._lb.rdf_pose_fit_workspace_bytes(64, 120, 90)
    import inspect
    p = inspect.signature(rdf.PoseFitter.__init__).parameters
    assert list(p)[1:] == ["depth_dims", "intrinsics", "plane", "model", "mirrored", "candidates", "window", "labels", "target_labels",
                           "labels_reduce", "w_boundary", "w_label", "sigma", "ranges", "anneal_every", "seed"]
    # the config the C call reads is the one the restatement is given
    c = pc.fit_case()
    g = rdf.PoseFitter((90, 120), pc.CAM, c["plane"], candidates=16, window=pc.WINDOW, seed=pc.SEED)
    for name in ("sigma", "lo", "hi", "cam_from_plane", "geometry"):
        assert np.array_equal(np.array(getattr(g._cfg, name)[:]), c["cfg"][name]), name
    assert (g._cfg.x0, g._cfg.y0, g._cfg.ww, g._cfg.wh) == pc.WINDOW and g._cfg.seed == pc.SEED and g._cfg.candidates == 16
    assert np.array_equal(g.tri_label, c["mesh"][3])
    assert (np.abs(g.lo[3:]) <= np.pi).all() and (np.abs(g.hi[3:]) <= np.pi).all()
    for bad in (dict(candidates=0), dict(candidates=5000), dict(window=(100, 0, 30, 10)), dict(window=(0, 0, 0, 10)),
                dict(labels_reduce=0), dict(labels_reduce=100), dict(target_labels=[64]), dict(target_labels=[]), dict(w_boundary=-1),
                dict(w_label=1 << 32), dict(anneal_every=0), dict(sigma=np.ones(25)), dict(sigma=-np.ones(26)),
                dict(ranges={"yaw": (-4., 4.)}), dict(ranges={"flexion": (1., 0.)}), dict(ranges={"thumb": (0., 1.)}),
                dict(labels=np.zeros(5, np.uint16)), dict(intrinsics=(0., 1., 1.)), dict(plane=np.zeros((4, 4))), dict(depth_dims=(0, 10))):
        with pytest.raises((ValueError, np.linalg.LinAlgError)):
            rdf.PoseFitter(**{**ok, **bad})
    # what fit checks before it touches the device
    depth, labels = np.zeros((90, 120), np.uint16), np.zeros((90, 120), np.uint16)
    for args, kwargs in (((depth, labels), {}), ((depth, labels, np.zeros(25)), {}), ((depth, labels, np.full(26, np.nan)), {}),
                         ((depth, labels, np.zeros(26)), {"fresh": False}), ((depth, labels, np.zeros(26)), {"generations": -1})):
        with pytest.raises(ValueError):
            f.fit(*args, **kwargs)
    with pytest.raises(ValueError):
        f.track([depth], [labels, labels], np.zeros(26), 2)
    # window_around: the hand's window holds the hand, and is clipped to the frame
    win = f.window_around(c["true"], margin_mm=10.)
    hand = np.argwhere(c["labels"] > 0)
    assert win[0] <= hand[:, 1].min() and hand[:, 1].max() < win[0] + win[2] and win[1] <= hand[:, 0].min() and hand[:, 0].max() < win[1] + win[3]
    assert 0 <= win[0] and win[0] + win[2] <= 120 and 0 <= win[1] and win[1] + win[3] <= 90
    big = rdf.PoseFitter((480, 848), (600., 423.5, 239.5), plane)
    w = big.window_around(c["true"])
    assert w[2] < 848 and w[3] <= 480 and big.set_window(w) == w and big.workspace_bytes() < rdf.PoseFitter((480, 848), (600., 423.5, 239.5), plane).workspace_bytes()
    assert fit.reference_cost([1, 2, 5, 300]) == 303.


# ------------------------------------------------------------------ GPU -----------------------------------------------------
def _labels_lib():
    _lib = importlib.import_module("3d-beats_amd._lib")
    return _lib, _lib.load("labels")


@pytest.mark.gpu
@pytest.mark.parametrize("r", [1, 2])
@pytest.mark.parametrize("W,H", pc.COST_FRAMES)
def test_rdf_pose_cost_matches_the_restatement_bit_for_bit(W, H, r, rdf, gpu_runtime):
    _lib, lib = _labels_lib()
    c = pc.cost_case(W, H, r)
    depth, labels = rdf.to_device(c["depth"]), rdf.to_device(c["labels"])
    for run in c["runs"]:
        K, window = run["K"], run["window"]
        n = K * window[2] * window[3]
        # the candidates at an odd element offset: their 16-byte boundary is wherever it falls
        cd, cl = rdf.DeviceArray((n + 9,), np.uint16), rdf.DeviceArray((n + 9,), np.uint16)
        off = 1 + 2 * (K % 3)
        cd[off:off + n].set(run["cand_depth"].reshape(-1))
        cl[1:1 + n].set(run["cand_labels"].reshape(-1))
        terms = rdf.to_device(run["base"])
        rc = lib.rdf_pose_cost(W, H, depth.ptr, labels.ptr, r, *window, K, cd.ptr + 2 * off, cl.ptr + 2, pc.COST_MASK, terms.ptr,
                               gpu_runtime.stream())
        _lib.check(lib, rc, "rdf_pose_cost")
        got = terms.get()
        want = run["base"] + run["terms"]           # the call adds to what was there
        bad = int((got != want).sum())
        if bad:
            print(f"{W}x{H} r={r} window {window} K={K}: {bad} of {want.size} terms differ; first candidate got "
                  f"{(got[0] - run['base'][0]).tolist()} want {run['terms'][0].tolist()}")
        assert np.array_equal(got, want), (window, K)
        # rejected arguments leave the terms untouched
        for bad_args in ((W, H, depth.ptr, labels.ptr, 0, *window, K), (W, H, depth.ptr, labels.ptr, r, W - 1, 0, 2, 1, K),
                         (W, H, depth.ptr, labels.ptr, r, *window, 0), (W, H, depth.ptr + 1, labels.ptr, r, *window, K)):
            assert lib.rdf_pose_cost(*bad_args, cd.ptr + 2 * off, cl.ptr + 2, pc.COST_MASK, terms.ptr, gpu_runtime.stream()) == -1
        assert np.array_equal(terms.get(), want)


@pytest.mark.gpu
@pytest.mark.parametrize("name,r", [(name, r) for name, case in pc.CHUNK_CASES.items() for r in case[3]])
def test_rdf_pose_cost_over_several_trips_matches_the_restatement_bit_for_bit(name, r, rdf, gpu_runtime):
    _lib, lib = _labels_lib()
    (W, H), window, K, _, (off_d, off_l), plan = pc.CHUNK_CASES[name]
    c = pc.chunk_cost_case(name, r)
    depth, labels = rdf.to_device(c["depth"]), rdf.to_device(c["labels"])
    n = K * window[2] * window[3]
    cd, cl = rdf.DeviceArray((n + 16,), np.uint16), rdf.DeviceArray((n + 16,), np.uint16)
    cd[off_d:off_d + n].set(c["cand_depth"].reshape(-1))
    cl[off_l:off_l + n].set(c["cand_labels"].reshape(-1))
    assert cd.ptr % 16 == 0 and cl.ptr % 16 == 0            # what the CPU test's head lengths assume
    terms = rdf.to_device(c["base"])
    rc = lib.rdf_pose_cost(W, H, depth.ptr, labels.ptr, r, *window, K, cd.ptr + 2 * off_d, cl.ptr + 2 * off_l, pc.COST_MASK, terms.ptr,
                           gpu_runtime.stream())
    _lib.check(lib, rc, "rdf_pose_cost")
    got = terms.get()
    want = c["base"] + c["terms"]
    bad = int((got != want).sum())
    print(f"{name} r={r}: plan (sets, chunk, workgroups) {plan}: {bad} of {want.size} terms differ; first candidate got "
          f"{(got[0] - c['base'][0]).tolist()} want {c['terms'][0].tolist()}")
    assert np.array_equal(got, want)


def _state_bytes(state):
    raw = np.zeros(256, np.uint8)
    raw[:208] = np.asarray(state["pose"], np.float64).view(np.uint8)
    raw[208:216] = np.array([state["cost"]], np.uint64).view(np.uint8)
    raw[216:248] = np.asarray(state["terms"], np.uint64).view(np.uint8)
    raw[248:256] = np.array([state["g"], state["accepted"]], np.uint32).view(np.uint8)
    return raw


@pytest.mark.gpu
@pytest.mark.parametrize("mirrored", [False, True])
@pytest.mark.parametrize("K", [1, 8, 65])
def test_rdf_pose_propose_matches_the_restatement_bit_for_bit(K, mirrored, rdf, gpu_runtime):
    _lib, lib = _labels_lib()
    for g, fresh in ((7, False), (8, False), (23, True)):       # either side of an annealing boundary, and a fresh start
        c = pc.propose_case(K, mirrored, g, fresh)
        state = pf.new_state(c["inc"])
        state.update(g=g, cost=123, accepted=2)
        before = _state_bytes(state)
        state_cu = rdf.to_device(before)
        poses, tforms = rdf.DeviceArray((K, 26), np.float64).fill(0), rdf.DeviceArray((K, 16, 12), np.float32).fill(0)
        terms = rdf.to_device(np.full((K, 4), 77, np.uint64))
        s = _config_struct(c["cfg"])
        rc = lib.rdf_pose_propose(ctypes.addressof(s), state_cu.ptr, int(fresh), poses.ptr, tforms.ptr, terms.ptr, gpu_runtime.stream())
        _lib.check(lib, rc, "rdf_pose_propose")
        got_p, got_t = poses.get(), tforms.get()
        print(f"K={K} mirrored={mirrored} g={g} fresh={fresh}: {int((_bits(got_p) != _bits(c['poses'])).sum())} pose numbers and "
              f"{int((_bits(got_t) != _bits(c['tforms'])).sum())} transform entries differ")
        assert np.array_equal(_bits(got_p), _bits(c["poses"])) and np.array_equal(_bits(got_t), _bits(c["tforms"]))
        assert not terms.get().any() and np.array_equal(state_cu.get(), before)
        assert (c["poses"] == c["cfg"]["lo"]).any() or (c["poses"] == c["cfg"]["hi"]).any() or K == 1
        # a range outside [-pi, pi] is refused, and nothing is written
        poses.fill(0)
        wide = _config_struct(c["cfg"], hi=(3, 3.2))
        assert lib.rdf_pose_propose(ctypes.addressof(wide), state_cu.ptr, int(fresh), poses.ptr, tforms.ptr, terms.ptr,
                                    gpu_runtime.stream()) == -1
        assert not poses.get().any()


@pytest.mark.gpu
def test_rdf_pose_select_matches_the_restatement(rdf, gpu_runtime):
    _lib, lib = _labels_lib()
    for name, K, terms, before, wb, wl, fresh in pc.select_cases():
        want = {k: (v.copy() if hasattr(v, "copy") else v) for k, v in before.items()}
        poses = pc.select_poses(K)
        entry = pf.select(want, poses, terms, wb, wl, fresh)
        state_cu, slot = rdf.to_device(_state_bytes(before)), rdf.to_device(np.array([5], np.uint64))
        terms_cu, poses_cu = rdf.to_device(terms), rdf.to_device(poses)
        rc = lib.rdf_pose_select(K, terms_cu.ptr, poses_cu.ptr, wb, wl, int(fresh), state_cu.ptr, slot.ptr, gpu_runtime.stream())
        _lib.check(lib, rc, "rdf_pose_select")
        assert np.array_equal(state_cu.get(), _state_bytes(want)), name
        assert int(slot.get()[0]) == entry, name
        # no history asked for
        again = rdf.to_device(_state_bytes(before))
        _lib.check(lib, lib.rdf_pose_select(K, terms_cu.ptr, poses_cu.ptr, wb, wl, int(fresh), again.ptr, None, gpu_runtime.stream()),
                   "rdf_pose_select")
        assert np.array_equal(again.get(), _state_bytes(want)), name


def _assert_state(result, want, history):
    r = result.get()
    assert np.array_equal(_bits(r.pose), _bits(want["pose"])) and r.cost == want["cost"] and np.array_equal(r.terms, want["terms"])
    assert r.generation == want["g"] and r.accepted == want["accepted"] and r.history.tolist() == list(history)


@pytest.mark.gpu
def test_rdf_pose_fit_matches_the_restated_fit(rdf, gpu_runtime):
    c, ref = pc.fit_case(), pc.fit_reference()
    depth, labels = rdf.to_device(c["depth"]), rdf.to_device(c["labels"])

    def fitter():
        return rdf.PoseFitter((pc.FRAME_H, pc.FRAME_W), pc.CAM, c["plane"], candidates=pc.K_FIT, window=pc.WINDOW, seed=pc.SEED)
    one = fitter()
    whole = one.fit(depth, labels, c["start"], generations=pc.G_FIT).get()
    print(f"device fit: history {whole.history.tolist()}, accepted {whole.accepted}; restated {ref['history']}, {ref['state']['accepted']}")
    _assert_state(whole, ref["state"], ref["history"])
    keys = one._lb.rdf_hand_scene_workspace_bytes(pc.K_FIT, pc.WINDOW[2], pc.WINDOW[3])
    assert keys == pc.K_FIT * 96 * 72 * 8 and (one._dev["workspace"].get()[:keys] == 0xFF).all()
    assert whole.reference_cost == pf.reference_cost(ref["state"]["terms"])
    tips = whole.fingertips()
    assert tips.shape == (5, 3) and np.array_equal(tips, one.model.fingertips(ref["state"]["pose"], one.cam_from_plane)[0])
    # three generations, then five more on the same frame: the same fit
    two = fitter()
    first = two.fit(depth, labels, c["start"], generations=3)
    second = two.fit(depth, labels, generations=5, fresh=False)
    _assert_state(first, ref["after3"], ref["history"][:3])
    _assert_state(second, ref["state"], ref["history"][3:])
    assert (two._dev["workspace"].get()[:keys] == 0xFF).all()
    # numpy frames are uploaded; no generations is a no-op that reports the state
    same = two.fit(c["depth"], c["labels"], generations=0, fresh=False).get()
    assert same.cost == ref["state"]["cost"] and same.generation == 8 and len(same.history) == 0


@pytest.mark.gpu
def test_rdf_pose_fit_on_a_window_with_an_odd_pixel_count_matches_the_restated_fit(rdf, gpu_runtime):
    c, ref = pc.odd_fit_case(), pc.odd_fit_reference()
    f = rdf.PoseFitter((pc.FRAME_H, pc.FRAME_W), pc.CAM, c["plane"], candidates=pc.K_ODD, window=pc.ODD_WINDOW, seed=pc.SEED)
    got = f.fit(rdf.to_device(c["depth"]), rdf.to_device(c["labels"]), c["start"], generations=pc.G_ODD)
    print(f"device fit on the odd window: history {got.get().history.tolist()}; restated {ref['history']}")
    _assert_state(got, ref["state"], ref["history"])
    keys = f._lb.rdf_hand_scene_workspace_bytes(pc.K_ODD, pc.ODD_WINDOW[2], pc.ODD_WINDOW[3])
    assert keys == pc.K_ODD * 95 * 71 * 8 and (f._dev["workspace"].get()[:keys] == 0xFF).all()


@pytest.mark.gpu
def test_a_device_fit_from_the_true_pose_costs_nothing(rdf, gpu_runtime):
    c, ref = pc.self_fit_case(), pc.self_fit_reference()
    f = rdf.PoseFitter((pc.FRAME_H, pc.FRAME_W), pc.CAM, c["plane"], candidates=pc.K_FIT, window=pc.WINDOW, seed=pc.SEED,
                       w_label=c["cfg"]["w_label"])
    got = f.fit(rdf.to_device(c["depth"]), rdf.to_device(c["labels"]), c["pose"], generations=pc.G_SELF).get()
    assert got.cost == 0 and got.history.tolist() == [0] * pc.G_SELF and got.accepted == 1 and not got.terms.any()
    assert np.array_equal(_bits(got.pose), _bits(c["pose"]))
    _assert_state(got, ref["state"], ref["history"])


@pytest.mark.gpu
def test_track_is_the_chain_of_fits_made_by_hand(rdf, gpu_runtime):
    c = pc.fit_case()
    frames = [pc.camera_frame(c["model"], c["plane"], pc.true_pose(c["model"], step)) for step in range(3)]
    depth = rdf.to_device(np.stack([f[0] for f in frames]))
    labels = rdf.to_device(np.stack([f[1] for f in frames]))
    G = 3

    def fitter():
        return rdf.PoseFitter((pc.FRAME_H, pc.FRAME_W), pc.CAM, c["plane"], candidates=pc.K_FIT, seed=pc.SEED)
    got = fitter().track(depth, labels, c["start"], G).get()
    assert got.poses.shape == (3, 26) and got.history.shape == (3, G) and got.fingertips().shape == (3, 5, 3)
    by_hand, pose = fitter(), c["start"]
    for i in range(3):
        one = by_hand.fit(frames[i][0], frames[i][1], pose, generations=G).get()      # read back and handed in again
        assert np.array_equal(_bits(got.poses[i]), _bits(one.pose)) and got.costs[i] == one.cost, i
        assert np.array_equal(got.terms[i], one.terms) and got.accepted[i] == one.accepted and got.history[i].tolist() == one.history.tolist(), i
        assert all(b <= a for a, b in zip(one.history, one.history[1:]))
        pose = one.pose
    assert not np.array_equal(got.poses[0], got.poses[2])
