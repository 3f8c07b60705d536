"""The scenes and inputs tests/test_pose_fit.py shares between its CPU and GPU tests, and the restated answers, each
computed once and handed out unchanged (callers copy what they change).

`fit_case`, `self_fit_case`   the 96 x 72 window of a 120 x 90 frame: an offset start, and a frame the true pose costs nothing on.
`odd_fit_case`                the same frame under a 95 x 71 window: every candidate's images start elsewhere within 16 bytes.
`cost_case`                   rule C on random images: small windows of every width class, one set per workgroup.
`chunk_cost_case`             rule C where a workgroup takes several sets in a row (CHUNK_CASES).
`select_cases`                rule S: ties, the strict "<", the fresh acceptance, RDF_POSE_MAX_CANDIDATES candidates.
`propose_case`                rules P and K with ranges that clamp."""
import functools
import importlib

import numpy as np

import hand_scene_numpy as hs
import pose_fit_numpy as pf

# the fit: a 96x72 window (odd x0) inside a 120x90 frame, 16 candidates, 8 generations
FRAME_W, FRAME_H = 120, 90
WINDOW = (13, 9, 96, 72)
K_FIT, G_FIT, SEED = 16, 8, 7
CAM = (100., 59.5, 44.5)
HEIGHT, TILT = 5500., 0.1
TRUE_WRIST = (0., -700., 800.)
# the start the fit is given: 10 mm and 6 mm off in the wrist, 0.15 rad in yaw, 0.2 rad in every knuckle
START_OFFSET = {0: 100., 1: 60., 3: 0.15, 7: 0.2, 11: 0.2, 15: 0.2, 19: 0.2, 23: 0.2}
G_SELF = 3


def _modules():
    return (importlib.import_module("3d-beats_amd.hand_model"), importlib.import_module("3d-beats_amd.hand_scene"),
            importlib.import_module("3d-beats_amd.pose_fit"))


def true_pose(model, step=0):
    """A hand above the table with every finger a little bent; `step` moves it on (the frames of a sequence)."""
    pose = model.rest_pose(TRUE_WRIST)
    pose[0] += 40. * step
    pose[3] = 0.1 + 0.03 * step
    pose[4] = -0.1
    for f in range(5):
        pose[7 + 4 * f:10 + 4 * f] = (0.3, 0.25 + 0.02 * step, 0.2)
    return pose


def start_pose(model):
    pose = true_pose(model)
    for j, v in START_OFFSET.items():
        pose[j] += v
    return pose


def config(model, plane, window, K=K_FIT, w_label=0, seed=SEED, anneal_every=8, cam=CAM):
    """The dict pose_fit_numpy.fit takes, with PoseFitter's defaults for everything PoseFitter has a default for."""
    hm, scene, fit = _modules()
    u = model.units_per_mm
    lo, hi = fit.pose_ranges(None, u)
    return {"K": K, "mirrored": model.is_mirrored, "anneal_every": anneal_every, "seed": seed, "window": tuple(window),
            "w_boundary": 10000, "w_label": w_label, "target_mask": 0xFE, "f": np.float32(cam[0]), "ppx": np.float32(cam[1]),
            "ppy": np.float32(cam[2]), "zmin": scene.Z_NEAR, "zmax": scene.Z_FAR, "sigma": fit.pose_vector(fit.DEFAULT_SIGMA, u),
            "lo": lo, "hi": hi, "cam_from_plane": np.linalg.inv(plane)[:3].reshape(12), "geometry": pf.geometry_of(model)}


def mesh_of(model, scheme="fine"):
    hm = _modules()[0]
    return (model.verts, model.vert_part, model.tris, hm.HandModel.label_table(scheme)[model.tri_part].astype(np.uint16))


def camera_frame(model, plane, pose, cam=CAM, W=FRAME_W, H=FRAME_H):
    """(depth, labels) uint16 [H, W] of the hand at `pose` over the table, as HandSceneRenderer.camera_sequence draws it."""
    scene = _modules()[1]
    t = model.part_transforms(pose[None], np.linalg.inv(plane))
    depth, labels, _ = hs.render(W, H, *mesh_of(model), t, scene.table_of_plane(plane)[None], *cam, empty_depth=0)
    return depth[0], labels[0]


@functools.lru_cache(maxsize=None)
def fit_case(mirrored=False):
    """The observed frame of the true pose (the table behind the hand), the start and the config."""
    hm, scene, _ = _modules()
    model = hm.HandModel(mirrored=mirrored)
    plane = scene.look_down_plane(HEIGHT, TILT)
    depth, labels = camera_frame(model, plane, true_pose(model))
    return {"model": model, "plane": plane, "depth": depth, "labels": labels, "start": start_pose(model),
            "true": true_pose(model), "cfg": config(model, plane, WINDOW), "mesh": mesh_of(model)}


@functools.lru_cache(maxsize=None)
def fit_reference():
    """The restated fit of fit_case from its offset start: G_FIT generations in one call, and the state after the first
    three of them."""
    c = fit_case()
    state = pf.new_state(c["start"])
    history = pf.fit(state, 3, True, c["cfg"], c["depth"], c["labels"], 1, c["mesh"])
    after3 = {k: (v.copy() if hasattr(v, "copy") else v) for k, v in state.items()}
    history += pf.fit(state, G_FIT - 3, False, c["cfg"], c["depth"], c["labels"], 1, c["mesh"])
    return {"state": state, "history": history, "after3": after3}


# the same frame under a window with an odd pixel count: 95 * 71 = 6745, so candidate k's images start k * 6745 * 2 bytes
# into their region of the workspace and every candidate of rdf_pose_fit has another head length in rule C
ODD_WINDOW = (13, 9, 95, 71)
K_ODD, G_ODD = 5, 2


@functools.lru_cache(maxsize=None)
def odd_fit_case():
    c = fit_case()
    return dict(c, cfg=config(c["model"], c["plane"], ODD_WINDOW, K=K_ODD))


@functools.lru_cache(maxsize=None)
def odd_fit_reference():
    c = odd_fit_case()
    state = pf.new_state(c["start"])
    history = pf.fit(state, G_ODD, True, c["cfg"], c["depth"], c["labels"], 1, c["mesh"])
    return {"state": state, "history": history}


@functools.lru_cache(maxsize=None)
def self_fit_case():
    """A frame on which the true pose costs exactly nothing: the true pose drawn by rule K's own transforms at window
    size, as rdf_pose_fit draws a candidate, set into a frame whose every other pixel is a flat background."""
    c = fit_case()
    cfg = dict(c["cfg"], w_label=3000)
    x0, y0, ww, wh = cfg["window"]
    t = pf.part_tforms(c["true"][None], cfg["cam_from_plane"], cfg["geometry"], False)
    F = np.float32
    cd, cl, _ = hs.render(ww, wh, *c["mesh"], t, None, F(cfg["f"]), F(cfg["ppx"]) - F(x0), F(cfg["ppy"]) - F(y0), empty_depth=0)
    depth = np.full((FRAME_H, FRAME_W), 5400, np.uint16)
    labels = np.zeros((FRAME_H, FRAME_W), np.uint16)
    depth[y0:y0 + wh, x0:x0 + ww] = np.where(cd[0] != 0, cd[0], 5400)
    labels[y0:y0 + wh, x0:x0 + ww] = cl[0]
    return {"cfg": cfg, "depth": depth, "labels": labels, "mesh": c["mesh"], "pose": c["true"], "model": c["model"], "plane": c["plane"]}


@functools.lru_cache(maxsize=None)
def self_fit_reference():
    c = self_fit_case()
    state = pf.new_state(c["pose"])
    history = pf.fit(state, G_SELF, True, c["cfg"], c["depth"], c["labels"], 1, c["mesh"])
    return {"state": state, "history": history}


# ------------------------------------------------------------------ rule C on random images ---------------------------------
COST_FRAMES = ((33, 17), (200, 70))         # the second: more than one workgroup per candidate
COST_K = (1, 3, 65)
DEPTHS = np.array([0, 0, 1, 65534, 65535, 4000, 4003, 4100, 3990], np.uint16)   # two pixels alone overflow 32 bits of sq
OBSERVED_LABELS = np.array([0, 1, 2, 3, 5, 7, 8, 63, 64, 100, 65535], np.uint16)
COST_MASK = 0xFE | (1 << 63)


def cost_windows(W, H):
    """Odd x0 with ww 1, 7, 8 and 33 (33 from x0 = 0 where the frame is no wider), one window on each edge of the frame,
    and the whole frame."""
    x33 = 0 if W <= 33 + 1 else 5
    return ((3, 2, 1, 5), (5, 1, 7, 9), (1, 3, 8, 6), (x33, 4, 33, 3), (0, 5, 9, 4), (7, 0, 11, 3), (W - 13, 2, 13, 7),
            (3, H - 5, 10, 5), (0, 0, W, H))


@functools.lru_cache(maxsize=None)
def cost_case(W, H, r):
    """Random observed frame and, per window and K, random candidates with the restated terms."""
    rng = np.random.default_rng(1000 * W + 10 * H + r)
    depth = rng.choice(DEPTHS, (H, W))
    labels = rng.choice(OBSERVED_LABELS, (H // r, W // r))
    runs = []
    for window in cost_windows(W, H):
        for K in COST_K:
            cd = rng.choice(DEPTHS, (K, window[3], window[2]))
            cl = rng.integers(0, 9, (K, window[3], window[2])).astype(np.uint16)
            base = rng.integers(0, 1 << 40, (K, 4)).astype(np.uint64)       # the call adds to what is there
            runs.append({"window": window, "K": K, "cand_depth": cd, "cand_labels": cl, "base": base,
                         "terms": pf.cost_terms(depth, labels, r, window, cd, cl, COST_MASK)})
    return {"depth": depth, "labels": labels, "runs": runs}


# ------------------------------------------------------------------ rule C, several trips per workgroup --------------------
# launch_cost deals a candidate's groups of eight pixels out in sets of 256 (one per lane): sets = ceil(floor(n_px / 8) / 256),
# a workgroup takes chunk = clamp(floor(sets * K / 1024), 1, 16) sets in a row, and a candidate gets ceil(sets / chunk)
# workgroups.  cost_case above never leaves chunk = 1.
# name: frame, window, K, the r's, the element offsets of the candidates' depth and labels in their arrays (odd; 8 apart
# in the second row, so that the labels keep the depth's 16-byte boundary and are loaded as vectors), then what the plan must
# come to: sets, chunk, workgroups per candidate.
#   the second row: the last workgroup's first trip is full (set 3), its second ends inside wave 1 (set 4 holds groups 1024
#   to 1123 or 1124), its third is empty;  the third row: three of four trips do nothing, at K = RDF_POSE_MAX_CANDIDATES.
# The clamp at 16 is left out: it needs sets * K >= 16384, about 33 million candidate pixels, and with ceil(sets / chunk)
# workgroups it changes only how the same sets are dealt out.
CHUNK_CASES = {
    "the benchmarked plan": ((300, 260), (5, 3, 256, 256), 64, (1, 2), (3, 1), (32, 2, 16)),
    "sets no multiple of chunk": ((120, 100), (7, 4, 100, 90), 615, (1,), (5, 13), (5, 3, 2)),
    "more trips than sets": ((33, 17), (0, 0, 33, 17), 4096, (1,), (7, 1), (1, 4, 1)),
}


@functools.lru_cache(maxsize=None)
def chunk_cost_case(name, r):
    """One run of rule C on random images: what cost_case's runs hold, a base that is nowhere zero, and the offsets."""
    (W, H), window, K, rs, offsets, _ = CHUNK_CASES[name]
    assert r in rs
    rng = np.random.default_rng(7000 + 10 * list(CHUNK_CASES).index(name) + r)
    depth = rng.choice(DEPTHS, (H, W))
    labels = rng.choice(OBSERVED_LABELS, (H // r, W // r))
    cd = rng.choice(DEPTHS, (K, window[3], window[2]))
    cl = rng.integers(0, 9, (K, window[3], window[2])).astype(np.uint16)
    base = rng.integers(1, 1 << 40, (K, 4)).astype(np.uint64)
    return {"depth": depth, "labels": labels, "window": window, "K": K, "cand_depth": cd, "cand_labels": cl, "base": base,
            "offsets": offsets, "terms": pf.cost_terms(depth, labels, r, window, cd, cl, COST_MASK)}


# ------------------------------------------------------------------ rule S --------------------------------------------------
MAX_CANDIDATES = 4096           # RDF_POSE_MAX_CANDIDATES: every lane of k_pose_select walks 64 of them


def _terms(rows):
    return np.array(rows, np.uint64).reshape(-1, 4)


def select_cases():
    """(name, K, terms, state before, w_boundary, w_label, fresh_first): ties, the strict "<", the fresh acceptance."""
    rng = np.random.default_rng(3)
    out = []

    def add(name, terms, cost_before, w_boundary=10000, w_label=0, fresh=False, g=5, accepted=2):
        terms = _terms(terms)
        state = pf.new_state(np.arange(26) * 0.5)
        state.update(cost=int(cost_before), terms=np.array([9, 8, 7, 6], np.uint64), g=g, accepted=accepted)
        out.append((name, len(terms), terms, state, w_boundary, w_label, fresh))
    add("the lowest cost wins", [(1, 0, 0, 500), (0, 0, 0, 700), (0, 1, 0, 0)], 10 ** 6)
    add("of equal costs the lowest k", [(1, 0, 0, 0), (0, 0, 4, 2000), (0, 1, 0, 0), (0, 0, 0, 10000)], 10 ** 6, w_label=2000)
    add("equal to the incumbent is not better", [(0, 0, 0, 800), (0, 0, 0, 900)], 800)
    add("one below the incumbent is", [(0, 0, 0, 900), (0, 0, 0, 799)], 800)
    add("nothing better: only g moves", [(1, 1, 0, 0), (0, 0, 0, 801)], 800)
    add("a fresh first generation takes the best although it is worse", [(0, 0, 0, 900), (0, 0, 0, 850)], 800, fresh=True)
    add("one candidate", [(2, 3, 4, 5)], 10 ** 9, w_label=7)
    many = rng.integers(50, 1000, (130, 4))
    many[70] = many[6] = many[127] = (0, 0, 0, 3)          # a tie between lanes and between a lane's own candidates
    add("130 candidates, a tie across the wave", many, 10 ** 12)
    big = np.array([[2 ** 31 - 1, 2 ** 31 - 1, 0, 2 ** 62], [2 ** 31 - 1, 2 ** 31 - 1, 0, 2 ** 62 - 1]], np.uint64)
    add("costs beyond 2^63", big, 2 ** 64 - 1, w_boundary=2 ** 32 - 1)
    most = rng.integers(50, 1000, (MAX_CANDIDATES, 4))
    most[61] = most[4032] = most[4095] = (0, 0, 0, 3)       # a low k in lane 61, a high k in lane 0, the last k in lane 63
    add("4096 candidates, the minimum three times", most, 10 ** 12)
    add("4096 candidates, all equal", np.tile((1, 2, 3, 4), (MAX_CANDIDATES, 1)), 10 ** 12, w_label=5)
    return out


def select_poses(K):
    return np.random.default_rng(K).normal(size=(K, 26))


# ------------------------------------------------------------------ rule P --------------------------------------------------
def propose_case(K, mirrored, g, fresh):
    """A config with narrow ranges around the incumbent, so that both ends clamp, and the restated candidates."""
    hm, scene, fit = _modules()
    model = hm.HandModel(mirrored=mirrored)
    rng = np.random.default_rng(100 * K + 10 * g + mirrored)
    plane = scene.look_down_plane(HEIGHT, 0.15)
    cfg = config(model, plane, (0, 0, 8, 8), K=K, seed=4321 + K)
    inc = model.sample_poses(1, rng)[0]
    cfg["lo"] = inc - np.abs(rng.normal(size=26)) * cfg["sigma"] * 1.2
    cfg["hi"] = inc + np.abs(rng.normal(size=26)) * cfg["sigma"] * 1.2
    poses = pf.propose(inc, cfg["seed"], g, K, cfg["sigma"], cfg["lo"], cfg["hi"], cfg["anneal_every"], fresh)
    return {"cfg": cfg, "inc": inc, "poses": poses, "tforms": pf.part_tforms(poses, cfg["cam_from_plane"], cfg["geometry"], mirrored),
            "model": model}
