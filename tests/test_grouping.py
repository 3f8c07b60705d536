"""The hand-group image on the device (rdf_hand_groups, HandGrouping, CppGrouping, and the three stand-alone kernels of the
reference's host round trip) against the reference's own grouping.cpp (tests/golden/grouping_v1.npz and, for the
tile-crossing and limit-sized frames of tests/grouping_cases.py, grouping_v2.npz; both recorded by
tests/golden/make_grouping_golden.py) and against the CPU restatement in tests/grouping_numpy.py."""
import ctypes
import functools
import importlib
import os

import numpy as np
import pytest

import grouping_cases as gcases
import grouping_numpy as gnp

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "grouping_v1.npz")
GOLDEN_V2 = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "grouping_v2.npz")
NEW_SYMBOLS = ("rdf_shrink_image", "rdf_write_pixel_groups_to_stencil_image", "rdf_grow_groups",
               "rdf_hand_groups_workspace_bytes", "rdf_hand_groups")
AUTO, RESIDENT, GLOBAL = 0, 1, 2


def _golden():
    z = np.load(GOLDEN)
    return [(str(n), z[f"{n}/img"], float(z[f"{n}/pct"]), z[f"{n}/g_info"], z[f"{n}/coords"]) for n in z["names"]]


def _rows(c):
    c = np.asarray(c).reshape(-1, 3)
    return c[np.lexsort((c[:, 2], c[:, 1], c[:, 0]))]


# ------------------------------------------------------------------ CPU ------------------------------------------------------
def test_golden_fixture_is_small_data():
    assert os.path.getsize(GOLDEN) < 1_000_000
    z = np.load(GOLDEN, allow_pickle=False)
    assert len(z["names"]) >= 30


def test_restatement_matches_the_reference_fixture():
    for name, img, pct, g_info, coords in _golden():
        gi, stencil, comps = gnp.make_groups(img, pct)
        assert np.array_equal(gi.view(np.uint32), g_info.view(np.uint32)), name
        want_st = gnp.write_stencil(coords, len(coords), img.shape)
        assert np.array_equal(stencil, want_st), name
        assert np.array_equal(_rows(gnp.coords_of(stencil)), _rows(coords)), name
        assert np.array_equal(gnp.grow(stencil), gnp.grow(want_st)), name
        assert int(gi[0, 0]) + int(gi[1, 0]) == len(coords), name


def test_reference_toy_picks_the_bottom_band():
    name, img, pct, g_info, coords = _golden()[0]
    assert name == "toy" and g_info[0, 0] == 15 and abs(g_info[0, 1] - 3.4667) < 1e-4


def test_grow_and_stencil_restatements_on_hand_derived_cases():
    s = np.array([[0, 0, 0, 0],
                  [0, 1, 0, 2],
                  [0, 0, 0, 0]], np.uint16)
    # left, right, up, down: (1, 2) sees 1 on its left before 2 on its right; (0, 2) sees nothing left/right, 2 is not up
    want = np.array([[0, 1, 0, 2],
                     [1, 1, 1, 2],
                     [0, 1, 0, 2]], np.uint16)
    assert np.array_equal(gnp.grow(s), want)
    s2 = np.array([[0, 2], [1, 0]], np.uint16)
    assert np.array_equal(gnp.grow(s2), np.array([[2, 2], [1, 1]], np.uint16))   # (0,0): right before down
    c = np.array([[0, 1, 1], [1, 0, 2], [7, 7, 7]], np.int32)
    assert np.array_equal(gnp.write_stencil(c, 2, (2, 2)), np.array([[0, 1], [2, 0]], np.uint16))
    assert np.array_equal(gnp.shrink(np.arange(30, dtype=np.uint16).reshape(5, 6), 1), np.array([[0, 2, 4], [12, 14, 16]]))

@functools.lru_cache(maxsize=None)
def _golden_v2():
    """{name: (img, pct, g_info, coords or None)} of grouping_v2.npz, in the order of grouping_cases.cases()."""
    z = np.load(GOLDEN_V2, allow_pickle=False)
    out = {}
    for n in z["names"]:
        n = str(n)
        has = bool(z[f"{n}/has_coords"]) if f"{n}/has_coords" in z.files else True
        out[n] = (z[f"{n}/img"], float(z[f"{n}/pct"]), z[f"{n}/g_info"], z[f"{n}/coords"] if has else None)
    return out


@functools.lru_cache(maxsize=None)
def _want_v2(name):
    """The restatement's (groups, g_info, comps, coords rows) of one v2 case: computed once, shared, never written."""
    img, pct, _, _ = _golden_v2()[name]
    return gnp.hand_groups(img, 0, pct)


def _flood(img):
    """Components by a raster-order flood fill over the four neighbours, as grouping.cpp walks them (no scipy): int32
    [Hm, Wm] of each foreground pixel's first-met pixel = its component's minimum raster index, -1 for background."""
    hm, wm = img.shape
    fg = (img != 0).reshape(-1).tolist()
    out = [-1] * (hm * wm)
    for s in range(hm * wm):
        if not fg[s] or out[s] >= 0:
            continue
        out[s] = s
        todo = [s]
        while todo:
            i = todo.pop()
            y, x = divmod(i, wm)
            for ok, j in ((x > 0, i - 1), (x + 1 < wm, i + 1), (y > 0, i - wm), (y + 1 < hm, i + wm)):
                if ok and fg[j] and out[j] < 0:
                    out[j] = s
                    todo.append(j)
    return np.array(out, np.int32).reshape(hm, wm)


def test_v2_fixture_is_small_data_of_the_named_cases():
    assert os.path.getsize(GOLDEN_V2) < 1_000_000
    built = gcases.cases()
    gold = _golden_v2()
    assert list(gold) == [name for name, _, _ in built] and len(built) == 17
    for name, img, pct in built:
        g_img, g_pct, g_info, coords = gold[name]
        assert img.dtype == np.uint16 and np.array_equal(img, g_img), name
        assert np.float32(pct) == np.float32(g_pct), name
        assert (coords is None) == (name in gcases.WITHOUT_COORDS), name
    assert [n for n, (img, _, _, _) in gold.items() if not gcases.fits_resident(img)] == [
        "checker_127x126", "row_16001x1", "comb_200x150", "comb_upside_down_200x150",
        "large_sums_400x300", "large_sums_one_side_400x300"]


def test_restatement_matches_the_v2_reference_fixture():
    for name, (img, pct, g_info, coords) in _golden_v2().items():
        _, gi, _, rows = _want_v2(name)
        stencil = gnp.make_groups(img, pct)[1]
        assert np.array_equal(gi.view(np.uint32), g_info.view(np.uint32)), name
        assert int(gi[0, 0]) + int(gi[1, 0]) == len(rows), name
        if coords is None:
            continue
        assert np.array_equal(stencil, gnp.write_stencil(coords, len(coords), img.shape)), name
        assert np.array_equal(_rows(rows), _rows(coords)), name
        assert len(coords) == len(rows), name


# name: (components, size of the largest), from each case's construction
V2_COMPONENTS = {
    "serpentine_160x100": (1, 50 * 160 + 50), "two_serpentines_160x100": (2, 50 * 79 + 50),
    "checker_160x100": (8000, 1), "checker_125x127": ((125 * 127 + 1) // 2, 1), "spiral_121": (1, 7439),
    "staircase_130x120": (1, 240), "border_lines_100x90": (11, 400),
    "corner_touch_100x90": (10, 1), "full_160x100": (1, 16000), "empty_160x100": (0, 0),
    "checker_127x126": (8001, 1), "row_16001x1": (4572, 3), "column_1x4099": (1, 4099),
    "comb_200x150": (1, 100 * 150 + 100), "comb_upside_down_200x150": (1, 15100),
    "large_sums_400x300": (2, 200 * 300 - 2), "large_sums_one_side_400x300": (1, 400 * 300 - 2),
}


def test_the_hard_cases_are_what_they_claim():
    gold = _golden_v2()
    assert set(V2_COMPONENTS) == set(gold)
    for name, (img, pct, g_info, _) in gold.items():
        comps = _flood(img)
        assert np.array_equal(comps, _want_v2(name)[2]), name              # the restatement's scipy labels agree
        roots, sizes = np.unique(comps[comps >= 0], return_counts=True)
        assert (len(roots), int(sizes.max()) if len(sizes) else 0) == V2_COMPONENTS[name], name
        fg = np.nonzero(img.reshape(-1))[0]
        if name.startswith("checker") or name == "corner_touch_100x90":    # every pixel is its own component
            assert np.array_equal(comps.reshape(-1)[fg], fg), name
        if name.split("_")[0] in ("serpentine", "spiral", "comb", "staircase", "column", "full"):
            assert (comps.reshape(-1)[fg] == 0).all() and fg[0] == 0, name
    sizes = {n: img.size for n, (img, _, _, _) in gold.items()}
    assert sizes["serpentine_160x100"] == sizes["checker_160x100"] == gcases.RESIDENT_MAX_PIXELS == 16000
    assert sizes["checker_127x126"] == 16002 and sizes["row_16001x1"] == 16001 and sizes["checker_125x127"] == 15875
    # resident_lds_bytes of grouping_hip.hip: parent int32 [P] + {count, sum x, sum y} int32 [ceil(P / 2)]
    lds = lambda p: 4 * p + 12 * ((p + 1) // 2)
    assert lds(16000) == 160_000 and lds(16000) + 152 <= 160 * 1024 and lds(15875) == 4 * 15875 + 12 * 7938
    # the ties: 4000 equal bidders per side in the 160x100 checkerboard, the smallest root of each side wins
    gi = gold["checker_160x100"][2]
    assert gi.tolist() == [[1, 0, 0], [1, 80, 0]]
    two = _flood(gold["two_serpentines_160x100"][0])
    assert set(np.unique(two).tolist()) == {-1, 0, 81}
    # the corner pairs: ten one-pixel components, diagonal neighbours never joined
    ys, xs = np.nonzero(gold["corner_touch_100x90"][0])
    assert list(zip(ys.tolist(), xs.tolist())) == [(k + d, k + d) for k in (15, 31, 47, 63, 79) for d in (0, 1)]
    # the row: runs 3, 1, 3, 1, ...: 2286 components of size 3, 2286 of size 1, all of them bid at pct = 0
    row = _flood(gold["row_16001x1"][0])
    assert np.unique(np.unique(row[row >= 0], return_counts=True)[1], return_counts=True)[1].tolist() == [2286, 2286]


def test_library_exports_the_grouping_entry_points(rdf):
    _lib = importlib.import_module("3d-beats_amd._lib")
    _build = importlib.import_module("3d-beats_amd._build")
    lib = ctypes.CDLL(_build.build())
    for name in NEW_SYMBOLS:
        assert name in _lib.SIGNATURES, name
        getattr(lib, name)
    assert "grouping_hip.hip" in " ".join(_build.SOURCES)
    lib.rdf_hand_groups_workspace_bytes.restype = ctypes.c_size_t
    assert lib.rdf_hand_groups_workspace_bytes(2, 848, 480, 0) == 2 * 16 + 2 * 848 * 480 * 16
    assert lib.rdf_hand_groups_workspace_bytes(-1, 848, 480, 0) == 0
    assert rdf.HandGrouping is importlib.import_module("3d-beats_amd.grouping").HandGrouping


# ------------------------------------------------------------------ GPU ------------------------------------------------------
def _launch(rdf, depth, level, pct, path, coords=True, workspace=True):
    """depth uint16 [n, H, W] -> (return code, (groups, g_info, comps, coords)) from rdf_hand_groups through the C ABI.
    Every output starts from a sentinel fill (7, NaN, -5, -9; 0xAB in the workspace); a shape that shrinks to no pixels
    gets one-element outputs."""
    lib = rdf.get_runtime().lib
    n, h, w = depth.shape
    hm, wm = h >> level, w >> level
    p1 = max(hm * wm, 1)
    d = rdf.to_device(depth)
    g = rdf.DeviceArray((n, hm, wm) if hm * wm else (n, 1), np.uint16).fill(7)
    gi = rdf.DeviceArray((n, 2, 3), np.float32).fill(np.float32(np.nan))
    comps = rdf.DeviceArray((n, hm, wm) if hm * wm else (n, 1), np.int32).fill(-5)
    co = rdf.DeviceArray((n, p1, 3), np.int32).fill(-9) if coords else None
    ws = rdf.DeviceArray((max(int(lib.rdf_hand_groups_workspace_bytes(n, w, h, level)), 8),), np.uint8).fill(0xAB)
    rc = lib.rdf_hand_groups(d.ptr, n, w, h, level, float(pct), g.ptr, gi.ptr, comps.ptr, co.ptr if coords else None,
                             ws.ptr if workspace else None, path, rdf.get_runtime().stream())
    rdf.get_runtime().synchronize()
    return rc, (g.get(), gi.get(), comps.get(), (co.get() if coords else None))


def _run(rdf, depth, level, pct, path, coords=True):
    """depth uint16 [n, H, W] -> (groups, g_info, comps, coords) from rdf_hand_groups through the C ABI."""
    _lib = importlib.import_module("3d-beats_amd._lib")
    rc, got = _launch(rdf, depth, level, pct, path, coords)
    _lib.check(rdf.get_runtime().lib, rc, "rdf_hand_groups")
    return got


def _check_frame(got, i, depth, level, pct, ref_ginfo=None, ref_coords=None, want=None):
    groups, g_info, comps, coords = got
    want_g, want_gi, want_c, want_rows = want if want is not None else gnp.hand_groups(depth, level, pct)
    assert np.array_equal(groups[i], want_g)
    assert np.array_equal(g_info[i].view(np.uint32), want_gi.view(np.uint32)), (g_info[i], want_gi)
    assert np.array_equal(comps[i], want_c)
    n = len(want_rows)
    assert np.array_equal(coords[i][:n], want_rows)           # raster order: exactly the restatement's rows
    assert (coords[i][n:] == -9).all()                          # rows past the two groups are untouched
    if ref_ginfo is not None:
        assert np.array_equal(g_info[i].view(np.uint32), ref_ginfo.view(np.uint32))
    if ref_coords is not None:
        assert np.array_equal(_rows(coords[i][:n]), _rows(ref_coords))


@pytest.mark.gpu
@pytest.mark.parametrize("path", [RESIDENT, GLOBAL])
def test_both_paths_match_the_reference_fixture(path, rdf, gpu_runtime):
    for name, img, pct, g_info, coords in _golden():
        got = _run(rdf, img[None], 0, pct, path)
        _check_frame(got, 0, img, 0, pct, g_info, coords)


def _fuzz(rng, n, h, w):
    out = np.zeros((n, h, w), np.uint16)
    for k in range(n):
        dens = rng.choice([0.0, 0.3, 0.5, 0.6, 0.9, 1.0])
        out[k] = (rng.random((h, w)) < dens) * rng.integers(1, 2000, (h, w))
        if k % 3 == 1:                                          # blobs with holes
            yy, xx = np.mgrid[:h, :w]
            m = np.zeros((h, w), bool)
            for _ in range(int(rng.integers(1, 6))):
                cy, cx, r = rng.uniform(0, h), rng.uniform(0, w), rng.uniform(2, max(h, w) / 3)
                m |= (yy - cy) ** 2 + (xx - cx) ** 2 < r * r
            out[k] = np.where(m & (rng.random((h, w)) > 0.05), 500, 0)
    return out.astype(np.uint16)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 3, 128])
def test_batches_on_both_paths_match_the_restatement(n, rdf, gpu_runtime):
    rng = np.random.default_rng(100 + n)
    h, w, level = (60, 106, 0) if n == 128 else (90 * 2, 160 * 2, 1)
    depth = _fuzz(rng, n, h, w)
    if n >= 3:
        depth[0] = 0                                            # mix in an empty frame and a full one
        depth[-1] = 3
    pct = 0.06 if n != 3 else 0.0
    res = _run(rdf, depth, level, pct, RESIDENT)
    glb = _run(rdf, depth, level, pct, GLOBAL)
    for a, b in zip(res, glb):
        assert np.array_equal(a, b)                             # the two paths agree bit for bit
    for i in (range(n) if n <= 3 else [0, 1, 2, 5, 17, 64, 100, n - 1]):
        _check_frame(res, i, depth[i], level, pct)
    again = _run(rdf, depth, level, pct, AUTO)                  # and again: the same bits
    for a, b in zip(res, again):
        assert np.array_equal(a, b)


def _live_like(rdf, idx, h=480, w=848):
    f = rdf.synth.live_frame(idx, h, w)
    return np.where(f == 65535, 0, f).astype(np.uint16)         # the camera's convention: 0 = no pixel


@pytest.mark.gpu
@pytest.mark.parametrize("level", [0, 1, 3])
def test_live_like_frames_at_levels_0_1_3(level, rdf, gpu_runtime):
    depth = np.stack([_live_like(rdf, 4200 + k) for k in range(2)])
    depth[1, :, 300:310] = 0                                    # split the second frame's surface in two
    got = _run(rdf, depth, level, 0.06, AUTO)
    for i in range(2):
        _check_frame(got, i, depth[i], level, 0.06)
    assert got[1][0, :, 0].sum() > 0
    if level == 3:                                              # the app's size runs the resident path; same as the global
        glb = _run(rdf, depth, level, 0.06, GLOBAL)
        for a, b in zip(got, glb):
            assert np.array_equal(a, b)


@pytest.mark.gpu
def test_stand_alone_kernels_are_byte_exact_and_chain_to_the_fused_call(rdf, gpu_runtime):
    po = importlib.import_module("3d-beats_amd.cuda.points_ops").PointsOps()
    cg = importlib.import_module("3d-beats_amd.cpp_grouping").CppGrouping()
    H, W, L = 480, 848, 3
    depth = _live_like(rdf, 4300)
    dims = (H >> L, W >> L)
    d = rdf.GpuBuffer((H, W), np.uint16, depth)
    mm = rdf.GpuBuffer(dims, np.uint16)
    po.shrink_image(np.array((W, H), np.int32), np.int32(L), d.cu(), mm.cu(), grid=(1, 1, 1), block=(32, 32, 1))
    mm_h = mm.cu().get()
    assert np.array_equal(mm_h, gnp.shrink(depth, L))
    coords = np.zeros((dims[0] * dims[1], 3), np.int32)
    g_info = np.zeros((2, 3), np.float32)
    cg.make_groups(mm_h, coords, g_info, 0.06)
    want_gi, want_st, _ = gnp.make_groups(mm_h, 0.06)
    assert np.array_equal(g_info.view(np.uint32), want_gi.view(np.uint32))
    n = int(g_info[0, 0]) + int(g_info[1, 0])
    assert n > 0
    st = rdf.GpuBuffer(dims, np.uint16)
    st.cu().fill(0)
    cgpu = rdf.GpuBuffer(coords.shape, np.int32, coords)
    po.write_pixel_groups_to_stencil_image(cgpu.cu(), np.int32(n), st.cu(), np.array(dims, np.int32))
    assert np.array_equal(st.cu().get(), want_st)
    grown = rdf.GpuBuffer(dims, np.uint16)
    po.grow_groups(np.array([dims[1], dims[0]], np.int32), st.cu(), grown.cu())
    assert np.array_equal(grown.cu().get(), gnp.grow(want_st))
    hg = rdf.HandGrouping((H, W), L, 0.06)
    fused = rdf.GpuBuffer(dims, np.uint16)
    hg.make_group_image(d, fused)
    assert np.array_equal(fused.cu().get(), grown.cu().get())
    assert np.array_equal(hg.g_info.get()[0].view(np.uint32), g_info.view(np.uint32))
    # grow on a stencil that touches both hands and every border
    rng = np.random.default_rng(5)
    s = (rng.integers(0, 3, (37, 53)) * (rng.random((37, 53)) < 0.2)).astype(np.uint16)
    a, b = rdf.to_device(s), rdf.DeviceArray(s.shape, np.uint16)
    po.grow_groups(np.array([53, 37], np.int32), a, b)
    assert np.array_equal(b.get(), gnp.grow(s))


@pytest.mark.gpu
def test_argument_errors(rdf, gpu_runtime):
    lib = gpu_runtime.lib
    s = gpu_runtime.stream()
    d = rdf.DeviceArray((480, 848), np.uint16).fill(0)
    g = rdf.DeviceArray((480, 848), np.uint16)
    ws = rdf.DeviceArray((int(lib.rdf_hand_groups_workspace_bytes(1, 848, 480, 0)),), np.uint8)
    BAD, NULL, LARGE = -1, -2, -3
    assert lib.rdf_hand_groups(None, 1, 848, 480, 3, 0.06, g.ptr, None, None, None, ws.ptr, 0, s) == NULL
    assert lib.rdf_hand_groups(d.ptr, 1, 848, 480, 3, 0.06, None, None, None, None, ws.ptr, 0, s) == NULL
    assert lib.rdf_hand_groups(d.ptr, 1, 848, 480, 0, 0.06, g.ptr, None, None, None, None, 0, s) == NULL   # global: workspace
    assert lib.rdf_hand_groups(d.ptr, 1, -848, 480, 3, 0.06, g.ptr, None, None, None, ws.ptr, 0, s) == BAD
    assert lib.rdf_hand_groups(d.ptr, -1, 848, 480, 3, 0.06, g.ptr, None, None, None, ws.ptr, 0, s) == BAD
    assert lib.rdf_hand_groups(d.ptr, 1, 848, 480, -1, 0.06, g.ptr, None, None, None, ws.ptr, 0, s) == BAD
    assert lib.rdf_hand_groups(d.ptr, 1, 848, 480, 3, 0.06, g.ptr, None, None, None, ws.ptr, 3, s) == BAD
    assert lib.rdf_hand_groups(d.ptr, 1, 848, 480, 0, 0.06, g.ptr, None, None, None, ws.ptr, RESIDENT, s) == BAD
    assert lib.rdf_hand_groups(d.ptr, 1, 1 << 14, 1 << 14, 0, 0.06, g.ptr, None, None, None, ws.ptr, 0, s) == LARGE
    assert lib.rdf_hand_groups(d.ptr, 0, 848, 480, 3, 0.06, g.ptr, None, None, None, ws.ptr, 0, s) == 0
    assert lib.rdf_shrink_image(848, 480, -1, d.ptr, g.ptr, s) == BAD
    assert lib.rdf_shrink_image(848, 480, 3, None, g.ptr, s) == NULL
    assert lib.rdf_grow_groups(-1, 4, d.ptr, g.ptr, s) == BAD
    assert lib.rdf_grow_groups(8, 4, d.ptr, None, s) == NULL
    assert lib.rdf_write_pixel_groups_to_stencil_image(None, 3, g.ptr, 4, 4, s) == NULL
    assert lib.rdf_write_pixel_groups_to_stencil_image(d.ptr, -3, g.ptr, 4, 4, s) == BAD
    hg = rdf.HandGrouping((480, 848), 3, 0.06)
    with pytest.raises(AssertionError):
        hg.make_group_image(d, rdf.DeviceArray((480, 848), np.uint16))   # wrong output shape
    gpu_runtime.synchronize()


def _two_hands_frame(rdf, H=480, W=848):
    live = np.where(rdf.synth.live_frame(4400, H, W) == 65535, 700, rdf.synth.live_frame(4400, H, W)).astype(np.uint16)
    yy, xx = np.mgrid[:H, :W]
    m = np.zeros((H, W), bool)
    for cx in (W * 0.27, W * 0.71):
        cy = H * 0.6
        m |= ((yy - cy) / (H * 0.2)) ** 2 + ((xx - cx) / (W * 0.11)) ** 2 <= 1
        for k in range(5):
            m |= (np.abs(xx - (cx + (k - 2) * W * 0.04)) < 9) & (yy > cy - H * 0.5) & (yy < cy)
    depth = np.where(m, live, 0).astype(np.uint16)
    depth[(np.random.default_rng(8).random((H, W)) < 0.004)] = 0
    return depth


@pytest.mark.gpu
def test_depth_frame_to_fingertip_heights_without_a_host_round_trip(rdf, gpu_runtime):
    H, W, R, L = 480, 848, 2, 3
    pl = importlib.import_module("3d-beats_amd.pipeline")
    synth = rdf.synth
    depth = _two_hands_frame(rdf)
    f0, f1 = synth.forest(3, 9, 4, "trained", 60), synth.forest(3, 10, 5, "trained", 70)
    cfg = {"layers": [{"model": rdf.DecisionForest.from_numpy(f0)},
                      {"model": rdf.DecisionForest.from_numpy(f1), "filter_model": 0, "filter_model_class": 3}],
           "conditions": [[0, 1], [0, 2], [1, 3], [0, 3], [0, 4], [0, 5], [0, 6], [0, 7]],
           "label_colors": [[10 * i, 255 - 10 * i, i, 255] for i in range(1, 8)]}
    lf = rdf.LayeredDecisionForest(cfg, (H, W), R)
    pipe = pl.HandPipeline(lf, (H, W), R, 0.75, 5, np.linspace(20., 60., 7).astype(np.float32), [3, 4, 5, 6, 7],
                           (421.3, 420.9, 423.1, 238.6), np.eye(4, dtype=np.float32), depth_mm_level=L)
    dbuf = rdf.GpuBuffer((H, W), np.uint16, depth)
    hg = rdf.HandGrouping((H, W), L, 0.06)
    groups = rdf.GpuBuffer((H >> L, W >> L), np.uint16)
    want_groups, want_gi, _, _ = gnp.hand_groups(depth, L, 0.06)
    assert want_gi[0, 0] > 0 and want_gi[1, 0] > 0
    ref_groups = rdf.GpuBuffer((H >> L, W >> L), np.uint16, want_groups)
    for g_id, flip in ((1, False), (2, True)):
        hg.make_group_image(dbuf, groups)                      # no synchronisation between the two calls
        means, heights = pipe.run(dbuf, groups, g_id, flip)
        labels = pipe.labels_image.cu().get()
        means_ref, heights_ref = pipe.run(dbuf, ref_groups, g_id, flip)
        assert np.array_equal(labels, pipe.labels_image.cu().get())
        assert (labels != 65535).sum() > 500
        assert np.array_equal(means.view(np.uint64), means_ref.view(np.uint64))
        assert np.array_equal(heights.view(np.uint64), heights_ref.view(np.uint64))
    assert np.array_equal(groups.cu().get(), want_groups)


@pytest.mark.gpu
@pytest.mark.parametrize("level", [3, 1])
def test_make_group_image_replays_from_a_captured_graph(level, rdf, gpu_runtime):
    import torch
    H, W = 480, 848
    hg = rdf.HandGrouping((H, W), level, 0.06)
    dims = (H >> level, W >> level)
    dbuf = rdf.GpuBuffer((H, W), np.uint16, _two_hands_frame(rdf))
    out, gi = rdf.GpuBuffer(dims, np.uint16), rdf.DeviceArray((1, 2, 3), np.float32)
    comps = rdf.DeviceArray(dims, np.int32)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        hg.make_group_image(dbuf, out, gi, comps)              # warm-up
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        hg.make_group_image(dbuf, out, gi, comps)
    for k in range(3):
        frame = _live_like(rdf, 4500 + k)
        frame[:, 400 + 20 * k:430 + 20 * k] = 0
        dbuf.cu().set(frame)
        out.cu().fill(9)
        graph.replay()
        torch.cuda.synchronize()
        got = (out.cu().get(), gi.get(), comps.get())
        direct_out, direct_gi, direct_c = rdf.GpuBuffer(dims, np.uint16), rdf.DeviceArray((1, 2, 3), np.float32), \
            rdf.DeviceArray(dims, np.int32)
        hg.make_group_image(dbuf, direct_out, direct_gi, direct_c)
        assert np.array_equal(got[0], direct_out.cu().get())
        assert np.array_equal(got[1].view(np.uint32), direct_gi.get().view(np.uint32))
        assert np.array_equal(got[2], direct_c.get())
        want_g, want_gi, _, _ = gnp.hand_groups(frame, level, 0.06)
        assert np.array_equal(got[0], want_g) and np.array_equal(got[1][0].view(np.uint32), want_gi.view(np.uint32))
    del graph


# ------------------------------------ tile-crossing shapes and the resident limit ---------------------------------------------
def _paths_for(img):
    return (RESIDENT, GLOBAL) if gcases.fits_resident(img) else (GLOBAL,)


def _same_bits(a, b):
    for u, v in zip(a, b):
        assert u.dtype == v.dtype and u.shape == v.shape
        assert np.array_equal(u.view(np.uint8), v.view(np.uint8))   # NaN sentinels compare as bytes


@pytest.mark.gpu
@pytest.mark.parametrize("name", gcases.NAMES)
def test_tile_crossing_shapes_match_the_reference_on_both_paths(name, rdf, gpu_runtime):
    img, pct, g_info, coords = _golden_v2()[name]
    first = None
    for path in _paths_for(img):
        got = _run(rdf, img[None], 0, pct, path)
        _check_frame(got, 0, img, 0, pct, g_info, coords, want=_want_v2(name))
        _same_bits(got, _run(rdf, img[None], 0, pct, path))        # the order lanes and workgroups ran in does not show
        if first is not None:
            _same_bits(first, got)                                  # resident == global
        first = got


@pytest.mark.gpu
def test_resident_limit(rdf, gpu_runtime):
    BAD, NULL = -1, -2
    gold = _golden_v2()
    for name in ("serpentine_160x100", "checker_160x100"):         # P = 16000: 160 000 B of dynamic LDS
        img, pct, g_info, coords = gold[name]
        rc_res, res = _launch(rdf, img[None], 0, pct, RESIDENT)
        rc_auto, auto = _launch(rdf, img[None], 0, pct, AUTO, workspace=False)   # resident: no workspace needed
        assert (rc_res, rc_auto) == (0, 0)
        _same_bits(res, auto)
        _check_frame(res, 0, img, 0, pct, g_info, coords, want=_want_v2(name))
    for name in ("checker_127x126", "row_16001x1"):                # the first frames past it
        img, pct, g_info, coords = gold[name]
        rc_glb, glb = _launch(rdf, img[None], 0, pct, GLOBAL)
        rc_auto, auto = _launch(rdf, img[None], 0, pct, AUTO)
        assert (rc_glb, rc_auto) == (0, 0)
        _same_bits(glb, auto)
        _check_frame(auto, 0, img, 0, pct, g_info, coords, want=_want_v2(name))
        rc, untouched = _launch(rdf, img[None], 0, pct, RESIDENT)
        assert rc == BAD
        rc2, untouched2 = _launch(rdf, img[None], 0, pct, AUTO, workspace=False)
        assert rc2 == NULL
        for out in (untouched, untouched2):                         # a refused call writes nothing
            assert (out[0] == 7).all() and np.isnan(out[1]).all() and (out[2] == -5).all() and (out[3] == -9).all()


@pytest.mark.gpu
@pytest.mark.parametrize("path", [RESIDENT, GLOBAL])
def test_a_batch_of_hard_frames(path, rdf, gpu_runtime):
    names = ["serpentine_160x100", "checker_160x100", "full_160x100", "empty_160x100", "two_serpentines_160x100"]
    gold = _golden_v2()
    depth = np.stack([gold[n][0] for n in names])
    pct = -1.0                                                      # the checkerboard's; the others keep every component
    got = _run(rdf, depth, 0, pct, path)
    for i, n in enumerate(names):
        img, own_pct, g_info, coords = gold[n]
        comps = _want_v2(n)[2]
        sizes = np.unique(comps[comps >= 0], return_counts=True)[1]
        assert (sizes.astype(np.float32) / np.float32(16000) > np.float32(own_pct)).all()   # so the fixture holds at -1 too
        _check_frame(got, i, img, 0, pct, g_info, coords)
    e = names.index("empty_160x100")
    assert not got[0][e].any() and not got[1][e].view(np.uint32).any()
    assert (got[2][e] == -1).all() and (got[3][e] == -9).all()
    _same_bits(got, _run(rdf, depth, 0, pct, path))


def _embed(pattern, level):
    """The largest depth frame that still shrinks to `pattern` at `level`: pixel (y << level, x << level) carries the
    pattern, every other pixel is its block's opposite (nonzero where the pattern is 0, 0 where it is not); the rows and
    columns past the last block take the opposite of the last block."""
    hm, wm = pattern.shape
    f = 1 << level
    h, w = (hm << level) + f - 1, (wm << level) + f - 1
    ys, xs = np.minimum(np.arange(h) >> level, hm - 1), np.minimum(np.arange(w) >> level, wm - 1)
    depth = np.where(pattern[np.ix_(ys, xs)] != 0, 0, 1234).astype(np.uint16)
    depth[:hm * f:f, :wm * f:f] = pattern
    return depth


@pytest.mark.gpu
@pytest.mark.parametrize("level", [1, 3])
@pytest.mark.parametrize("name", ["two_serpentines_160x100", "border_lines_100x90"])
def test_fused_shrink_samples_only_its_own_pixels(name, level, rdf, gpu_runtime):
    img, pct, g_info, coords = _golden_v2()[name]
    depth = _embed(img, level)
    assert depth.shape == ((img.shape[0] << level) + (1 << level) - 1, (img.shape[1] << level) + (1 << level) - 1)
    assert np.array_equal(gnp.shrink(depth, level), img)
    f = 1 << level
    hm, wm = img.shape
    block = np.kron(img != 0, np.ones((f, f), bool))               # each pixel's block's pattern
    sampled = np.zeros(block.shape, bool)
    sampled[::f, ::f] = True
    assert ((depth[:hm * f, :wm * f] != 0) != block)[~sampled].all()   # every pixel the shrink skips is the opposite
    assert (depth[hm * f:] != 0).any() and (depth[:, wm * f:] != 0).any()
    want = _want_v2(name)                                           # the level-0 result of the bare pattern
    first = None
    for path in _paths_for(img):
        got = _run(rdf, depth[None], level, pct, path)
        _check_frame(got, 0, depth, level, pct, g_info, coords, want=want)
        if first is not None:
            _same_bits(first, got)
        first = got


@pytest.mark.gpu
@pytest.mark.parametrize("path", [AUTO, RESIDENT, GLOBAL])
def test_a_level_that_leaves_no_pixels(path, rdf, gpu_runtime):
    depth = np.full((2, 8, 8), 500, np.uint16)                     # level 4: Hm = Wm = 0
    rc, (groups, g_info, comps, coords) = _launch(rdf, depth, 4, 0.06, path)
    assert rc == 0
    assert g_info.shape == (2, 2, 3) and not g_info.view(np.uint32).any()
    assert (groups == 7).all() and (comps == -5).all() and (coords == -9).all()   # the one-element stand-ins: untouched


@pytest.mark.gpu
def test_cpp_grouping_drop_in_on_the_hard_shapes(rdf, gpu_runtime):
    cg = importlib.import_module("3d-beats_amd.cpp_grouping").CppGrouping()
    gold = _golden_v2()
    for name in ("checker_160x100", "comb_200x150", "row_16001x1"):   # one object: resident, then larger buffers, then global
        img, pct, ref_gi, ref_coords = gold[name]
        coords = np.full((img.size, 3), -9, np.int32)
        g_info = np.full((2, 3), np.nan, np.float32)
        cg.make_groups(img, coords, g_info, pct)
        assert np.array_equal(g_info.view(np.uint32), ref_gi.view(np.uint32)), name
        rows = _want_v2(name)[3]
        assert len(rows) == len(ref_coords) and np.array_equal(coords[:len(rows)], rows), name
        assert (coords[len(rows):] == -9).all(), name
        assert np.array_equal(_rows(coords[:len(rows)]), _rows(ref_coords)), name
