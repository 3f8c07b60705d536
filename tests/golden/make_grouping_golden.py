#!/usr/bin/env python3
"""Records what the reference's own hand grouping (src/cpp_grouping/grouping.cpp, `CppGrouping::make_groups`) computes on a
set of shrunk frames into tests/golden/grouping_v1.npz, and on the tile-crossing and limit-sized frames of tests/grouping_cases.py
into tests/golden/grouping_v2.npz.  grouping.cpp is the one piece of the reference that runs on a CPU, so
rdf_hand_groups' components, sizes, centroids and selection are pinned to the reference's code, not to a restatement.

Runs in the build container only (it needs /root/reference, which never travels to the GPU box): grouping.cpp is compiled
with g++ -O2 into a temporary directory together with this script's own three-line extern "C" driver; nothing of the
reference is copied.  g_info is zero-filled before every call; for a side without a winner only the size (0) is recorded,
since the reference leaves that side's centroid uninitialised.  The fixtures hold data only.  grouping_v2.npz has the layout
of grouping_v1.npz; a case named in grouping_cases.WITHOUT_COORDS keeps its g_info only (its breadth-first coordinate list
would be most of the file): its `coords` has no rows and `<name>/has_coords` is False.

    python3 tests/golden/make_grouping_golden.py        # rewrites tests/golden/grouping_v1.npz and grouping_v2.npz
"""
import ctypes
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import grouping_cases  # noqa: E402
REF = "/root/reference/src/cpp_grouping"

DRIVER = r'''
#include "grouping.h"
extern "C" void drive(void *img, int dim_x, int dim_y, void *coords, void *g_info, float pct) {
    CppGrouping g; g.make_groups(img, dim_x, dim_y, coords, g_info, pct);
}
'''


def _build(tmp):
    drv = os.path.join(tmp, "driver.cpp")
    with open(drv, "w") as f:
        f.write(DRIVER)
    so = os.path.join(tmp, "libgrouping_ref.so")
    subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-I", REF, "-o", so, os.path.join(REF, "grouping.cpp"), drv])
    lib = ctypes.CDLL(so)
    lib.drive.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_float]
    lib.drive.restype = None
    return lib


def _blobs(rng, hm, wm, k):
    img = np.zeros((hm, wm), np.uint16)
    yy, xx = np.mgrid[:hm, :wm]
    for _ in range(k):
        cy, cx = rng.uniform(0, hm), rng.uniform(0, wm)
        ry, rx = rng.uniform(1, hm / 3 + 1), rng.uniform(1, wm / 3 + 1)
        img[((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1] = rng.integers(300, 1500)
    img[rng.random((hm, wm)) < 0.05] = 0          # holes
    img[rng.random((hm, wm)) < 0.02] = 700        # specks
    return img


def _two_hands(rng, hm, wm):
    img = np.zeros((hm, wm), np.uint16)
    yy, xx = np.mgrid[:hm, :wm]
    for cx in (wm * 0.28, wm * 0.7):
        cy = hm * rng.uniform(0.4, 0.6)
        m = ((yy - cy) / (hm * 0.22)) ** 2 + ((xx - cx) / (wm * 0.12)) ** 2 <= 1
        for k in range(5):                          # fingers
            fx = cx + (k - 2) * wm * 0.035
            m |= (np.abs(xx - fx) < max(1, wm * 0.01)) & (yy > cy - hm * 0.45) & (yy < cy)
        img[m] = rng.integers(400, 900)
    img[rng.random((hm, wm)) < 0.03] = 0
    img[rng.random((hm, wm)) < 0.01] = 650
    return img


def cases():
    rng = np.random.default_rng(20261016)
    out = []
    toy = np.ones((6, 8), np.uint16)
    toy[3, :] = 0
    toy[:, 4] = 0
    toy[5, :] = 2
    out.append(("toy", toy, 0.05))
    out.append(("all_zero", np.zeros((9, 13), np.uint16), 0.06))
    out.append(("all_nonzero", np.full((7, 10), 5, np.uint16), 0.06))
    sp = np.zeros((8, 10), np.uint16)
    sp[1, 2] = sp[5, 7] = sp[7, 0] = 3
    out.append(("single_pixels", sp, -1.0))
    out.append(("single_pixel_1x1", np.ones((1, 1), np.uint16), 0.5))
    diag = np.zeros((12, 12), np.uint16)
    for i in range(12):
        diag[i, i] = 9
        diag[i, 11 - i] = 9
    out.append(("diagonal_only", diag, -1.0))
    cb = ((np.indices((10, 11)).sum(0) % 2) == 0).astype(np.uint16)
    out.append(("checkerboard", cb, -1.0))
    n = 21
    spiral = np.zeros((n, n), np.uint16)
    for o in range(0, n, 2):                          # square rings, each opened at its top-left and bridged inwards
        e = n - 1 - o
        if e - o < 2:
            break
        spiral[o, o:e + 1] = spiral[o:e + 1, e] = spiral[e, o:e + 1] = 1
        spiral[o + 2:e + 1, o] = 1
        if e - o >= 6:
            spiral[o + 2, o + 1] = 1
    snake = np.zeros((15, 30), np.uint16)
    snake[::2, :] = 6
    snake[1::4, -1] = 6
    snake[3::4, 0] = 6                                # one serpentine path
    out.append(("snake", snake, 0.06))
    out.append(("spiral", spiral, 0.06))
    comb = np.zeros((16, 33), np.uint16)
    comb[15, :] = 4
    comb[:, ::2] = 4                                  # teeth joined at the bottom: long merge chains
    out.append(("comb", comb, 0.06))
    comb_up = comb[::-1].copy()
    out.append(("comb_upside_down", comb_up, 0.06))
    u = np.zeros((20, 24), np.uint16)
    u[2:18, 3:6] = u[2:18, 18:21] = u[15:18, 3:21] = 8
    u[4:12, 9:15] = 8
    out.append(("u_shape", u, 0.01))
    ring = np.zeros((9, 14), np.uint16)
    ring[0, :] = ring[-1, :] = ring[:, 0] = ring[:, -1] = 2
    ring[4, 5:9] = 2
    out.append(("border_ring", ring, 0.02))
    tie = np.zeros((10, 20), np.uint16)
    tie[1:4, 1:4] = 1
    tie[6:9, 5:8] = 1                                 # equal sizes on the left: the first met wins
    tie[1:3, 12:16] = 1
    tie[5:7, 14:18] = 1                               # and on the right
    out.append(("tie_break", tie, 0.01))
    tie2 = np.zeros((10, 20), np.uint16)
    tie2[6:9, 1:4] = 1
    tie2[1:4, 5:8] = 1
    out.append(("tie_break_upper_first", tie2, 0.01))
    half = np.zeros((6, 10), np.uint16)
    half[1:4, 3:8] = 1                                # c_x = 5 = Wm / 2: group 2
    out.append(("centroid_at_half", half, 0.0))
    half_odd = np.zeros((6, 11), np.uint16)
    half_odd[1:4, 4:7] = 1                            # c_x = 5 < 5.5: group 1
    half_odd[5, 6:11] = 1
    out.append(("odd_width", half_odd, 0.0))
    k = np.zeros((10, 10), np.uint16)
    k[1:3, 1:4] = 1                                   # size 6 of 100
    k[6:9, 6:9] = 1                                   # size 9
    out.append(("size_at_threshold", k, float(np.float32(6) / np.float32(100))))
    out.append(("size_above_threshold", k, float(np.float32(5) / np.float32(100))))
    out.append(("threshold_negative", _blobs(rng, 15, 21, 4), -0.5))
    out.append(("threshold_one", _blobs(rng, 15, 21, 4), 1.0))
    out.append(("threshold_above_one", np.full((4, 4), 3, np.uint16), 1.5))
    col = np.zeros((17, 1), np.uint16)
    col[2:9, 0] = col[11:14, 0] = 1
    out.append(("width_1", col, 0.0))
    row = np.zeros((1, 19), np.uint16)
    row[0, 1:7] = row[0, 9:18] = 1
    out.append(("height_1", row, 0.0))
    out.append(("hands_106x60", _two_hands(rng, 60, 106), 0.06))
    out.append(("hands_160x90", _two_hands(rng, 90, 160), 0.06))
    out.append(("hands_106x60_b", _two_hands(rng, 60, 106), 0.06))
    for i in range(8):
        hm, wm = int(rng.integers(5, 70)), int(rng.integers(5, 120))
        out.append((f"blobs_{i}", _blobs(rng, hm, wm, int(rng.integers(1, 8))), float(rng.choice([0.0, 0.01, 0.06]))))
    return out


def _record(lib, img, pct):
    """(g_info float32 [2, 3], coords int32 [n1 + n2, 3]) of the reference's make_groups on one shrunk frame."""
    hm, wm = img.shape
    coords = np.zeros((max(hm * wm, 1), 3), np.int32)
    g_info = np.zeros((2, 3), np.float32)
    lib.drive(img.ctypes.data, wm, hm, coords.ctypes.data, g_info.ctypes.data, ctypes.c_float(pct))
    n1, n2 = int(g_info[0, 0]), int(g_info[1, 0])
    for side, n in ((0, n1), (1, n2)):
        if n == 0:
            g_info[side, 1:] = 0.0                         # uninitialised in the reference: not recorded
    return g_info, coords[:n1 + n2].copy()


def record_v2(lib):
    data = {}
    names = []
    for name, img, pct in grouping_cases.cases():
        g_info, coords = _record(lib, img, pct)
        names.append(name)
        data[f"{name}/img"] = img
        data[f"{name}/pct"] = np.float32(pct)
        data[f"{name}/g_info"] = g_info
        if name in grouping_cases.WITHOUT_COORDS:
            coords = coords[:0]
            data[f"{name}/has_coords"] = np.bool_(False)
        data[f"{name}/coords"] = coords
    data["names"] = np.array(names)
    return data


def main():
    with tempfile.TemporaryDirectory() as tmp:
        lib = _build(tmp)
        data = {}
        names = []
        for name, img, pct in cases():
            img = np.ascontiguousarray(img, np.uint16)
            hm, wm = img.shape
            coords = np.zeros((hm * wm, 3), np.int32)
            g_info = np.zeros((2, 3), np.float32)
            lib.drive(img.ctypes.data, wm, hm, coords.ctypes.data, g_info.ctypes.data, ctypes.c_float(pct))
            n1, n2 = int(g_info[0, 0]), int(g_info[1, 0])
            for side, n in ((0, n1), (1, n2)):
                if n == 0:
                    g_info[side, 1:] = 0.0                 # uninitialised in the reference: not recorded
            names.append(name)
            data[f"{name}/img"] = img
            data[f"{name}/pct"] = np.float32(pct)
            data[f"{name}/g_info"] = g_info
            data[f"{name}/coords"] = coords[:n1 + n2].copy()
        data["names"] = np.array(names)
        data_v2 = record_v2(lib)
    path = os.path.join(HERE, "grouping_v1.npz")
    np.savez_compressed(path, **data)
    print(f"{path}: {len(names)} cases, {os.path.getsize(path)} bytes")
    path = os.path.join(HERE, "grouping_v2.npz")
    np.savez_compressed(path, **data_v2)
    print(f"{path}: {len(data_v2['names'])} cases, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    sys.exit(main())
