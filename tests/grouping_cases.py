"""Shrunk frames that are hard for rdf_hand_groups: components that cross every 16x16 tile of the global path, root chains
thousands of links long, thousands of equal-size bidders for a side's key, and frames at and just past the resident path's
limit of 16000 pixels.  Data only: tests/golden/make_grouping_golden.py records the reference's grouping.cpp on these cases
into tests/golden/grouping_v2.npz and tests/test_grouping.py runs the device paths on them.

Every case is (name, image uint16 [Hm, Wm], pct).  The sizes are the smallest at which each thing can still go wrong.  No
builder draws random numbers, so appending a case never changes an earlier one; the order below is the fixture's order."""
import numpy as np

RESIDENT_MAX_PIXELS = 16000          # kResMaxPixels of csrc/grouping_hip.hip
TILE = 16                            # kTile


def _img(hm, wm):
    return np.zeros((hm, wm), np.uint16)


def _serpentine(hm, wm, x0, x1, v):
    """Even rows full over columns [x0, x1]; odd rows hold one connector, alternately in the last and the first column."""
    img = _img(hm, wm)
    img[::2, x0:x1 + 1] = v
    img[1::4, x1] = v
    img[3::4, x0] = v
    return img


def serpentine_160x100():
    return _serpentine(100, 160, 0, 159, 6)          # one path of 50 * 160 + 50 = 8050 px through every tile, P = 16000


def two_serpentines_160x100():
    img = _serpentine(100, 160, 0, 78, 6) | _serpentine(100, 160, 81, 159, 9)
    assert not img[:, 79:81].any()                   # columns 79-80 stay clear: 4000 px on each side
    return img


def _checker(hm, wm):
    return ((np.indices((hm, wm)).sum(0) % 2) == 0).astype(np.uint16) * 3     # foreground at (0, 0)


def checker_160x100():
    return _checker(100, 160)                        # 8000 one-pixel components = ceil(P / 2) stats slots


def checker_125x127():
    return _checker(127, 125)                        # odd P = 15875, (P + 1) / 2 = 7938 components


def spiral_121():
    n = 121
    img = _img(n, n)
    for o in range(0, n, 2):                         # square rings, each opened at its top-left and bridged inwards
        e = n - 1 - o
        if e - o < 2:
            break
        img[o, o:e + 1] = img[o:e + 1, e] = img[e, o:e + 1] = 1
        img[o + 2:e + 1, o] = 1
        if e - o >= 6:
            img[o + 2, o + 1] = 1
    return img


def staircase_130x120():
    img = _img(120, 130)
    i = np.arange(120)
    img[i, i] = img[i, i + 1] = 5                    # crosses the tile borders at the tiles' corners
    return img


def border_lines_100x90():
    """Rows 15::16 (the last row of a tile row) and columns 16::16 (the first column of a tile column): every line pixel
    sits on a tile border, and each crossing (r, c) is where a left-border union and an up-border union meet.  Every third
    crossing is cut, which splits the grid of lines into several components."""
    img = _img(90, 100)
    img[TILE - 1::TILE, :] = 4
    img[:, TILE::TILE] = 4
    for a, r in enumerate(range(TILE - 1, 90, TILE)):
        for b, c in enumerate(range(TILE, 100, TILE)):
            if (a + 2 * b) % 3 == 0:
                img[r, c] = 0
    return img


def corner_touch_100x90():
    img = _img(90, 100)
    for k in range(TILE - 1, 89, TILE):              # k = 15, 31, 47, 63, 79
        img[k, k] = img[k + 1, k + 1] = 2            # diagonal neighbours across a tile corner: never one component
    return img


def full_160x100():
    return np.full((100, 160), 11, np.uint16)


def empty_160x100():
    return _img(100, 160)


def checker_127x126():
    return _checker(126, 127)                        # P = 16002: the first even-sided frame past the resident limit


def row_16001x1():
    img = np.resize(np.array([1, 1, 1, 0, 1, 0, 0], np.uint16), 16001).reshape(1, 16001)
    return np.ascontiguousarray(img)                 # a 1001 x 1 tile grid: left-border unions only


def column_1x4099():
    return np.full((4099, 1), 8, np.uint16)          # up-border unions only


def comb_200x150():
    img = _img(150, 200)
    img[:, ::2] = 4
    img[-1, :] = 4                                   # teeth joined at the bottom: roots are found through the last tile row
    return img


def comb_upside_down_200x150():
    return np.ascontiguousarray(comb_200x150()[::-1])


def _sums(mask):
    ys, xs = np.nonzero(mask)
    return len(ys), int(xs.sum()), int(ys.sum())


def large_sums_400x300():
    """One component per side, each of more than 40 000 px, with every coordinate sum odd: none of the four quotients
    (float)sum / (float)size is exact.  sum_x of the right component is above 2^24, so there the conversion to fp32 before
    the divide rounds as well.  (With two components of more than 40 000 px each in 400 x 300, neither sum_y nor the left
    sum_x can reach 2^24: a component of at most 80 000 px has sum_y <= 15 960 000, and a left component with
    sum_x > 2^24 needs more than 83 886 px.  large_sums_one_side_400x300 covers those.)"""
    img = _img(300, 400)
    img[:, :199] = 600
    img[0, 197] = img[299, 0] = 0                    # one odd x and one odd y less: both sums odd
    img[:, 200:] = 900
    img[0, 399] = img[299, 398] = 0
    (nl, sxl, syl), (nr, sxr, syr) = _sums(img[:, :199] != 0), _sums(img[:, 200:] != 0)
    sxr += 200 * nr
    assert nl > 40000 and nr > 40000
    assert sxl % 2 == 1 and syl % 2 == 1 and sxr % 2 == 1 and syr % 2 == 1
    assert sxr > 1 << 24 and sxl // nl < 200 <= sxr // nr
    return img


def large_sums_one_side_400x300():
    """One component of nearly the whole frame whose centroid stays left of the middle: sum_x and sum_y are both odd and
    above 2^24, so both int -> fp32 conversions round before the divide."""
    img = np.full((300, 400), 700, np.uint16)
    img[0, 399] = img[299, 398] = 0                  # one odd x and one odd y less
    n, sx, sy = _sums(img != 0)
    assert sx % 2 == 1 and sy % 2 == 1 and sx > 1 << 24 and sy > 1 << 24
    assert int(np.float32(sx)) != sx and int(np.float32(sy)) != sy and sx / n < 200
    return img


_CASES = (
    (serpentine_160x100, 0.06), (two_serpentines_160x100, 0.06), (checker_160x100, -1.0), (checker_125x127, -1.0),
    (spiral_121, 0.06), (staircase_130x120, 0.0), (border_lines_100x90, 0.0), (corner_touch_100x90, -1.0),
    (full_160x100, 0.06), (empty_160x100, 0.06),
    (checker_127x126, -1.0), (row_16001x1, 0.0), (column_1x4099, 0.0), (comb_200x150, 0.06),
    (comb_upside_down_200x150, 0.06), (large_sums_400x300, 0.06), (large_sums_one_side_400x300, 0.06),
)
NAMES = tuple(f.__name__ for f, _ in _CASES)
WITHOUT_COORDS = ("large_sums_400x300", "large_sums_one_side_400x300")   # g_info only: the coordinate list would fill the file


def cases():
    return [(f.__name__, np.ascontiguousarray(f(), np.uint16), pct) for f, pct in _CASES]


def fits_resident(img):
    return img.size <= RESIDENT_MAX_PIXELS
