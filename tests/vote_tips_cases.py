"""The cases of tests/test_vote_tips.py: hand-made inputs of rdf_labels_vote_tips (rules T of include/rdf_labels.h) that the CPU
tests and the GPU tests both build, so that both see the same arrays.

  kernel_case()   3 frames of 13 x 9 (dim_x x dim_y), labels_reduce 2, L = 6 classes, 5 tips, 6 joints.  Frames 0 and 1 are
                  written out below tip by tip; frame 2 is drawn.  RUNS lists the (flip, policy, max_dist, z_tol) the device
                  test makes.
  sweep_case()    300 frames of 8 x 8 with 5 tips: 1500 (frame, tip) pairs, more than the 1024 lanes of one sweep of k_vote_tips.

13 is odd: the mirror of pixel p is 12 - p and pixel 6 is its own mirror, so a case placed symmetrically about column 6 is met
with both flips.
"""
import itertools

import numpy as np

import vote_tips_numpy as tn

W, H, R, L, J = 13, 9, 2, 6, 6
INTR = (11.5, 12.25, 6.3, 4.1)                              # fx, fy, ppx, ppy
CLASS_IDS = (1, 2, 3, 9, 5)                                 # 9 names no class
TIP_JOINTS = (0, 1, 2, 3, -1)                               # the last tip never takes a vote
SENTINEL = 7.0
STRIDE = 7                                                  # heights_stride > n_ids: two sentinels a row
SWEEP_LANES = 4 * 256                                       # vote_tips_hip.hip: kMaxBlocks x kThreads

# (flip_x, policy, max_dist, z_tol).  Frame 0's tip 0 has its mode 2 pixels from its vote along x and the sensor 5 units from
# the voted depth: max_dist 2 and 1, z_tol 5 and 4 are the distance / the difference and one below.
RUNS = tuple((flip, policy, 2, 5) for flip in (0, 1) for policy in (tn.FILL, tn.GUARD, tn.VOTES)) + tuple(
    (flip, policy, md, zt) for flip in (0, 1) for policy in (tn.GUARD, tn.VOTES) for md, zt in ((1, 5), (2, 4)))


def plane():
    p = np.eye(4, dtype=np.float64)
    p[2] = (0.11, -0.43, 0.89, -512.25)                     # a tilted table: every term of T5 matters
    return p.astype(np.float32)


def centre(p):
    """X (or Y) of rule V5 for the centre of pixel p."""
    return 16 * p + 8


def kernel_case():
    """(means float64 [3, 6, 2], joints int32 [3, 6, 4], depth uint16 [3, 9, 13]).

    Frame 0.
      tip 0  class 1, mean (3.7, 2.2) -> mode pixel (6, 4), depth 650.  Joint 0 at the centre of pixel (8, 5), Z 705, support
             9: unflipped the vote's pixel is (8, 5), flipped (4, 5); both 2 from the mode along x and 1 along y: 2, not 3.
             depth[5][8] = 700 and depth[5][4] = 710: |zs - Z| = 5.  GUARD at max_dist 2: the mode; at 1: the vote.  z_tol 5: source 2; 4: source 3.
      tip 1  class 2, mean NaN: no mode.  Joint 1 at pixel (2, 1) / (10, 1), where the depth is 0: source 3, z = Z = 3 (within z_tol of 0: a hole is
             never taken).
      tip 2  class 3, mean (7.0, 1.0) -> pixel (14, 2): off the frame.  Joint 2 at pixel (3, 7) / (9, 7), depth 65535, Z 65533:
             source 3.
      tip 3  class 9: no class.  Joint 3 has support 0: neither candidate, NaN, (-1, -1, 0, 0).
      tip 4  class 5, mean (1.2, 3.9) -> pixel (2, 6), depth 0 taken as it is.  tip_joints -1: the mode under every policy.
    Frame 1.
      tip 0  class 1, mean (0.5, 0.5) -> pixel (0, 0).  Joint 0 at X = -40, Y = 147: floordiv gives (-3, 9); unflipped x clamps
             to 0, flipped Xu = 248 -> 15 clamps to 12; y clamps to 8.
      tip 1  class 2, mean (-1.5, 2.0) -> trunc -1 -> pixel (-2, 4): off the frame.  Joint 1 at X = 213, Y = -3: (13, -1);
             unflipped x clamps to 12, flipped Xu = -5 -> -1 clamps to 0; y clamps to 0.
      tip 2  class 3, mean (5.99, 3.99) -> pixel (10, 6), depth 65535 taken as it is.  Joint 2 at pixel (6, 2) (its own mirror),
             Z = the depth there: source 2 at any z_tol.
      tip 3  class 9.  Joint 3 at pixel (1, 5) / (11, 5), Z 800: the depth is 803 unflipped (source 2) and 740 flipped (source 3).
      tip 4  class 5, mean (1e9, 1.0): no mode; no vote either: NaN.
    Frame 2: drawn means and joints; class 2's mean is +inf, class 3's just below 1e9 (off the frame), class 1's (-0.6, 2.5)
    -> trunc gives pixel (0, 4), class 5's (6.4, 4.3) -> pixel (12, 8), the last column and row."""
    rng = np.random.default_rng(1307)
    depth = rng.integers(520, 900, (3, H, W)).astype(np.uint16)
    means = np.zeros((3, L, 2), np.float64)
    joints = np.zeros((3, J, 4), np.int32)
    joints[:] = (-1, -1, 0, 0)
    nan = float("nan")
    # frame 0
    means[0] = [(3.7, 2.2), (nan, 1.0), (7.0, 1.0), (2.0, 2.0), (1.2, 3.9), (0.0, 0.0)]
    depth[0, 4, 6], depth[0, 5, 8], depth[0, 5, 4] = 650, 700, 710
    joints[0, 0] = (centre(8), centre(5), 705, 9)
    depth[0, 1, 2] = depth[0, 1, 10] = 0
    joints[0, 1] = (centre(2), centre(1), 3, 3)
    depth[0, 7, 3] = depth[0, 7, 9] = 65535
    joints[0, 2] = (centre(3), centre(7), 65533, 1)
    joints[0, 3] = (centre(5), centre(5), 600, 0)
    depth[0, 6, 2] = 0
    # frame 1
    means[1] = [(0.5, 0.5), (-1.5, 2.0), (5.99, 3.99), (1.0, 1.0), (1e9, 1.0), (3.0, 3.0)]
    joints[1, 0] = (-40, 16 * 9 + 3, 610, 2)
    joints[1, 1] = (16 * 13 + 5, -3, 620, 2)
    depth[1, 6, 10] = 65535
    joints[1, 2] = (centre(6), centre(2), int(depth[1, 2, 6]), 40)
    depth[1, 5, 1], depth[1, 5, 11] = 803, 740
    joints[1, 3] = (centre(1), centre(5), 800, 2 ** 31 - 1)
    # frame 2
    means[2] = rng.uniform(-0.5, 6.9, (L, 2))
    means[2, 1] = (float("inf"), 2.0)
    means[2, 2] = (999999999.5, 1.0)
    means[2, 0] = (-0.6, 2.5)                               # truncates onto column 0; floored it is off the frame
    means[2, 4] = (6.4, 4.3)                                # the last column and the last row
    joints[2, :, 0] = rng.integers(-30, 16 * W + 30, J)
    joints[2, :, 1] = rng.integers(-30, 16 * H + 30, J)
    joints[2, :, 2] = rng.integers(515, 905, J)
    joints[2, :, 3] = (5, 0, 7, 1, -4, 9)
    for a in (means, joints, depth):
        a.setflags(write=False)
    return means, joints, depth


def run(mod, case, flip, policy, max_dist, z_tol, stride=None):
    means, joints, depth = case
    heights = None if stride is None else np.full((means.shape[0], stride), SENTINEL)
    return mod.vote_tips(means, CLASS_IDS, TIP_JOINTS, joints, flip, depth, R, INTR, plane(), policy, max_dist, z_tol, heights, stride)


SWEEP = dict(n=300, W=8, H=8, r=2, L=5, J=5, seed=29)
SWEEP_IDS = (1, 2, 3, 4, 5)
SWEEP_JOINTS = (4, 3, 2, 1, 0)


def sweep_case():
    """(means [300, 5, 2], joints [300, 5, 4], depth [300, 8, 8]): drawn; about a tenth of the means NaN, a fifth off the frame,
    a fifth of the joints without support, depths of 0 and 65535 sprinkled in, voted depths within a few units of the frame's."""
    m = SWEEP
    rng = np.random.default_rng(m["seed"])
    depth = rng.integers(600, 640, (m["n"], m["H"], m["W"])).astype(np.uint16)
    holes = rng.random(depth.shape)
    depth[holes < 0.1] = 0
    depth[holes > 0.9] = 65535
    means = rng.uniform(-0.9, 4.9, (m["n"], m["L"], 2))
    means[rng.random((m["n"], m["L"])) < 0.1] = float("nan")
    joints = np.zeros((m["n"], m["J"], 4), np.int32)
    joints[..., 0] = rng.integers(-20, 16 * m["W"] + 20, (m["n"], m["J"]))
    joints[..., 1] = rng.integers(-20, 16 * m["H"] + 20, (m["n"], m["J"]))
    joints[..., 2] = rng.integers(595, 645, (m["n"], m["J"]))
    joints[..., 3] = rng.integers(0, 5, (m["n"], m["J"]))
    for a in (means, joints, depth):
        a.setflags(write=False)
    return means, joints, depth


def run_sweep(mod, case, flip, policy):
    means, joints, depth = case
    return mod.vote_tips(means, SWEEP_IDS, SWEEP_JOINTS, joints, flip, depth, SWEEP["r"], INTR, plane(), policy, 3, 6)


SWEEP_RUNS = tuple(itertools.product((0, 1), (tn.FILL, tn.GUARD, tn.VOTES)))


# ------------------------------------------------------------ mutants ---------------------------------------------------------
# Wrong readings of rules T that a kernel could make (tests/mutants.py): every one must change what the device test of
# kernel_case() compares, under at least one of RUNS.
EDITS = {
    # T1
    "mode floored, not truncated": [("px, py = int(mx) * r, int(my) * r", "px, py = int(np.floor(mx)) * r, int(np.floor(my)) * r")],
    "mode scaled before the truncation": [("px, py = int(mx) * r, int(my) * r", "px, py = int(mx * r), int(my * r)")],
    "the last column and row are off the frame": [("px >= dim_x or py >= dim_y", "px >= dim_x - 1 or py >= dim_y - 1")],
    # (not here: |.| > 1e9 for >= 1e9 -- 1e9 itself is off every frame of at most 65535 pixels, so no input tells the two apart)
    # T2
    "support 0 votes": [("if S <= 0 or", "if S < 0 or")],
    "flip mirrors the pixel index of the left edge": [("return 16 * int(dim_x) - int(X)", "return 16 * (int(dim_x) - 1) - int(X)")],
    "flip forgotten": [("Xu = flipped(X, dim_x) if flip_x else X", "Xu = X")],
    # (not here: a quotient truncated towards 0 -- it differs from the floor only below 0, where both clamp to 0)
    "no vote past the frame instead of a clamp": [("    Xu = flipped(X, dim_x) if flip_x else X\n",
                                                   "    Xu = flipped(X, dim_x) if flip_x else X\n    if not (0 <= Xu // 16 < dim_x and 0 <= Y // 16 < dim_y):\n        return None\n")],
    # T3
    "fill prefers the vote": [('    if policy == FILL:\n        return "mode"', '    if policy == FILL:\n        return "vote"')],
    "votes prefers the mode": [('    if policy == VOTES:\n        return "vote"', '    if policy == VOTES:\n        return "mode"')],
    "guard <": [("<= max_dist else", "< max_dist else")],
    "guard along x only": [("max(abs(mode[0] - vote[0]), abs(mode[1] - vote[1]))", "abs(mode[0] - vote[0])")],
    "guard by the sum of the distances": [("max(abs(mode[0] - vote[0]), abs(mode[1] - vote[1]))", "(abs(mode[0] - vote[0]) + abs(mode[1] - vote[1]))")],
    # T4
    "z_tol <": [("abs(zs - Z) <= z_tol", "abs(zs - Z) < z_tol")],
    "a hole of 0 taken": [("if zs != 0 and zs != 65535 and", "if zs != 65535 and")],
    "65535 taken": [("if zs != 0 and zs != 65535 and", "if zs != 0 and")],
    "a mode on a hole gives no height": [('                elif which == "mode":\n                    px, py = mode\n                    z = int(depth[f, py, px])\n',
                                         '                elif which == "mode" and int(depth[f, mode[1], mode[0]]) in (0, 65535):\n                    out[f, i], tips[f, i] = np.nan, NONE\n'
                                         '                elif which == "mode":\n                    px, py = mode\n                    z = int(depth[f, py, px])\n')],
    "the voted depth always": [("        return zs, 2\n", "        return Z, 2\n")],
    # T5
    "deprojection in fp64": [("    x = (np.float32(px) - ppx) / fx\n", "    x = np.float64(px - np.float64(ppx)) / np.float64(fx)\n")],
    "the plane's row summed from the last term": [("for k in range(4):\n        pz = pz +", "for k in (3, 2, 1, 0):\n        pz = pz +")],
    "height not negated": [("    return -pz\n", "    return pz\n")],
}


def mutant(name):
    import mutants
    return mutants.load("vote_tips_numpy", EDITS[name])


def device_outputs(mod):
    """What test_the_kernel_against_the_restatement compares, under restatement `mod`."""
    case = kernel_case()
    out = []
    with np.errstate(all="ignore"):
        for r in RUNS:
            out += list(run(mod, case, *r))
        out += list(run(mod, case, 1, tn.VOTES, 2, 5, stride=STRIDE))
    return out
