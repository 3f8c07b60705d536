"""Rules T of include/rdf_labels.h (rdf_labels_vote_tips) restated with Python integers and numpy fp32 / fp64, one (frame, tip)
pair at a time, bit for bit:

  T1 mode candidate   c = class_ids[i] in 1..L, (mx, my) = means[f][c - 1] not NaN and |.| < 1e9, (pxm, pym) = (trunc(mx) r,
                      trunc(my) r) on the frame.
  T2 vote candidate   j = tip_joints[i] in 0..J - 1, (X, Y, Z, S) = joints[f][j] with S > 0, a frame with pixels;
                      Xu = 16 dim_x - X when flipped; (pxv, pyv) = (clamp(Xu // 16, 0, dim_x - 1), clamp(Y // 16, 0, dim_y - 1)).
  T3 choice           FILL: mode, else vote.  GUARD: both: the mode if max(|pxm - pxv|, |pym - pyv|) <= max_dist, else the vote;
                      one: that one.  VOTES: vote, else mode.  Neither: NaN and (-1, -1, 0, 0).
  T4 depth            mode: z = depth[pym][pxm] as it is, source 1.  vote: zs = depth[pyv][pxv]; zs not 0, not 65535 and
                      |zs - Z| <= z_tol: z = zs, source 2; else z = Z, source 3.
  T5 height           x = (fp32(px) - ppx) / fx, y alike, pt = (fp64(fp32(z) x), fp64(fp32(z) y), fp64(fp32(z)), 1),
                      height = -(((0 + p8 pt0) + p9 pt1) + p10 pt2) + p11 pt3) with the plane's third row promoted to fp64.
"""
import numpy as np

FILL, GUARD, VOTES = 0, 1, 2
POLICIES = {"fill": FILL, "guard": GUARD, "votes": VOTES}
NONE = (-1, -1, 0, 0)


def mode_candidate(mx, my, r, dim_x, dim_y):
    """T1 without the class test: (pxm, pym) or None."""
    mx, my = float(mx), float(my)
    if mx != mx or my != my or abs(mx) >= 1e9 or abs(my) >= 1e9:
        return None
    px, py = int(mx) * r, int(my) * r                       # int() truncates towards 0
    if px < 0 or py < 0 or px >= dim_x or py >= dim_y:
        return None
    return px, py


def flipped(X, dim_x):
    return 16 * int(dim_x) - int(X)


def clamp(v, lo, hi):
    return lo if v < lo else (hi if v > hi else v)


def vote_candidate(joint, flip_x, dim_x, dim_y):
    """T2 without the joint test: (pxv, pyv, Z) or None."""
    X, Y, Z, S = (int(v) for v in joint)
    if S <= 0 or dim_x < 1 or dim_y < 1:
        return None
    Xu = flipped(X, dim_x) if flip_x else X
    return clamp(Xu // 16, 0, dim_x - 1), clamp(Y // 16, 0, dim_y - 1), Z


def choose(mode, vote, policy, max_dist):
    """T3: 'mode', 'vote' or None."""
    if mode is None or vote is None:
        return "mode" if mode is not None else ("vote" if vote is not None else None)
    if policy == FILL:
        return "mode"
    if policy == VOTES:
        return "vote"
    return "mode" if max(abs(mode[0] - vote[0]), abs(mode[1] - vote[1])) <= max_dist else "vote"


def vote_depth(zs, Z, z_tol):
    """T4 for a vote: (z, source)."""
    zs, Z = int(zs), int(Z)
    if zs != 0 and zs != 65535 and abs(zs - Z) <= z_tol:
        return zs, 2
    return Z, 3


def height_at(px, py, z, intrinsics, plane):
    """T5.  plane: float32 [4, 4] (or 16)."""
    fx, fy, ppx, ppy = (np.float32(v) for v in intrinsics)
    row = np.asarray(plane, np.float32).reshape(4, 4)[2]
    zf = np.float32(z)
    x = (np.float32(px) - ppx) / fx
    y = (np.float32(py) - ppy) / fy
    pt = (np.float64(zf * x), np.float64(zf * y), np.float64(zf), np.float64(1.0))
    pz = np.float64(0.0)
    for k in range(4):
        pz = pz + np.float64(row[k]) * pt[k]
    return -pz


def vote_tips(means, class_ids, tip_joints, joints, flip_x, depth, labels_reduce, intrinsics, plane, policy, max_dist, z_tol,
              heights=None, heights_stride=None):
    """means float64 [n, L, 2]; joints int32 [n, J, 4]; depth uint16 [n, H, W].  Returns (heights float64 [n, stride], tips int32
    [n, n_ids, 4]); `heights` given: written into (a copy of) it, what lies beyond n_ids in a row kept."""
    means = np.asarray(means, np.float64)
    joints = np.asarray(joints)
    n, L = means.shape[:2]
    J = joints.shape[1]
    H, W = depth.shape[1:]
    n_ids = len(class_ids)
    policy = POLICIES.get(policy, policy)
    stride = n_ids if heights_stride is None else int(heights_stride)
    out = np.full((n, stride), np.nan, np.float64) if heights is None else np.array(heights, np.float64).reshape(n, stride)
    tips = np.zeros((n, n_ids, 4), np.int32)
    with np.errstate(all="ignore"):
        for f in range(n):
            for i in range(n_ids):
                c, j = int(class_ids[i]), int(tip_joints[i])
                mode = mode_candidate(means[f, c - 1, 0], means[f, c - 1, 1], labels_reduce, W, H) if 1 <= c <= L else None
                vote = vote_candidate(joints[f, j], flip_x, W, H) if 0 <= j < J else None
                which = choose(mode, vote, policy, max_dist)
                if which is None:
                    out[f, i], tips[f, i] = np.nan, NONE
                elif which == "mode":
                    px, py = mode
                    z = int(depth[f, py, px])
                    out[f, i], tips[f, i] = height_at(px, py, z, intrinsics, plane), (px, py, z, 1)
                else:
                    px, py, Z = vote
                    z, source = vote_depth(depth[f, py, px], Z, z_tol)
                    out[f, i], tips[f, i] = height_at(px, py, z, intrinsics, plane), (px, py, z, source)
    return out, tips
