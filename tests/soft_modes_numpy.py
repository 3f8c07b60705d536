"""CPU restatement of the soft-modes rules (S1-S8 of include/rdf_labels.h).  TEST INFRASTRUCTURE ONLY.

Composite weights: inputs are per-layer label maps and per-layer confidence maps, uint16 [n_img][dim_y][dim_x], and the
conditions table int32 [n_cond][2].
  S1 path    rdf_composite's walk: off = 0; for layer j: l = labels[j][p]; l in (0, 65535): stop, nothing written; e = off + l - 1
             outside 0 .. n_cond - 1: stop, nothing written; (t, v) = cond[e]; t == 0: final; else off = v.  Falling off the last
             layer writes nothing.
  S2 weight  w = 65535; at every layer visited, the final one included, w = (w * conf[j][p] + 32767) // 65535 (uint32).
  S3 store   out[i][y][dim_x - 1 - x if flip_x else x] = w.
Weighted modes: labels, weights uint16 [n_img][dim_y][dim_x]; weights None = all 1.
  S4 pixels  class c = 1 .. L: labels == c, integer weight w; w == 0 contributes nothing.
  S5 round 0 m = (sum w x / sum w, sum w y / sum w), integer sums, one IEEE divide each; sum w == 0: NaN.
  S6 round r v2 = float64(float32(var * var)); g = exp(-((x - mx)^2 + (y - my)^2) / (2 v2)); m += (sum (w g) dx, sum (w g) dy) /
             sum w g.  num_rounds == 0: zeros.
  S7 heights oracle.mean_shift_numpy.fingertip_heights on the final means.
"""
import math

import numpy as np

NO_LABEL = 65535


def composite_weights(layer_labels, layer_conf, cond, flip_x=False, prefill=0):
    """layer_labels / layer_conf: sequences of uint16 [n_img, h, w] (or [h, w]) maps.  Returns (weights uint16 of the maps' shape
    over `prefill`, written bool of the same shape: where a weight was stored)."""
    labs = [np.asarray(a, np.uint16) for a in layer_labels]
    confs = [np.asarray(a, np.uint16) for a in layer_conf]
    shape = labs[0].shape
    h, w = shape[-2:]
    labs = [a.reshape(-1, h, w) for a in labs]
    confs = [a.reshape(-1, h, w) for a in confs]
    cond = np.asarray(cond, np.int64).reshape(-1, 2)
    out = np.full(labs[0].shape, prefill, np.uint16)
    written = np.zeros(labs[0].shape, bool)
    for i in range(labs[0].shape[0]):
        for y in range(h):
            for x in range(w):
                off, wt = 0, 65535
                for j in range(len(labs)):
                    l = int(labs[j][i, y, x])
                    if l == 0 or l == NO_LABEL:
                        break
                    e = off + l - 1
                    if e < 0 or e >= len(cond):
                        break
                    wt = (wt * int(confs[j][i, y, x]) + 32767) // 65535
                    assert wt * 65535 < 1 << 32
                    t, v = cond[e]
                    if t == 0:
                        q = w - 1 - x if flip_x else x
                        out[i, y, q] = wt
                        written[i, y, q] = True
                        break
                    off = int(v)
    return out.reshape(shape), written.reshape(shape)


def weighted_modes(labels, weights, num_labels, variances, num_rounds, trace=None):
    """One frame: labels (and weights, or None) [h, w].  Returns float64 [num_labels, 2]; trace receives a copy per round."""
    lab = np.asarray(labels).reshape(labels.shape[-2], labels.shape[-1]).astype(np.int64)
    h, w = lab.shape
    om = np.ones((h, w), np.float64) if weights is None else np.asarray(weights).reshape(h, w).astype(np.float64)
    iw = np.ones((h, w), np.int64) if weights is None else np.asarray(weights).reshape(h, w).astype(np.int64)
    yy, xx = np.mgrid[0:h, 0:w]
    var = np.asarray(variances, np.float32)
    means = np.zeros((num_labels, 2), np.float64)
    for rnd in range(num_rounds):
        for c in range(num_labels):
            m = (lab == c + 1) & (iw != 0)
            with np.errstate(invalid="ignore", divide="ignore", under="ignore"):
                if rnd == 0:
                    # integer sums (python ints: no bound), converted once
                    s = [np.float64(int((iw[m] * xx[m]).sum())), np.float64(int((iw[m] * yy[m]).sum())), np.float64(int(iw[m].sum()))]
                elif not m.any():
                    s = [np.float64(0.)] * 3
                else:
                    dx, dy = xx[m].astype(np.float64) - means[c, 0], yy[m].astype(np.float64) - means[c, 1]
                    v2 = np.float64(np.float32(var[c] * var[c]))
                    wg = om[m] * np.exp(-((dx * dx) + (dy * dy)) / (2 * v2))
                    s = [(dx * wg).sum(), (dy * wg).sum(), wg.sum()]
                means[c] = (means[c, 0] + s[0] / s[2], means[c, 1] + s[1] / s[2])
        if trace is not None:
            trace.append(means.copy())
    return means


def weighted_modes_long(labels, weights, num_labels, variances, num_rounds):
    """The same rounds with np.longdouble terms and math.fsum for every sum: the yardstick for the restatement's own rounding.
    Returns the means after every round."""
    LD = np.longdouble
    lab = np.asarray(labels)
    iw = np.ones(lab.shape, np.int64) if weights is None else np.asarray(weights).astype(np.int64)
    var = np.asarray(variances, np.float32)
    means = np.zeros((num_labels, 2), LD)
    out = []
    for rnd in range(num_rounds):
        for c in range(num_labels):
            ys, xs = np.nonzero((lab == c + 1) & (iw != 0))
            if xs.size == 0:
                means[c] = np.nan
                continue
            om = iw[ys, xs]
            if rnd == 0:
                s = (LD(int((om * xs).sum())), LD(int((om * ys).sum())), LD(int(om.sum())))
            else:
                dx, dy = xs.astype(LD) - means[c, 0], ys.astype(LD) - means[c, 1]
                v2 = LD(np.float32(var[c] * var[c]))
                with np.errstate(invalid="ignore", divide="ignore", under="ignore"):
                    p = om.astype(LD) * np.exp(-((dx * dx) + (dy * dy)) / (2 * v2))
                    tx, ty = dx * p, dy * p
                s = (LD(np.nan),) * 3 if np.isnan(p).any() else (LD(math.fsum(tx)), LD(math.fsum(ty)), LD(math.fsum(p)))
            with np.errstate(invalid="ignore", divide="ignore"):
                means[c] = (means[c, 0] + s[0] / s[2], means[c, 1] + s[1] / s[2])
        out.append(means.copy())
    return out
