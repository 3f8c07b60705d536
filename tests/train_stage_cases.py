"""Inputs of the trainer's stage tests (tests/test_training_stages.py): small seeded numpy builders that the CPU tests (the
restatement against values stated by hand and against float64) and the GPU tests (each entry point of
csrc/tree_train_hip.hip against the restatement's stage) both call, so that both see the same arrays.

Every output array of a case comes pre-filled -- the tree and the child counts with a sentinel bit pattern, not zero -- so a
word the stage must leave alone shows when it is touched.  WAVE and the two limits below are the kernels'."""
import functools
from typing import NamedTuple

import numpy as np

from oracle import train_numpy as tn

WAVE = 64               # k_train_pick_best: lane l scans proposals l, l + 64, ...; four waves (nodes) per workgroup
MAX_CLASSES = 64        # kMaxClasses
SCAN_THREADS = 1024     # k_train_next_active: one workgroup, thread t takes ceil(n_active / 1024) consecutive nodes
INIT_GRID_CAP = 2048    # rdf_train_init: blocks of 256 pixels, at most this many, then a grid-stride loop

SENT32 = np.uint32(0xCAFEBABE)                    # as float32: -8346975.0, a plain number below every gain
SENT_F32 = np.array([SENT32], np.uint32).view(np.float32)[0]
SENT64 = np.uint64(0xDEADBEEFCAFEF00D)
SENT_I32 = np.int32(-559038737)                   # 0xDEADBEEF
F32 = np.float32


# ---------------------------------------------------------------------------------------------------------------------
# rdf_train_pick_best
# ---------------------------------------------------------------------------------------------------------------------
class PickCase(NamedTuple):
    name: str
    active: np.ndarray        # int32 [n_active], ascending parents of `level`
    node_counts: np.ndarray   # uint64 [2^D, C]   parents' counts, by parent
    counts: np.ndarray        # uint64 [P, NB, C] children's counts of the node block [start, end)
    props: np.ndarray         # float32 [P, 5], props[j, 0] == j: the winner can be read off the record
    tree: np.ndarray          # float32 [2^D - 1, 7 + 2C], sentinel
    next_counts: np.ndarray   # uint64 [2^D, C], sentinel
    best_gain: np.ndarray     # float32 [n_active]
    level: int
    D: int
    start: int
    end: int
    expect: dict              # what the case states by hand (may be empty)

    @property
    def C(self):
        return self.node_counts.shape[1]

    @property
    def P(self):
        return self.props.shape[0]

    @property
    def NB(self):
        return self.counts.shape[1]


def make_props(P, seed):
    rng = np.random.default_rng(seed)
    props = rng.standard_normal((P, 5)).astype(np.float32)
    props[:, 0] = np.arange(P, dtype=np.float32)
    return props


def assemble(name, active, pc, lc, level, D, start=0, end=None, NB=None, best_gain=None, expect=None, seed=0):
    """pc uint64 [n, C] and lc uint64 [n, P, C] with lc <= pc, per active node; rc = pc - lc.  Bins of the count block that
    belong to no active node hold small random counts; parents that are not active hold 7s."""
    active = np.asarray(active, np.int32)
    pc, lc = np.asarray(pc, np.uint64), np.asarray(lc, np.uint64)
    n, P, C = lc.shape
    assert pc.shape == (n, C) and active.shape == (n,) and (np.diff(active) > 0).all()
    assert 0 <= level < D and (active >= 0).all() and (active < (1 << level)).all()
    assert (lc <= pc[:, None, :]).all()
    end = (1 << (level + 1)) if end is None else end
    NB = (end - start) if NB is None else NB
    assert 0 <= start < end <= (1 << (level + 1)) and end - start <= NB
    rng = np.random.default_rng(seed + 977)
    node_counts = np.full((1 << D, C), 7, np.uint64)
    node_counts[active] = pc
    counts = rng.integers(0, 6, size=(P, NB, C)).astype(np.uint64)
    for i, parent in enumerate(active.tolist()):
        if parent * 2 >= start and parent * 2 + 1 < end:
            counts[:, parent * 2 - start, :] = lc[i]
            counts[:, parent * 2 + 1 - start, :] = pc[i][None, :] - lc[i]
    tree = np.full(((1 << D) - 1, 7 + 2 * C), SENT_F32, np.float32)
    next_counts = np.full((1 << D, C), SENT64, np.uint64)
    if best_gain is None:
        best_gain = np.full(n, -1.0, np.float32)
    best_gain = np.asarray(best_gain, np.float32)
    case = PickCase(name, active, node_counts, counts, make_props(P, seed), tree, next_counts, best_gain, level, D, start,
                    end, expect or {})
    for a in (case.active, case.node_counts, case.counts, case.props, case.tree, case.next_counts, case.best_gain):
        a.setflags(write=False)
    return case


def children(case):
    """(indices into active of the nodes inside the window, pc [n, C], lc [n, P, C], rc [n, P, C]) read back from the arrays."""
    a = case.active.astype(np.int64)
    inside = np.nonzero((a * 2 >= case.start) & (a * 2 + 1 < case.end))[0]
    par = a[inside]
    lc = case.counts[:, par * 2 - case.start, :].transpose(1, 0, 2)
    rc = case.counts[:, par * 2 + 1 - case.start, :].transpose(1, 0, 2)
    return inside, case.node_counts[par], lc, rc


def gains(pc, lc):
    """float32 gains [n, P] of the restatement for pc [n, C], lc [n, P, C]."""
    pc, lc = np.asarray(pc, np.uint64), np.asarray(lc, np.uint64)
    return tn.block_gains(pc, lc, pc[:, None, :] - lc)


def random_pc(rng, n, C, lo, hi):
    """n count vectors whose sums lie in [lo, hi]: a sum, then that many draws of a class."""
    pc = np.zeros((n, C), np.uint64)
    for i in range(n):
        np.add.at(pc[i], rng.integers(0, C, size=int(rng.integers(lo, hi + 1))), 1)
    return pc


def random_lc(rng, pc, P):
    pc = np.asarray(pc, np.uint64)
    return rng.integers(0, pc[:, None, :].astype(np.int64) + 1, size=(pc.shape[0], P, pc.shape[1])).astype(np.uint64)


def plant_strict_maximum(pc_i, lc_i, positions):
    """Make the columns `positions` of one node identical and the strict maximum: the best random column goes there, every
    other column that reaches its gain is emptied on the right (gain 0)."""
    g = gains(pc_i[None], lc_i[None])[0]
    assert g.max() > 0
    best = lc_i[int(np.argmax(g))].copy()
    lc_i[g == g.max()] = pc_i
    lc_i[list(positions)] = best
    g = gains(pc_i[None], lc_i[None])[0]
    assert sorted(np.nonzero(g == g.max())[0].tolist()) == sorted(positions)


LANES_P = (1, 63, 64, 65, 128, 200, 1000)
LANES_N = (1, 3, 4, 5)      # four waves per workgroup: 5 leaves a workgroup with idle waves


@functools.lru_cache(maxsize=None)
def lanes_and_passes(P, n_active):
    """Counts that sum to at most 8, so exact fp32 ties between proposals are the rule.  For P >= 65 the first node's
    maximum sits at a, a + 64 (one lane, two passes) and at b in another lane, a the lowest: the lane's "first of equals"
    meets the wave's "lowest index of equals"."""
    seed = 1000 * P + n_active
    rng = np.random.default_rng(seed)
    C, level, D = 3, 3, 5
    active = np.sort(rng.choice(1 << level, size=n_active, replace=False))
    pc = random_pc(rng, n_active, C, 4, 8)
    lc = random_lc(rng, pc, P)
    if P > WAVE:
        while gains(pc[:1], lc[:1]).max() <= 0:
            pc[0] = random_pc(rng, 1, C, 4, 8)[0]
            lc[0] = random_lc(rng, pc[:1], P)[0]
        a = int(rng.integers(0, P - WAVE))
        b = int(rng.choice([j for j in range(a + 1, P) if j % WAVE != a % WAVE]))
        plant_strict_maximum(pc[0], lc[0], (a, a + WAVE, b))
    case = assemble(f"lanes_P{P}_n{n_active}", active, pc, lc, level, D, seed=seed)
    if P > WAVE:
        g = gains(pc, lc)
        tied = [np.nonzero(row == row.max())[0] for row in g]
        assert any(len(set((t % WAVE).tolist())) >= 2 for t in tied), "no tie across lanes"
        assert any(np.isin(t + WAVE, t).any() for t in tied), "no tie inside a lane (j and j + 64)"
    return case


PLACED = ((2, 65), (65, 66), (3, 67, 129), (64, 128))
PLACED_WINNERS = (2, 65, 3, 64)


@functools.lru_cache(maxsize=None)
def placed_ties():
    """P = 130; node k has identical columns at PLACED[k], the strict maximum; the first must win."""
    rng = np.random.default_rng(130)
    C, level, D, P = 3, 2, 4, 130
    pc = random_pc(rng, 4, C, 6, 8)
    pc[pc.sum(axis=1) == pc.max(axis=1)] = np.array([3, 3, 2], np.uint64)      # (a pure parent has no positive gain)
    lc = random_lc(rng, pc, P)
    for k, pos in enumerate(PLACED):
        plant_strict_maximum(pc[k], lc[k], pos)
    return assemble("placed_ties", np.arange(4), pc, lc, level, D, seed=130, expect={"winner": PLACED_WINNERS})


@functools.lru_cache(maxsize=None)
def many_nodes():
    """1030 active nodes of level 11, an ascending random subset of 0 .. 2047: more than one workgroup, the last one with
    idle waves, and parents far apart in the count block."""
    rng = np.random.default_rng(1030)
    C, level, D, P, n = 4, 11, 13, 70, 1030
    active = np.sort(rng.choice(1 << level, size=n, replace=False))
    pc = rng.integers(0, 50, size=(n, C)).astype(np.uint64)
    pc[:, 0] += 1
    return assemble("many_nodes", active, pc, random_lc(rng, pc, P), level, D, seed=1030)


@functools.lru_cache(maxsize=None)
def node_blocks():
    """The window [32, 48) of the 64 children of level 5: parents 16 .. 23 are inside, all others must keep the sentinel."""
    rng = np.random.default_rng(16)
    C, level, D, P = 3, 5, 7, 70
    active = np.array([0, 3, 14, 15, 16, 17, 19, 22, 23, 24, 25, 31])
    pc = random_pc(rng, active.size, C, 5, 30)
    outside = (active < 16) | (active > 23)
    best_gain = np.where(outside, SENT_F32, F32(-1)).astype(np.float32)
    return assemble("node_blocks", active, pc, random_lc(rng, pc, P), level, D, start=32, end=48, best_gain=best_gain,
                    seed=16, expect={"outside": np.nonzero(outside)[0].tolist()})


NO_SPLIT_PC = ((1, 2, 1), (8, 0, 8), (3, 4, 1))
NO_SPLIT_PDF = ((0.25, 0.5, 0.25), (0.5, 0.0, 0.5), (0.375, 0.5, 0.125))


@functools.lru_cache(maxsize=None)
def no_split():
    """Every proposal sends all pixels to one side: gain 0 > -1, a leaf with the parent's PDF on both sides, proposal 0."""
    rng = np.random.default_rng(5)
    P = 70
    pc = np.array(NO_SPLIT_PC, np.uint64)
    lc = np.where(rng.random((3, P, 1)) < 0.5, pc[:, None, :], np.uint64(0)).astype(np.uint64)
    return assemble("no_split", [1, 2, 6], pc, lc, 3, 5, seed=5, expect={"pdf": NO_SPLIT_PDF})


@functools.lru_cache(maxsize=None)
def negative_gain_triples():
    """(pc, lc) with both sides non-empty whose fp32 gain is below zero.  Searched: every pc = (a, b) with a + b <= 64 and
    every 0 <= lc <= pc (C = 2); for C = 3 only the splits in the parent's own proportions, lc = k * base and pc = m * base
    (the true gain is 0 there; elsewhere it is at least of the order 64^-3, well above the fp32 error)."""
    found = []
    rows_pc, rows_lc = [], []
    for a in range(0, 65):
        for b in range(0, 65 - a):
            x, y = np.meshgrid(np.arange(a + 1), np.arange(b + 1), indexing="ij")
            rows_lc.append(np.stack([x.ravel(), y.ravel()], axis=1))
            rows_pc.append(np.broadcast_to(np.array([a, b]), rows_lc[-1].shape))
    found.append(_negative(np.concatenate(rows_pc), np.concatenate(rows_lc)))
    rows_pc, rows_lc = [], []
    for base in np.ndindex(22, 22, 22):
        s = sum(base)
        if s == 0 or np.gcd.reduce(base) != 1:
            continue
        for m in range(2, 64 // s + 1):
            for k in range(1, m):
                rows_pc.append([m * v for v in base])
                rows_lc.append([k * v for v in base])
    found.append(_negative(np.array(rows_pc), np.array(rows_lc)))
    return found


def _negative(pc, lc):
    pc, lc = pc.astype(np.uint64), lc.astype(np.uint64)
    rc = pc - lc
    both = (lc.sum(axis=1) > 0) & (rc.sum(axis=1) > 0)
    pc, lc, rc = pc[both], lc[both], rc[both]
    g = tn._gini_gain_block(pc, lc, rc)
    neg = g < 0
    return pc[neg], lc[neg], g[neg]


@functools.lru_cache(maxsize=None)
def negative_gain():
    """Nodes all of whose proposals have a gain below zero (above the -1 of a fresh level): recorded, as leaves."""
    P = 6
    cases = []
    for C, (pc, lc, _) in zip((2, 3), negative_gain_triples()):
        if not len(pc):
            continue
        keys, inv, n_per = np.unique(pc, axis=0, return_inverse=True, return_counts=True)
        pcs, lcs = [], []
        for k in np.argsort(-n_per, kind="stable")[:5]:
            cols = lc[inv.ravel() == k]
            pcs.append(keys[k])
            lcs.append(cols[np.arange(P) % len(cols)])
        pcs, lcs = np.array(pcs, np.uint64), np.array(lcs, np.uint64)
        assert (gains(pcs, lcs) < 0).all()
        cases.append(assemble(f"negative_gain_C{C}", np.arange(len(pcs)) + 1, pcs, lcs, 3, 5, seed=C))
    return tuple(cases)


@functools.lru_cache(maxsize=None)
def previous_gain():
    """best_gain already holds the block's best gain exactly (nodes 0, 1: strict > leaves the record alone), one ulp less
    (2, 3: written) and one ulp more (4, 5: left alone)."""
    rng = np.random.default_rng(77)
    C, P = 3, 70
    pc = random_pc(rng, 6, C, 20, 40)
    pc[pc.sum(axis=1) == pc.max(axis=1)] = np.array([9, 8, 7], np.uint64)
    lc = random_lc(rng, pc, P)
    gb = gains(pc, lc).max(axis=1)
    assert (gb > 0).all()
    prev = gb.copy()
    prev[2:4] = np.nextafter(gb[2:4], F32(-np.inf))
    prev[4:6] = np.nextafter(gb[4:6], F32(np.inf))
    assert (prev[2:4] < gb[2:4]).all() and (prev[4:6] > gb[4:6]).all()
    return assemble("previous_gain", [0, 2, 3, 5, 6, 7], pc, lc, 3, 5, best_gain=prev, seed=77,
                    expect={"untouched": [0, 1, 4, 5], "written": [2, 3], "block_best": gb})


CUTOFF_SIDES = {2: ((999, 1), (1998, 2), (998, 2), (0, 1000)), 3: ((1, 999, 0),)}
CUTOFF_OTHER = {2: (500, 500), 3: (500, 300, 200)}
CUTOFF_CLASS = {(999, 1): 0, (1998, 2): 0, (998, 2): None, (0, 1000): 1, (1, 999, 0): 1}
assert F32(999) / F32(1000) == F32(0.999) and F32(1998) / F32(2000) == F32(0.999) and F32(998) / F32(1000) < F32(0.999)


@functools.lru_cache(maxsize=None)
def cutoff(C, last_level):
    """Each stated side once as the left and once as the right child of the winning proposal, the other child mixed; the
    second proposal splits nothing.  Node 2k has side k on the left, node 2k + 1 on the right."""
    sides, other = CUTOFF_SIDES[C], np.array(CUTOFF_OTHER[C], np.uint64)
    pcs, lcs, where = [], [], []
    for s in sides:
        s = np.array(s, np.uint64)
        for on_right in (0, 1):
            pc = s + other
            pcs.append(pc)
            lcs.append([other if on_right else s, pc])
            where.append((tuple(int(v) for v in s), on_right))
    level = 3
    D = level + 1 if last_level else level + 2
    return assemble(f"cutoff_C{C}_{'last' if last_level else 'inner'}", np.arange(len(pcs)), np.array(pcs), np.array(lcs),
                    level, D, seed=999, expect={"sides": where})


BIG = (2 ** 24 + 1, 2 ** 24 + 3, 2 ** 33 + 2 ** 9 + 1, 3 * 10 ** 9)


@functools.lru_cache(maxsize=None)
def big_counts():
    """Counts that (float) rounds -- 2^24 + 1 to even, 2^24 + 3 up, 2^33 + 2^9 + 1 just above a half ulp -- and counts above
    2^32, next to small ones.  Half of the proposals put exactly the big count on the left."""
    rng = np.random.default_rng(24)
    C, P = 3, 70
    pc = np.array([[b + int(rng.integers(1, 40)), int(rng.integers(1, 40)), int(rng.integers(0, 2 ** 20))] for b in BIG],
                  np.uint64)
    lc = np.zeros((len(BIG), P, C), np.uint64)
    for i, b in enumerate(BIG):
        for k in range(C):
            lc[i, :, k] = rng.integers(0, int(pc[i, k]) + 1, size=P, dtype=np.uint64)
        lc[i, ::2, 0] = np.uint64(b)
        lc[i, 1::4, 0] = np.uint64(b - 1)
    assert (pc > 2 ** 24).any() and (pc > 2 ** 32).any()
    return assemble("big_counts", [0, 1, 4, 7], pc, lc, 3, 5, seed=24)


@functools.lru_cache(maxsize=None)
def class_limits(C):
    """C = 1: every gain is 0.  C = 64 (kMaxClasses): records of 135 floats."""
    assert C in (1, MAX_CLASSES)
    rng = np.random.default_rng(C)
    n, P = 5, 70
    pc = rng.integers(0, 10, size=(n, C)).astype(np.uint64)
    pc[:, 0] += 1
    return assemble(f"class_limits_C{C}", [0, 1, 2, 3], pc[:4], random_lc(rng, pc[:4], P), 2, 4, seed=C)


@functools.lru_cache(maxsize=None)
def two_blocks(last_level):
    """Two proposal blocks for the same twelve nodes, the second call starting from what the first one left.  Small skewed
    counts: pure sides are common, so the second block often writes a single 1.0 into a PDF the first one filled."""
    rng = np.random.default_rng(212 + last_level)
    C, P, level = 4, 70, 4
    D = level + 1 if last_level else level + 3
    active = np.sort(rng.choice(1 << level, size=12, replace=False))
    pc = random_pc(rng, 12, C, 4, 12)
    pc[pc.sum(axis=1) == pc.max(axis=1)] = np.array([3, 1, 1, 0], np.uint64)
    lc_a = random_lc(rng, pc, P)
    lc_b = random_lc(rng, pc, P)
    ga_all, gb_all = gains(pc, lc_a), gains(pc, lc_b)
    for i in range(12):                    # nodes 0, 2, ..: the second block is better; 1, 5, 9: worse; 3, 7, 11: as drawn
        if i % 2 == 0:
            lc_a[i][ga_all[i] >= gb_all[i].max()] = pc[i]
        elif i % 4 == 1:
            lc_b[i][gb_all[i] >= ga_all[i].max()] = pc[i]
    ga, gb = gains(pc, lc_a).max(axis=1), gains(pc, lc_b).max(axis=1)
    assert (gb > ga).sum() >= 2 and (gb <= ga).sum() >= 2, (ga, gb)
    first = assemble(f"two_blocks_{'last' if last_level else 'inner'}_a", active, pc, lc_a, level, D, seed=1)
    second = assemble(f"two_blocks_{'last' if last_level else 'inner'}_b", active, pc, lc_b, level, D, seed=2)
    return first, second


def pick_cases():
    out = [lanes_and_passes(P, n) for P in LANES_P for n in LANES_N]
    out += [placed_ties(), many_nodes(), node_blocks(), no_split(), *negative_gain(), previous_gain()]
    out += [cutoff(C, last) for C in (2, 3) for last in (False, True)]
    out += [big_counts(), class_limits(1), class_limits(MAX_CLASSES)]
    return out


PICK_IDS = ([f"lanes_P{P}_n{n}" for P in LANES_P for n in LANES_N] +
            ["placed_ties", "many_nodes", "node_blocks", "no_split", "negative_gain_C2", "negative_gain_C3", "previous_gain",
             "cutoff_C2_inner", "cutoff_C2_last", "cutoff_C3_inner", "cutoff_C3_last", "big_counts", "class_limits_C1",
             "class_limits_C64"])


def pick_case(name):
    for c in pick_cases():
        if c.name == name:
            return c
    raise KeyError(name)


def run_pick_best(case, state=None, vectorised=True):
    """The restatement's stage on copies of the case's arrays (or on `state`, what an earlier call left)."""
    tree, nxt, bg = state if state is not None else (case.tree.copy(), case.next_counts.copy(), case.best_gain.copy())
    tn.pick_best(case.active, case.node_counts, case.counts, case.props, tree, nxt, bg, case.level, case.D, case.start,
                 case.end, vectorised=vectorised)
    return tree, nxt, bg


def gains_f64(pc, lc, rc):
    """Gini gain of every proposal in float64 from the integer counts, 0 where a side is empty: pc [n, C], lc, rc [n, P, C]."""
    def impurity(c):
        s = c.sum(axis=-1, keepdims=True)
        with np.errstate(all="ignore"):
            return 1.0 - ((c / s) ** 2).sum(axis=-1)
    pc, lc, rc = (np.asarray(a, np.uint64).astype(np.float64) for a in (pc, lc, rc))
    ls, rs, ps = lc.sum(axis=-1), rc.sum(axis=-1), pc.sum(axis=-1)[:, None]
    with np.errstate(all="ignore"):
        g = impurity(pc)[:, None] - (ls / ps * impurity(lc) + rs / ps * impurity(rc))
    return np.where((ls == 0) | (rs == 0), 0.0, g)


def gain_eps(C):
    """How far below the float64 maximum the fp32 winner's float64 gain may lie.  The fp32 expression has at most
    12 C + 15 roundings (three impurities of C + 1 conversions, C divisions, C squares, C additions and a subtraction; then
    three conversions, two divisions, two products, a sum and a difference).  Every intermediate lies in [0, 1], so a
    rounding is off by at most 2^-25 (half an ulp below 1); a square at most doubles an error that enters it (factor 2),
    every other step passes errors on with a weight of at most 1; and two gains are compared, the winner's and the
    float64 maximum's (another factor 2): 2 * 2 * (12 C + 15) * 2^-25 = 2 (12 C + 15) 2^-24.  Loose, and not measured."""
    return 2.0 * (12 * C + 15) * 2.0 ** -24


# ---------------------------------------------------------------------------------------------------------------------
# rdf_train_next_active
# ---------------------------------------------------------------------------------------------------------------------
class NextCase(NamedTuple):
    name: str
    tree: np.ndarray          # float32 [2^D - 1, 7 + 2C]
    active: np.ndarray        # int32 [max(n_active, 1)]
    n_active: int
    level: int
    D: int
    C: int
    next_active: np.ndarray   # int32 [2 n_active + 8], sentinel
    n_next: np.ndarray        # int32 [1], sentinel


NEXT_N = (0, 1, 1023, 1024, 1025, 2048, 5000)
NEXT_DENSITY = (0.0, 0.5, 1.0)


@functools.lru_cache(maxsize=None)
def next_active_case(n_active, density):
    """n_active nodes of level 13 (ascending random subset); their two flags are -1.0 with probability `density`, else 0.0.
    The records of the level's other nodes carry -1.0 flags that must not be picked up."""
    rng = np.random.default_rng(n_active * 10 + int(density * 2))
    level, D, C = 13, 14, 2
    tree = np.full(((1 << D) - 1, 7 + 2 * C), SENT_F32, np.float32)
    base = (1 << level) - 1
    tree[base:, 5:7] = -1.0
    active = np.sort(rng.choice(1 << level, size=n_active, replace=False)).astype(np.int32)
    tree[base + active.astype(np.int64), 5:7] = np.where(rng.random((n_active, 2)) < density, F32(-1), F32(0))
    if n_active == 0:
        active = np.array([SENT_I32], np.int32)
    case = NextCase(f"next_n{n_active}_d{density}", tree, active, n_active, level, D, C,
                    np.full(2 * n_active + 8, SENT_I32, np.int32), np.array([SENT_I32], np.int32))
    for a in (case.tree, case.active, case.next_active, case.n_next):
        a.setflags(write=False)
    return case


def run_next_active(case, per=None):
    """(next_active buffer, n_next) as the stage must leave them.  `per` (tests of the tests only) walks the list the way the
    kernel's 1024 threads do with that run length instead of ceil(n_active / 1024)."""
    act = case.active[:case.n_active]
    if per is not None:
        act = np.concatenate([act[t * per:t * per + per] for t in range(SCAN_THREADS)]) if case.n_active else act
    nxt = tn.next_active(case.tree, act, case.level, case.C)
    buf = case.next_active.copy()
    buf[:nxt.size] = nxt
    return buf, np.array([nxt.size], np.int32)


# ---------------------------------------------------------------------------------------------------------------------
# rdf_train_update_pixels
# ---------------------------------------------------------------------------------------------------------------------
class UpdateCase(NamedTuple):
    name: str
    depth: np.ndarray         # uint16 [n, h, w]
    nodes: np.ndarray         # int32 [n, h, w]
    tree: np.ndarray          # float32 [2^D - 1, 7 + 2C]
    level: int
    D: int
    C: int


def _records(rng, n):
    """n records of offsets, threshold and flags, drawn from the menu of the module docstring's edges."""
    inf = np.inf
    menu = np.concatenate([rng.uniform(-3000, 3000, 24), rng.uniform(-4e5, 4e5, 12),
                           [2.0 ** 20, -2.0 ** 20, 3e38, -3e38, inf, -inf, 0.0, -0.0]]).astype(np.float32)
    rec = np.zeros((n, 7), np.float32)
    rec[:, 0:4] = menu[rng.integers(0, menu.size, size=(n, 4))]
    thr = np.concatenate([np.exp(np.arange(12.0)), -np.exp(np.arange(12.0)), [np.nan, np.nan, np.nan]]).astype(np.float32)
    rec[:, 4] = thr[rng.integers(0, thr.size, size=n)]
    rec[:, 5:7] = np.array([[-1, -1], [-1, 0], [0, -1], [0, 0]], np.float32)[rng.integers(0, 4, size=n)]
    return rec


@functools.lru_cache(maxsize=None)
def update_pixels_case(shape=(3, 37, 53)):
    """Three frames of 37 x 53 (or one of 1 x 1) at level 11: nodes in 0 .. 2047, about 30 % retired; depth with 0, 65535
    and single digits (offsets of 2^20 then reach 10^5 .. 10^6 pixels); offsets that stay in the frame, leave it on every
    side, saturate the floor (3e38, inf) and wrap the add; thresholds +-e^k and NaN (never left); all four flag pairs."""
    rng = np.random.default_rng(sum(shape))
    level, D, C = 11, 13, 2
    depth = rng.integers(400, 4000, size=shape).astype(np.uint16)
    r = rng.random(shape)
    depth[r < 0.05] = 0
    depth[(r >= 0.05) & (r < 0.10)] = 65535
    depth[(r >= 0.10) & (r < 0.15)] = rng.integers(1, 10, size=int(((r >= 0.10) & (r < 0.15)).sum()))
    nodes = rng.integers(0, 1 << level, size=shape).astype(np.int32)
    nodes[rng.random(shape) < 0.3] = -1
    tree = np.full(((1 << D) - 1, 7 + 2 * C), SENT_F32, np.float32)
    base = (1 << level) - 1
    tree[base:base + (1 << level), 0:7] = _records(rng, 1 << level)
    if shape == (1, 1, 1):
        depth[:] = 7
        nodes[:] = 5
    case = UpdateCase("update_%dx%dx%d" % shape, depth, nodes, tree, level, D, C)
    for a in (case.depth, case.nodes, case.tree):
        a.setflags(write=False)
    return case


UPDATE_SHAPES = ((3, 37, 53), (1, 1, 1))


# ---------------------------------------------------------------------------------------------------------------------
# rdf_train_init
# ---------------------------------------------------------------------------------------------------------------------
class InitCase(NamedTuple):
    name: str
    labels: np.ndarray        # uint16 [n_px]
    C: int
    root: np.ndarray          # uint64 [C + 2]: non-zero counts the kernel adds to, then two sentinels


INIT_PX = (1, 255, 257, INIT_GRID_CAP * 256 + 77)     # the last one takes a second trip of the grid-stride loop
INIT_C = (1, 4, MAX_CLASSES)


@functools.lru_cache(maxsize=None)
def init_case(n_px, C):
    rng = np.random.default_rng(n_px + C)
    labels = rng.integers(0, C + 3, size=n_px).astype(np.uint16)
    labels[rng.random(n_px) < 0.02] = 65535
    if n_px > 1:
        labels[0], labels[-1] = 0, C          # not a pixel of the tree; a pixel of node 0 that no class counts
    root = np.concatenate([(1000 * np.arange(1, C + 1) + 7).astype(np.uint64), np.array([SENT64, SENT64], np.uint64)])
    labels.setflags(write=False)
    root.setflags(write=False)
    return InitCase(f"init_px{n_px}_C{C}", labels, C, root)


def init_expected(case):
    """nodes = 0 where the label is not 0, else -1; root += the number of pixels of each label 1 .. C - 1."""
    lab = case.labels.astype(np.int64)
    nodes = np.where(lab > 0, 0, -1).astype(np.int32)
    root = case.root.copy()
    root[:case.C] += np.bincount(lab[(lab > 0) & (lab < case.C)], minlength=case.C).astype(np.uint64)
    return nodes, root


# ---------------------------------------------------------------------------------------------------------------------
# rdf_train_right_counts
# ---------------------------------------------------------------------------------------------------------------------
class RightCase(NamedTuple):
    name: str
    active: np.ndarray        # int32 [37]
    node_counts: np.ndarray   # uint64 [64, C]
    counts: np.ndarray        # uint64 [P, NB, C], random; left children of the active nodes <= their parents
    start: int
    end: int


@functools.lru_cache(maxsize=None)
def right_counts_case():
    """37 of the 64 nodes of level 6, P = 130, C = 5, the window [32, 96) of the 128 children: parents 16 .. 47 inside."""
    rng = np.random.default_rng(37)
    n, P, C, start, end = 37, 130, 5, 32, 96
    active = np.sort(rng.choice(64, size=n, replace=False)).astype(np.int32)
    node_counts = rng.integers(0, 2 ** 40, size=(64, C)).astype(np.uint64)
    counts = rng.integers(0, 2 ** 62, size=(P, end - start, C)).astype(np.uint64)
    for parent in active.tolist():
        if 16 <= parent <= 47:
            counts[:, parent * 2 - start, :] = rng.integers(0, node_counts[parent].astype(np.int64) + 1, size=(P, C))
    assert ((active < 16) | (active > 47)).any() and ((active >= 16) & (active <= 47)).sum() > 8
    for a in (active, node_counts, counts):
        a.setflags(write=False)
    return RightCase("right_counts", active, node_counts, counts, start, end)


def right_counts_expected(case):
    out = case.counts.copy()
    for parent in case.active.tolist():
        if parent * 2 >= case.start and parent * 2 + 1 < case.end:
            left = out[:, parent * 2 - case.start, :]
            out[:, parent * 2 + 1 - case.start, :] = case.node_counts[parent][None, :] - left
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the counting kernels
# ---------------------------------------------------------------------------------------------------------------------
class CountCase(NamedTuple):
    name: str
    depth: np.ndarray         # uint16 [2, 19, 23]
    labels: np.ndarray        # uint16 [2, 19, 23]: 0 .. C + 1 (labels >= C are not counted, label 0 on a live node is)
    nodes: np.ndarray         # int32 [2, 19, 23]: 0 .. 7 and -1
    props: np.ndarray         # float32 [P, 5], as the trainer draws them
    C: int
    level: int
    parents: np.ndarray       # uint64 [8, C]: the plain count of the live pixels by (node, label)


COUNT_P = (1, 3, 5, 130, 1025)       # kBatch = 4 proposals at a time; above 1024 there are no sorted rows
COUNT_WINDOWS = ((0, 16, 16), (4, 12, 8))     # (start, end, NB) over the 16 children of level 3


@functools.lru_cache(maxsize=None)
def count_case(P):
    rng = np.random.default_rng(19 * 23)              # (the same frames for every P)
    shape, C, level = (2, 19, 23), 4, 3
    yy, xx = np.mgrid[0:shape[1], 0:shape[2]]
    depth = np.stack([600 + 40 * yy + 25 * xx, 3000 - 35 * yy + 11 * xx]).astype(np.uint16)
    depth += rng.integers(0, 200, size=shape).astype(np.uint16)
    r = rng.random(shape)
    depth[r < 0.04] = 0
    depth[(r >= 0.04) & (r < 0.08)] = 65535
    labels = rng.integers(0, C + 2, size=shape).astype(np.uint16)
    nodes = rng.integers(0, 1 << level, size=shape).astype(np.int32)
    nodes[rng.random(shape) < 0.25] = -1
    state = np.random.get_state()
    np.random.seed(1000 + P)
    props = tn.make_random_features(P)
    np.random.set_state(state)
    live = (nodes >= 0) & (labels < C)
    parents = np.zeros((1 << level, C), np.uint64)
    np.add.at(parents, (nodes[live], labels[live].astype(np.int64)), 1)
    assert (labels[nodes >= 0] >= C).any() and (labels[nodes >= 0] == 0).any()
    for a in (depth, labels, nodes, props, parents):
        a.setflags(write=False)
    return CountCase(f"counts_P{P}", depth, labels, nodes, props, C, level, parents)


@functools.lru_cache(maxsize=None)
def plain_counts(P, window):
    """The restatement's plain count of count_case(P) over one window, computed once and shared."""
    c = count_case(P)
    start, end, NB = window
    out = tn.count_children(c.depth, c.labels, c.nodes, c.props, start, end, NB, c.C)
    out.setflags(write=False)
    return out
