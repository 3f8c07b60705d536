// forest_refit_hip.hip -- leaf refit: the leaf distributions of a trained forest re-estimated from labelled depth frames,
// with the tree structure left as it is.  rdf_labels_refit_count walks every labelled pixel through every tree of the
// reference-layout forest exactly as inference walks it and ends in a 64-bit histogram over (tree, node, side, class) where
// inference ends in an argmax; rdf_labels_refit_apply turns the histogram into leaf PDFs.  Built into librdf_labels.so.  The
// forest's layout, the flag rule, the walk (walk_tree) and the ancestor's PDF are in rdf_forest_ref.hpp, shared with the
// pruning and the posterior.  The contract (rules R) is in include/rdf_labels.h and tests/refit_numpy.py restates it; all
// counts are integers, so no result depends on the order in which pixels are visited and two runs give the same bytes.
//
// k_refit_count: one lane per pixel, a wave takes 64 consecutive pixels and leaves at once when none of them carries a label
// (about 85 % of a frame).  A lane walks the trees one after the other; the level loop runs while any lane of the wave is
// still walking.  Where the walk ends decides how the pixel is counted:
//   - leaf slots of the first L levels (L the largest with T (2^L - 1) 2C <= kLdsCells) are few and take most pixels: a
//     wave's lanes share them, and so do all waves of the launch.  They are counted in a 32-bit LDS histogram (a workgroup
//     sees < 2^31 pixels) and a workgroup adds each non-zero cell to global memory once, at its end: atomics of a million
//     waves on one cache line would run at about 90 per microsecond.
//   - deeper leaf slots: the lanes of a wave that hold the same (slot, class) key go through ONE add, for the first
//     kAggIters distinct keys of the wave (wave_key_group, as in the trainer's k_train_sort); the lanes left after that hold keys
//     of their own -- at depth a wave's 64 pixels sit in up to 64 slots -- and add 1 each.  An add goes to the workgroup's
//     table of 2048 (cell, count) pairs in LDS, hashed by the cell's index in counts, when the cell's bucket is free or its
//     own, else to global memory as a 64-bit atomic: whatever the forest's shape, the slots that take most pixels end up in
//     the table (they arrive first and often), and a workgroup adds each pair to global memory once, at its end.
// totals stay in lane registers and are summed once per wave.
//
// rdf_labels_refit_apply: one launch per level bottom-up for the subtree sums (only with the ancestor fallback), then one
// launch per level top-down: a lane owns a node, learns from its parent whether it is reachable, and rewrites the PDFs of
// its leaf slots.  2D launches at most, no host synchronisation.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/rdf_labels.h"
#include "rdf_forest_ref.hpp"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxBlocks = 1024;      // larger calls stride over the grid: every workgroup ends with a flush of its LDS cells
constexpr int kLdsCells = 4096;       // 16 KB of 32-bit counters
constexpr int kAggIters = 4;          // distinct keys a wave aggregates before its remaining lanes add one each
constexpr int kTableBits = 11;        // 2048 (cell, count) pairs of 32 bits: another 16 KB
constexpr uint32_t kNoTag = 0xffffffffu;

struct CountArgs : ForestShape {
    const uint16_t *depth, *labels;
    uint32_t n_px, pix;               // all pixels (< 2^31), pixels of one image
    int W, H;
    const float *forest;
    int lds_levels;                   // L
    float scale;
    u64 *counts, *totals;
};

// n pixels of one (slot, class) below the histogram's levels: cell = its index in counts.  The workgroup's table takes it
// when the cell's bucket is free or already the cell's own; a bucket that another cell holds sends it to global memory.
__device__ __forceinline__ void add_deep(uint32_t *__restrict__ tags, uint32_t *__restrict__ vals, bool use_table,
                                         u64 *__restrict__ counts, size_t cell, uint32_t n)
{
    if (use_table) {
        const uint32_t tag = (uint32_t)cell, h = (tag * 0x9E3779B1u) >> (32 - kTableBits);
        const uint32_t was = atomicCAS(&tags[h], kNoTag, tag);
        if (was == kNoTag || was == tag) {
            atomicAdd(&vals[h], n);
            return;
        }
    }
    atomicAdd(counts + cell, (u64)n);
}

__global__ void __launch_bounds__(kThreads) k_refit_count(const CountArgs a)
{
    __shared__ uint32_t hist[kLdsCells];
    __shared__ uint32_t tags[1 << kTableBits], vals[1 << kTableBits];
    const int tid = threadIdx.x, lane = tid & 63;
    const int T = a.T, C = a.C, L = a.lds_levels;
    const uint32_t lds_nodes = (1u << L) - 1u;                      // per tree
    const uint32_t lds_cells = (uint32_t)T * lds_nodes * 2u * (uint32_t)C;
    const bool use_table = (u64)a.nodes() * 2u * (u64)C < (u64)kNoTag;   // a cell's index is its tag
    for (uint32_t i = tid; i < lds_cells; i += kThreads) hist[i] = 0u;
    for (uint32_t i = tid; i < (1u << kTableBits); i += kThreads) {
        tags[i] = kNoTag;
        vals[i] = 0u;
    }
    __syncthreads();

    uint32_t n_walked = 0u, n_unknown = 0u, n_no_depth = 0u, n_fell = 0u;
    // (no bound depends on the lane: every lane of a wave makes the same trips, as the ballots and shuffles need)
    for (uint32_t i0 = (blockIdx.x * (uint32_t)kThreads + (uint32_t)tid) - (uint32_t)lane; i0 < a.n_px;
         i0 += gridDim.x * (uint32_t)kThreads) {
        const uint32_t i = i0 + (uint32_t)lane;
        const uint32_t l = i < a.n_px ? (uint32_t)a.labels[i] : 0u;
        if (__ballot(l != 0u) == 0ull) continue;                    // (most of a frame is unlabelled)
        bool live = false;
        uint32_t d = 1u;
        if (l != 0u) {
            if (l >= (uint32_t)C) {
                ++n_unknown;
            } else {
                d = a.depth[i];
                if (d == 0u || d == kNoPixel) {
                    ++n_no_depth;
                } else {
                    live = true;
                    ++n_walked;
                }
            }
        }
        if (__ballot(live) == 0ull) continue;
        const uint32_t img = i / a.pix, rem = i - img * a.pix;
        const int y = (int)(rem / (uint32_t)a.W), x = (int)(rem - (uint32_t)y * (uint32_t)a.W);
        const WalkPixel p = {a.depth + (size_t)img * a.pix, a.W, a.H, x, y, (float)d, a.scale};

        for (int t = 0; t < T; ++t) {
            uint32_t key = 0u;
            bool has_key = false;
            walk_tree(a.forest + a.rec(t, 0), a.D, a.E(), p, live,
                      [&](int j, uint32_t n, uint32_t side, const float *) {
                          has_key = j >= L;                               // below the LDS histogram's levels
                          if (has_key) key = (n * 2u + side) * (uint32_t)C + l;    // < 2^32: the launcher checks
                          else atomicAdd(&hist[(((uint32_t)t * lds_nodes + n) * 2u + side) * (uint32_t)C + l], 1u);
                      },
                      [&] { ++n_fell; });
            u64 todo = __ballot(has_key);
            if (todo == 0ull) continue;
            const size_t cell0 = a.cell(t, 0, 0);                   // of the tree's first cell in counts
            for (int it = 0; it < kAggIters && todo != 0ull; ++it) {
                const KeyGroup grp = wave_key_group(todo, (int)key, has_key);
                if (lane == grp.src) add_deep(tags, vals, use_table, a.counts, cell0 + (uint32_t)grp.key, (uint32_t)__popcll(grp.lanes));
                if (has_key && key == (uint32_t)grp.key) has_key = false;
                todo &= ~grp.lanes;
            }
            if (has_key) add_deep(tags, vals, use_table, a.counts, cell0 + key, 1u);   // deep levels: every pixel a slot of its own
        }
    }

    const uint32_t w = wave_sum(n_walked), u = wave_sum(n_unknown), z = wave_sum(n_no_depth), o = wave_sum(n_fell);
    if (lane == 0) {
        if (w) atomicAdd(a.totals + 0, (u64)w);
        if (u) atomicAdd(a.totals + 1, (u64)u);
        if (z) atomicAdd(a.totals + 2, (u64)z);
        if (o) atomicAdd(a.totals + 3, (u64)o);
    }
    __syncthreads();
    const uint32_t per_tree = lds_nodes * 2u * (uint32_t)C;
    for (uint32_t i = tid; i < lds_cells; i += kThreads) {
        const uint32_t v = hist[i];
        if (v) {
            const uint32_t t = i / per_tree;
            atomicAdd(a.counts + a.cell(t, 0, 0) + (i - t * per_tree), (u64)v);
        }
    }
    for (uint32_t i = tid; i < (1u << kTableBits); i += kThreads)
        if (vals[i]) atomicAdd(a.counts + tags[i], (u64)vals[i]);
}

struct ApplyArgs : ForestShape {
    float *forest;
    const u64 *counts;
    u64 *sub;                         // [T][N][C], NULL without the ancestor fallback
    uint8_t *reach;                   // [T][N]
    u64 *report;
    int level;
    int fallback;
    u64 min_count;
};

// sub[t][a][c] for the nodes a of one level: per side, the slot's own counts where it is a leaf slot, else the child's
// sums (nothing at level D - 1, whose "go on" sides lead nowhere).  The level below is complete: launches are ordered.
__global__ void __launch_bounds__(kThreads) k_refit_subtree(const ApplyArgs a)
{
    const int C = a.C, j = a.level;
    const size_t level_nodes = (size_t)1 << j;
    const size_t idx = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (idx >= level_nodes * (size_t)a.T) return;
    const size_t t = idx >> j, g = idx & (level_nodes - 1), n = level_nodes - 1 + g;
    const float *rec = a.forest + a.rec(t, n);
    const u64 *own = a.counts + a.cell(t, n, 0);
    u64 *dst = a.sub + a.row(t, n);
    const bool leaf0 = is_leaf_slot(rec, 0), leaf1 = is_leaf_slot(rec, 1), last = j == a.D - 1;
    const u64 *child = a.sub + a.row(t, 2 * n + 1);                // the left child's sums; the right one's follow
    for (int c = 0; c < C; ++c) {
        const u64 v0 = leaf0 ? own[c] : last ? 0ull : child[c];
        const u64 v1 = leaf1 ? own[C + c] : last ? 0ull : child[C + c];
        dst[c] = v0 + v1;
    }
}

// One level, top-down.  A lane owns node n of tree t and learns from its parent whether it is reachable (the root is).
// Reachable leaf slots get their PDF by rule R3.
__global__ void __launch_bounds__(kThreads) k_refit_apply(const ApplyArgs a)
{
    const int C = a.C, j = a.level;
    const size_t level_nodes = (size_t)1 << j;
    const size_t idx = (size_t)blockIdx.x * kThreads + threadIdx.x;
    uint32_t n_own = 0u, n_anc = 0u, n_kept = 0u;
    if (idx < level_nodes * (size_t)a.T) {
        const size_t t = idx >> j, g = idx & (level_nodes - 1), n = level_nodes - 1 + g;
        float *rec = a.forest + a.rec(t, n);
        const bool reachable = is_reachable(a, a.forest, t, n, [&](size_t parent) { return a.reach[parent] != 0; });
        a.reach[a.at(t, n)] = reachable ? 1 : 0;
        if (reachable) {
            for (int s = 0; s < 2; ++s) {
                if (!is_leaf_slot(rec, s)) continue;
                SubRow src = {a.counts + a.cell(t, n, s), 0ull};
                for (int c = 0; c < C; ++c) src.sum += src.row[c];
                if (src.sum >= a.min_count) {
                    ++n_own;
                } else {
                    src.row = nullptr;
                    if (a.fallback == RDF_REFIT_FALLBACK_ANCESTOR) src = nearest_ancestor(a, a.sub, t, n, j, a.min_count);
                    if (src.row) ++n_anc; else ++n_kept;
                }
                if (src.row) write_pdf(rec + 7 + s * C, src.row, src.sum, C);
            }
        }
    }
    // (no lane has returned: the wave sums take all 64)
    const uint32_t o = wave_sum(n_own), an = wave_sum(n_anc), k = wave_sum(n_kept);
    if ((threadIdx.x & 63) == 0) {
        if (o) atomicAdd(a.report + 0, (u64)o);
        if (an) atomicAdd(a.report + 1, (u64)an);
        if (k) atomicAdd(a.report + 2, (u64)k);
        if (o + an + k) atomicAdd(a.report + 3, (u64)(o + an + k));
    }
}

}  // namespace

extern "C" {

int rdf_labels_refit_count(const uint16_t *depth, const uint16_t *labels, int n_img, int dim_x, int dim_y, const float *forest,
                           int n_trees, int max_depth, int n_classes, float scale_factor, uint64_t *counts, uint64_t *totals,
                           void *stream)
{
    if (n_img < 0 || dim_x < 0 || dim_y < 0 || bad_forest_shape(n_trees, max_depth, n_classes)) return RDF_ERR_BAD_ARG;
    CountArgs a = {{n_trees, max_depth, n_classes}};
    // a (slot, class) index within one tree is 32-bit
    if ((u64)a.N() * 2ull * (u64)n_classes >= (1ull << 32)) return RDF_ERR_TOO_LARGE;
    if (n_img == 0 || dim_x == 0 || dim_y == 0) return RDF_OK;
    if (!depth || !labels || !forest || !counts || !totals) return RDF_ERR_NULL_PTR;
    const long long pix = (long long)dim_x * dim_y;
    if (pix >= (1ll << 31) || pix * n_img >= (1ll << 31)) return RDF_ERR_TOO_LARGE;
    if (misaligned(depth, 2) || misaligned(labels, 2) || misaligned(forest, 4) || misaligned(counts, 8) || misaligned(totals, 8))
        return RDF_ERR_BAD_ARG;

    a.depth = depth;
    a.labels = labels;
    a.n_px = (uint32_t)(pix * n_img);
    a.pix = (uint32_t)pix;
    a.W = dim_x;
    a.H = dim_y;
    a.forest = forest;
    a.scale = scale_factor;
    a.counts = reinterpret_cast<u64 *>(counts);
    a.totals = reinterpret_cast<u64 *>(totals);
    a.lds_levels = 0;
    while (a.lds_levels < max_depth &&
           (unsigned long long)n_trees * ((2ull << a.lds_levels) - 1) * 2ull * (unsigned long long)n_classes <= (unsigned long long)kLdsCells)
        ++a.lds_levels;
    unsigned grid = blocks(a.n_px, kThreads);
    grid = grid > (unsigned)kMaxBlocks ? (unsigned)kMaxBlocks : grid;
    hipLaunchKernelGGL(k_refit_count, dim3(grid), dim3(kThreads), 0, S(stream), a);
    return (int)hipGetLastError();
}

size_t rdf_labels_refit_workspace_bytes(int n_trees, int max_depth, int n_classes)
{
    if (bad_forest_shape(n_trees, max_depth, n_classes)) return 0;
    const ForestShape f = {n_trees, max_depth, n_classes};
    return f.nodes() * (size_t)n_classes * sizeof(uint64_t) + ((f.nodes() + 7) & ~(size_t)7);
}

int rdf_labels_refit_apply(float *forest, int n_trees, int max_depth, int n_classes, const uint64_t *counts, uint64_t min_count,
                           int fallback, void *workspace, uint64_t *report, void *stream)
{
    if (bad_forest_shape(n_trees, max_depth, n_classes) || min_count < 1 ||
        (fallback != RDF_REFIT_FALLBACK_KEEP && fallback != RDF_REFIT_FALLBACK_ANCESTOR))
        return RDF_ERR_BAD_ARG;
    if (!forest || !counts || !workspace || !report) return RDF_ERR_NULL_PTR;
    if (misaligned(forest, 4) || misaligned(counts, 8) || misaligned(workspace, 8) || misaligned(report, 8)) return RDF_ERR_BAD_ARG;

    ApplyArgs a = {{n_trees, max_depth, n_classes}};
    a.forest = forest;
    a.counts = reinterpret_cast<const u64 *>(counts);
    a.sub = reinterpret_cast<u64 *>(workspace);
    a.reach = reinterpret_cast<uint8_t *>(a.sub + a.nodes() * (size_t)n_classes);
    a.report = reinterpret_cast<u64 *>(report);
    a.fallback = fallback;
    a.min_count = min_count;
    hipStream_t s = S(stream);
    hipError_t err = hipMemsetAsync(report, 0, 4 * sizeof(uint64_t), s);
    if (err != hipSuccess) return (int)err;
    if (fallback == RDF_REFIT_FALLBACK_ANCESTOR) {
        for (a.level = max_depth - 1; a.level >= 0; --a.level)
            hipLaunchKernelGGL(k_refit_subtree, dim3(blocks((long long)n_trees << a.level, kThreads)), dim3(kThreads), 0, s, a);
    }
    for (a.level = 0; a.level < max_depth; ++a.level)
        hipLaunchKernelGGL(k_refit_apply, dim3(blocks((long long)n_trees << a.level, kThreads)), dim3(kThreads), 0, s, a);
    return (int)hipGetLastError();
}

}  // extern "C"
