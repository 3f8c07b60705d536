// forest_refit_hip.hip -- leaf refit: the leaf distributions of a trained forest re-estimated from labelled depth frames,
// with the tree structure left as it is.  rdf_labels_refit_count walks every labelled pixel through every tree of the
// reference-layout forest (float32 [T][2^D - 1][7 + 2C], what DecisionForest.forest_cu holds) exactly as inference walks it
// and ends in a 64-bit histogram over (tree, node, side, class) where inference ends in an argmax;
// rdf_labels_refit_apply turns the histogram into leaf PDFs.  Built into librdf_labels.so.  The contract (rules R) is in
// include/rdf_labels.h and tests/refit_numpy.py restates it; all counts are integers, so no result depends on the order
// in which pixels are visited and two runs give the same bytes.
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
#include "rdf_device.hpp"
#include "rdf_kernel_util.hpp"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxBlocks = 1024;      // larger calls stride over the grid: every workgroup ends with a flush of its LDS cells
constexpr int kLdsCells = 4096;       // 16 KB of 32-bit counters
constexpr int kAggIters = 4;          // distinct keys a wave aggregates before its remaining lanes add one each
constexpr int kTableBits = 11;        // 2048 (cell, count) pairs of 32 bits: another 16 KB
constexpr uint32_t kNoTag = 0xffffffffu;
constexpr int kMaxDepth = 30;

struct CountArgs {
    const uint16_t *depth, *labels;
    uint32_t n_px, pix;               // all pixels (< 2^31), pixels of one image
    int W, H;
    const float *forest;
    int T, D, C;
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
    const int T = a.T, D = a.D, C = a.C, E = 7 + 2 * C, L = a.lds_levels;
    const size_t N = ((size_t)1 << D) - 1;
    const uint32_t lds_nodes = (1u << L) - 1u;                      // per tree
    const uint32_t lds_cells = (uint32_t)T * lds_nodes * 2u * (uint32_t)C;
    const bool use_table = (u64)T * N * 2u * (u64)C < (u64)kNoTag;  // a cell's index is its tag
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
        const uint16_t *__restrict__ frame = a.depth + (size_t)img * a.pix;
        const float df = (float)d;

        for (int t = 0; t < T; ++t) {
            const float *__restrict__ tree = a.forest + (size_t)t * N * E;
            uint32_t g = 0u, key = 0u;
            bool walking = live, has_key = false;
            for (int j = 0; j < D && __ballot(walking) != 0ull; ++j) {
                if (!walking) continue;
                const uint32_t n = ((1u << j) - 1u) + g;
                const float *__restrict__ rec = tree + (size_t)n * E;
                const float s = a.scale;
                // `uv_scale * u.x / d_f`: one multiply and one IEEE divide, both rounded to nearest (no contraction, no
                // reciprocal: the library's flags); floor with saturation, NaN -> 0; a wrapping add
                const int ux = offset_coord(x, s * rec[0], df), uy = offset_coord(y, s * rec[1], df);
                const int vx = offset_coord(x, s * rec[2], df), vy = offset_coord(y, s * rec[3], df);
                const float f = depth_or_no_pixel<uint32_t>(frame, a.W, a.H, ux, uy) - depth_or_no_pixel<uint32_t>(frame, a.W, a.H, vx, vy);
                const uint32_t side = f < rec[4] ? 0u : 1u;         // NaN goes right
                if (floor_i32(rec[5 + side]) != -1) {               // a leaf slot, at every level
                    walking = false;
                    if (j < L) {
                        atomicAdd(&hist[(((uint32_t)t * lds_nodes + n) * 2u + side) * (uint32_t)C + l], 1u);
                    } else {
                        has_key = true;
                        key = (n * 2u + side) * (uint32_t)C + l;    // < 2^32: the launcher checks
                    }
                } else if (j == D - 1) {                            // the flag says "go on" and there is no level to go to
                    walking = false;
                    ++n_fell;
                } else {
                    g = g * 2u + side;
                }
            }
            u64 todo = __ballot(has_key);
            if (todo == 0ull) continue;
            const size_t cell0 = (size_t)t * N * 2u * (size_t)C;   // of the tree's first cell in counts
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
            atomicAdd(a.counts + (size_t)t * N * 2u * (size_t)C + (i - t * per_tree), (u64)v);
        }
    }
    for (uint32_t i = tid; i < (1u << kTableBits); i += kThreads)
        if (vals[i]) atomicAdd(a.counts + tags[i], (u64)vals[i]);
}

struct ApplyArgs {
    float *forest;
    const u64 *counts;
    u64 *sub;                         // [T][N][C], NULL without the ancestor fallback
    uint8_t *reach;                   // [T][N]
    u64 *report;
    int T, D, C, level;
    int fallback;
    u64 min_count;
};

// sub[t][a][c] for the nodes a of one level: per side, the slot's own counts where it is a leaf slot, else the child's
// sums (nothing at level D - 1, whose "go on" sides lead nowhere).  The level below is complete: launches are ordered.
__global__ void __launch_bounds__(kThreads) k_refit_subtree(const ApplyArgs a)
{
    const int C = a.C, E = 7 + 2 * C, j = a.level;
    const size_t N = ((size_t)1 << a.D) - 1, level_nodes = (size_t)1 << j;
    const size_t idx = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (idx >= level_nodes * (size_t)a.T) return;
    const size_t t = idx >> j, g = idx & (level_nodes - 1), n = level_nodes - 1 + g;
    const float *rec = a.forest + (t * N + n) * E;
    const u64 *own = a.counts + (t * N + n) * 2 * C;
    u64 *dst = a.sub + (t * N + n) * C;
    const bool leaf0 = floor_i32(rec[5]) != -1, leaf1 = floor_i32(rec[6]) != -1, last = j == a.D - 1;
    const u64 *child = a.sub + (t * N + (2 * level_nodes - 1 + 2 * g)) * C;      // the left child's sums; the right one's follow
    for (int c = 0; c < C; ++c) {
        const u64 v0 = leaf0 ? own[c] : last ? 0ull : child[c];
        const u64 v1 = leaf1 ? own[C + c] : last ? 0ull : child[C + c];
        dst[c] = v0 + v1;
    }
}

// One level, top-down.  A lane owns node n of tree t: reachable iff it is the root or its parent is reachable and the
// parent's flag towards it floors to -1.  Reachable leaf slots get their PDF by rule R3.
__global__ void __launch_bounds__(kThreads) k_refit_apply(const ApplyArgs a)
{
    const int C = a.C, E = 7 + 2 * C, j = a.level;
    const size_t N = ((size_t)1 << a.D) - 1, level_nodes = (size_t)1 << j;
    const size_t idx = (size_t)blockIdx.x * kThreads + threadIdx.x;
    uint32_t n_own = 0u, n_anc = 0u, n_kept = 0u;
    if (idx < level_nodes * (size_t)a.T) {
        const size_t t = idx >> j, g = idx & (level_nodes - 1), n = level_nodes - 1 + g;
        float *rec = a.forest + (t * N + n) * E;
        bool reachable = true;
        if (j > 0) {
            const size_t parent = (level_nodes >> 1) - 1 + (g >> 1);
            reachable = a.reach[t * N + parent] != 0 && floor_i32(a.forest[(t * N + parent) * E + 5 + (g & 1)]) == -1;
        }
        a.reach[t * N + n] = reachable ? 1 : 0;
        if (reachable) {
            for (int s = 0; s < 2; ++s) {
                if (floor_i32(rec[5 + s]) == -1) continue;
                const u64 *src = a.counts + ((t * N + n) * 2 + s) * C;
                u64 sum = 0ull;
                for (int c = 0; c < C; ++c) sum += src[c];
                if (sum >= a.min_count) {
                    ++n_own;
                } else {
                    src = nullptr;
                    if (a.fallback == RDF_REFIT_FALLBACK_ANCESTOR) {        // the nearest ancestor-or-self with enough pixels
                        size_t an = n;
                        for (int lv = j; lv >= 0; --lv) {
                            const u64 *cand = a.sub + (t * N + an) * C;
                            sum = 0ull;
                            for (int c = 0; c < C; ++c) sum += cand[c];
                            if (sum >= a.min_count) {
                                src = cand;
                                break;
                            }
                            an = (an - 1) >> 1;     // (not followed at the root: lv ends the loop)
                        }
                    }
                    if (src) ++n_anc; else ++n_kept;
                }
                if (src) {
                    const float den = (float)sum;                          // uint64 -> fp32, round to nearest even
                    for (int c = 0; c < C; ++c) rec[7 + s * C + c] = (float)src[c] / den;
                }
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

bool bad_shape(int T, int D, int C) { return T < 1 || D < 1 || D > kMaxDepth || C < 1 || C > 65535; }

}  // namespace

extern "C" {

int rdf_labels_refit_count(const uint16_t *depth, const uint16_t *labels, int n_img, int dim_x, int dim_y, const float *forest,
                           int n_trees, int max_depth, int n_classes, float scale_factor, uint64_t *counts, uint64_t *totals,
                           void *stream)
{
    if (n_img < 0 || dim_x < 0 || dim_y < 0 || bad_shape(n_trees, max_depth, n_classes)) return RDF_ERR_BAD_ARG;
    // a (slot, class) index within one tree is 32-bit
    if ((((unsigned long long)1 << max_depth) - 1) * 2ull * (unsigned long long)n_classes >= (1ull << 32)) return RDF_ERR_TOO_LARGE;
    if (n_img == 0 || dim_x == 0 || dim_y == 0) return RDF_OK;
    if (!depth || !labels || !forest || !counts || !totals) return RDF_ERR_NULL_PTR;
    const long long pix = (long long)dim_x * dim_y;
    if (pix >= (1ll << 31) || pix * n_img >= (1ll << 31)) return RDF_ERR_TOO_LARGE;
    if (misaligned(depth, 2) || misaligned(labels, 2) || misaligned(forest, 4) || misaligned(counts, 8) || misaligned(totals, 8))
        return RDF_ERR_BAD_ARG;

    CountArgs a;
    a.depth = depth;
    a.labels = labels;
    a.n_px = (uint32_t)(pix * n_img);
    a.pix = (uint32_t)pix;
    a.W = dim_x;
    a.H = dim_y;
    a.forest = forest;
    a.T = n_trees;
    a.D = max_depth;
    a.C = n_classes;
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
    if (bad_shape(n_trees, max_depth, n_classes)) return 0;
    const size_t nodes = (size_t)n_trees * (((size_t)1 << max_depth) - 1);
    return nodes * (size_t)n_classes * sizeof(uint64_t) + ((nodes + 7) & ~(size_t)7);
}

int rdf_labels_refit_apply(float *forest, int n_trees, int max_depth, int n_classes, const uint64_t *counts, uint64_t min_count,
                           int fallback, void *workspace, uint64_t *report, void *stream)
{
    if (bad_shape(n_trees, max_depth, n_classes) || min_count < 1 ||
        (fallback != RDF_REFIT_FALLBACK_KEEP && fallback != RDF_REFIT_FALLBACK_ANCESTOR))
        return RDF_ERR_BAD_ARG;
    if (!forest || !counts || !workspace || !report) return RDF_ERR_NULL_PTR;
    if (misaligned(forest, 4) || misaligned(counts, 8) || misaligned(workspace, 8) || misaligned(report, 8)) return RDF_ERR_BAD_ARG;

    const size_t nodes = (size_t)n_trees * (((size_t)1 << max_depth) - 1);
    ApplyArgs a;
    a.forest = forest;
    a.counts = reinterpret_cast<const u64 *>(counts);
    a.sub = reinterpret_cast<u64 *>(workspace);
    a.reach = reinterpret_cast<uint8_t *>(workspace) + nodes * (size_t)n_classes * sizeof(uint64_t);
    a.report = reinterpret_cast<u64 *>(report);
    a.T = n_trees;
    a.D = max_depth;
    a.C = n_classes;
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
