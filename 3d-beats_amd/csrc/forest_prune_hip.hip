// forest_prune_hip.hip -- reduced-error pruning of a trained forest on held-out counts: subtrees whose split does not pay for
// its leaves are folded into one leaf slot of their parent.  rdf_labels_prune_plan reads the reference-layout forest (through
// rdf_forest_ref.hpp, as the refit and the posterior do) and the counts of the leaf refit (uint64 [T][N][2][C], where labelled
// pixels land) and decides; rdf_labels_prune_apply rewrites forest and counts by the last plan.  Built into librdf_labels.so.
// The contract (rules P1 to P4) is in include/rdf_labels.h and tests/prune_numpy.py restates it; everything but the final PDFs
// is unsigned 64-bit integer arithmetic, so two runs give the same bytes.
//
// A plan is three sweeps over the levels: reachability top-down, rule P2 bottom-up, the reachability that is left top-down.
// rdf_labels_refit_apply pays one launch per level and direction; here the levels are cut in two instead:
//   - the top levels, those with T * 2^j <= 1024 (at least level 0), belong to ONE workgroup of 1024 threads that sweeps them
//     with a barrier between levels (k_prune_top_reach, k_prune_top_plan);
//   - below them every node of the first deep level is the root of a subtree that no other subtree touches: one workgroup of
//     256 threads per such root sweeps its subtree down, up and (after the top levels are decided) down again, a barrier
//     between levels (k_prune_deep_up, k_prune_deep_after).  A subtree's nodes of one level are consecutive in heap order.
// So a plan is four launches and two memsets (the report, the state bytes) whatever the depth.  A lane owns a node for the
// time of a level; a node that is not reachable costs its lane one byte (the workspace's state bytes are zeroed by the
// memset): trained forests are sparse at depth and heap-order neighbours share ancestors, so whole waves leave a level
// without loading a count, and a subtree stops descending at the first level that holds none of its reachable nodes.
// apply needs no order between the levels, the plan's state bytes say everything: k_prune_fold (one lane per node) rewrites
// the collapsed sides of the nodes that stay, k_prune_clear zeroes the records and counts of the nodes that do not.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/rdf_labels.h"
#include "rdf_forest_ref.hpp"

namespace {

constexpr int kTopThreads = 1024;     // the one workgroup of the top levels
constexpr int kThreads = 256;
constexpr uint8_t kReachBefore = 1, kCollapse = 2, kReachAfter = 4;

struct Meta { u64 err, errB, leaves, leavesB; };   // rule P2, per node

struct PruneArgs : ForestShape {
    float *forest;                    // written by apply only
    u64 *counts;                      // likewise
    uint8_t *state;                   // [T][N]: kReachBefore | kCollapse | kReachAfter
    u64 *sub;                         // [T][N][C]
    Meta *meta;                       // [T][N]
    u64 *report;                      // [8], plan only
    int top;                          // levels 0 .. top - 1 are the one workgroup's, 1 <= top <= D
    int max_levels;
    u64 cost, min_count;
};

// reachable before (is_reachable): the level above is complete
__device__ __forceinline__ void reach_step(const PruneArgs &a, size_t t, int j, size_t g)
{
    const size_t n = ((size_t)1 << j) - 1 + g;
    if (is_reachable(a, a.forest, t, n, [&](size_t parent) { return (a.state[parent] & kReachBefore) != 0; }))
        a.state[a.at(t, n)] = kReachBefore;            // (the memset left 0)
}

// rule P2 for one reachable node: sub, err, errB, leaves, leavesB and the collapse bit.  The level below is complete.
__device__ __forceinline__ void plan_step(const PruneArgs &a, size_t t, int j, size_t g)
{
    const int C = a.C;
    const size_t n = ((size_t)1 << j) - 1 + g, at = a.at(t, n);
    if (!(a.state[at] & kReachBefore)) return;
    const float *rec = a.forest + a.rec(t, n);
    u64 *dst = a.sub + a.row(t, n);
    Meta m = {0ull, 0ull, 0ull, 0ull};
    const bool last = j == a.D - 1;
    bool summed = false;                               // dst holds a side's counts already
    for (int s = 0; s < 2; ++s) {
        if (is_leaf_slot(rec, s)) {                    // rule P1
            const u64 *cnt = a.counts + a.cell(t, n, s);
            const float *pdf = rec + 7 + s * C;
            float best = 0.f;
            int k = 0;
            u64 sum = 0ull;
            for (int c = 0; c < C; ++c) {
                const float v = pdf[c];
                const u64 x = cnt[c];
                if (v > best) {
                    best = v;
                    k = c;
                }
                sum += x;
                dst[c] = summed ? dst[c] + x : x;
            }
            summed = true;
            const u64 e = sum - cnt[k];
            m.err += e;
            m.errB += e;
            m.leaves += 1ull;
            m.leavesB += 1ull;
        } else if (!last) {
            const size_t child = a.at(t, 2 * n + 1 + s);
            const u64 *cs = a.sub + a.row(t, 2 * n + 1 + s);
            u64 sum = 0ull, top = 0ull;
            for (int c = 0; c < C; ++c) {
                const u64 x = cs[c];
                sum += x;
                top = x > top ? x : top;
                dst[c] = summed ? dst[c] + x : x;
            }
            summed = true;
            const Meta cm = a.meta[child];
            m.errB += cm.errB;
            m.leavesB += cm.leavesB;
            if (a.state[child] & kCollapse) {
                m.err += sum - top;
                m.leaves += 1ull;
            } else {
                m.err += cm.err;
                m.leaves += cm.leaves;
            }
        }
    }
    if (!summed)
        for (int c = 0; c < C; ++c) dst[c] = 0ull;
    a.meta[at] = m;
    if (n != 0) {
        u64 Z = 0ull, top = 0ull;
        for (int c = 0; c < C; ++c) {
            const u64 x = dst[c];
            Z += x;
            top = x > top ? x : top;
        }
        const u64 extra = m.leaves > 0ull ? m.leaves - 1ull : 0ull;
        if (j >= a.max_levels || Z < a.min_count || Z - top <= m.err + a.cost * extra) a.state[at] = kReachBefore | kCollapse;
    }
}

struct AfterSums { uint32_t nodes, turned, deepest; };   // of one lane: reachable nodes after, sides turned, 1 + deepest level

// reachable after: the root, and a child that does not collapse, whose parent is reachable after and flags "go on" towards
// it.  Returns whether the node is.
__device__ __forceinline__ bool after_step(const PruneArgs &a, size_t t, int j, size_t g, AfterSums &sums)
{
    const size_t n = ((size_t)1 << j) - 1 + g, at = a.at(t, n);
    const uint8_t st = a.state[at];
    if (!(st & kReachBefore) || (st & kCollapse)) return false;
    if (j > 0 && !(a.state[a.at(t, (n - 1) >> 1)] & kReachAfter)) return false;     // (its flag said "go on": st has kReachBefore)
    a.state[at] = st | kReachAfter;
    sums.nodes += 1u;
    sums.deepest = (uint32_t)(j + 1);                   // a lane's levels only grow
    if (j < a.D - 1) {
        const float *rec = a.forest + a.rec(t, n);
        for (int s = 0; s < 2; ++s)
            if (!is_leaf_slot(rec, s) && (a.state[a.at(t, 2 * n + 1 + s)] & kCollapse)) sums.turned += 1u;
    }
    return true;
}

// (every lane of the workgroup arrives: the wave sums take all 64)
__device__ __forceinline__ void add_after_sums(const PruneArgs &a, const AfterSums &sums)
{
    const uint32_t nodes = wave_sum(sums.nodes), turned = wave_sum(sums.turned);
    uint32_t deepest = sums.deepest;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const uint32_t o = (uint32_t)__shfl_xor((int)deepest, m, 64);
        deepest = o > deepest ? o : deepest;
    }
    if ((threadIdx.x & 63) == 0) {
        if (nodes) atomicAdd(a.report + 7, (u64)nodes);
        if (turned) atomicAdd(a.report + 2, (u64)turned);
        if (deepest) atomicMax(a.report + 3, (u64)deepest);
    }
}

__global__ void __launch_bounds__(kTopThreads) k_prune_top_reach(const PruneArgs a)
{
    for (int j = 0; j < a.top; ++j) {
        const size_t per = (size_t)1 << j, all = per * (size_t)a.T;
        for (size_t idx = threadIdx.x; idx < all; idx += kTopThreads) reach_step(a, idx >> j, j, idx & (per - 1));
        __syncthreads();
    }
}

__global__ void __launch_bounds__(kTopThreads) k_prune_top_plan(const PruneArgs a)
{
    for (int j = a.top - 1; j >= 0; --j) {
        const size_t per = (size_t)1 << j, all = per * (size_t)a.T;
        for (size_t idx = threadIdx.x; idx < all; idx += kTopThreads) plan_step(a, idx >> j, j, idx & (per - 1));
        __syncthreads();
    }
    for (size_t t = threadIdx.x; t < (size_t)a.T; t += kTopThreads) {        // rule P4, the roots' part
        const Meta m = a.meta[a.at(t, 0)];
        u64 Z = 0ull;
        for (int c = 0; c < a.C; ++c) Z += a.sub[a.row(t, 0) + c];
        atomicAdd(a.report + 0, m.leavesB);
        atomicAdd(a.report + 1, m.leaves);
        atomicAdd(a.report + 4, m.errB);
        atomicAdd(a.report + 5, m.err);
        atomicAdd(a.report + 6, Z);
    }
    AfterSums sums = {0u, 0u, 0u};
    for (int j = 0; j < a.top; ++j) {
        const size_t per = (size_t)1 << j, all = per * (size_t)a.T;
        for (size_t idx = threadIdx.x; idx < all; idx += kTopThreads) after_step(a, idx >> j, j, idx & (per - 1), sums);
        __syncthreads();
    }
    add_after_sums(a, sums);
}

// One workgroup per node of level a.top: blockIdx = tree * 2^top + the node's index in its level.  Down for reachability,
// then up for rule P2; the subtree's root is decided last.
__global__ void __launch_bounds__(kThreads) k_prune_deep_up(const PruneArgs a)
{
    const size_t bid = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
    if (bid >= ((size_t)a.T << a.top)) return;          // (the workgroup as one)
    const size_t t = bid >> a.top, g0 = bid & (((size_t)1 << a.top) - 1);
    int bottom = a.top - 1;                             // the deepest level with a reachable node of this subtree
    for (int j = a.top; j < a.D; ++j) {
        const size_t width = (size_t)1 << (j - a.top), first = g0 << (j - a.top);
        int any = 0;
        for (size_t i = threadIdx.x; i < width; i += kThreads) {
            reach_step(a, t, j, first + i);
            any |= a.state[a.at(t, ((size_t)1 << j) - 1 + first + i)] & kReachBefore;
        }
        if (!__syncthreads_or(any)) break;
        bottom = j;
    }
    for (int j = bottom; j >= a.top; --j) {
        const size_t width = (size_t)1 << (j - a.top), first = g0 << (j - a.top);
        for (size_t i = threadIdx.x; i < width; i += kThreads) plan_step(a, t, j, first + i);
        __syncthreads();
    }
}

__global__ void __launch_bounds__(kThreads) k_prune_deep_after(const PruneArgs a)
{
    const size_t bid = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
    if (bid >= ((size_t)a.T << a.top)) return;
    const size_t t = bid >> a.top, g0 = bid & (((size_t)1 << a.top) - 1);
    AfterSums sums = {0u, 0u, 0u};
    for (int j = a.top; j < a.D; ++j) {
        const size_t width = (size_t)1 << (j - a.top), first = g0 << (j - a.top);
        int any = 0;
        for (size_t i = threadIdx.x; i < width; i += kThreads) any |= after_step(a, t, j, first + i, sums) ? 1 : 0;
        if (!__syncthreads_or(any)) break;
    }
    add_after_sums(a, sums);
}

// Rule P3 for the nodes that stay: a "go on" side whose child collapses becomes a leaf slot with the child's counts.
__global__ void __launch_bounds__(kThreads) k_prune_fold(const PruneArgs a)
{
    const int C = a.C;
    const size_t inner = a.N() >> 1;                    // the nodes that have children
    const size_t idx = ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * kThreads + threadIdx.x;
    if (idx >= inner * (size_t)a.T) return;
    const size_t t = idx / inner, n = idx - t * inner;
    if (!(a.state[a.at(t, n)] & kReachAfter)) return;
    float *rec = a.forest + a.rec(t, n);
    for (int s = 0; s < 2; ++s) {
        const size_t c = 2 * n + 1 + s;
        if (is_leaf_slot(rec, s) || !(a.state[a.at(t, c)] & kCollapse)) continue;
        const u64 *own = a.sub + a.row(t, c);
        u64 *cnt = a.counts + a.cell(t, n, s);
        for (int k = 0; k < C; ++k) cnt[k] = own[k];
        // the nearest of c (of level floor(log2(c + 1))), parent(c), ..., root with a pixel below it; zeros when there is none
        const SubRow src = nearest_ancestor(a, a.sub, t, c, 63 - __clzll((long long)(c + 1)), 1ull);
        float *pdf = rec + 7 + s * C;
        if (src.row) write_pdf(pdf, src.row, src.sum, C);
        else for (int k = 0; k < C; ++k) pdf[k] = 0.f;
        rec[5 + s] = 0.f;
    }
}

// Rule P3 for the nodes that do not stay: records of +0.0f, counts of 0.  A workgroup takes 256 consecutive nodes (of all
// trees as one run); its lanes go over their floats and counts in address order.
__global__ void __launch_bounds__(kThreads) k_prune_clear(const PruneArgs a)
{
    __shared__ uint8_t gone[kThreads];
    const uint32_t E = (uint32_t)a.E(), K = 2u * (uint32_t)a.C;
    const size_t all = a.nodes(), n0 = ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * kThreads;
    if (n0 >= all) return;                              // (the workgroup as one)
    const uint32_t have = all - n0 < (size_t)kThreads ? (uint32_t)(all - n0) : (uint32_t)kThreads;
    const bool g = threadIdx.x < have && !(a.state[n0 + threadIdx.x] & kReachAfter);
    gone[threadIdx.x] = g ? 1 : 0;
    if (!__syncthreads_or(g ? 1 : 0)) return;
    float *recs = a.forest + n0 * E;
    for (uint32_t i = threadIdx.x; i < have * E; i += kThreads)
        if (gone[i / E]) recs[i] = 0.f;
    u64 *cnts = a.counts + n0 * K;
    for (uint32_t i = threadIdx.x; i < have * K; i += kThreads)
        if (gone[i / K]) cnts[i] = 0ull;
}

size_t state_bytes(size_t nodes) { return (nodes + 7) & ~(size_t)7; }

// the workspace: state bytes, then sub, then meta
void carve(PruneArgs &a, void *workspace)
{
    const size_t nodes = a.nodes();
    uint8_t *p = reinterpret_cast<uint8_t *>(workspace);
    a.state = p;
    a.sub = reinterpret_cast<u64 *>(p + state_bytes(nodes));
    a.meta = reinterpret_cast<Meta *>(p + state_bytes(nodes) + nodes * (size_t)a.C * sizeof(u64));
    a.top = 1;
    while (a.top < a.D && ((long long)a.T << a.top) <= kTopThreads) ++a.top;
}

// n workgroups as a grid of at most 2^16 - 1 rows of 2^15
dim3 grid_of(size_t n)
{
    const size_t row = (size_t)1 << 15;
    return n <= row ? dim3((unsigned)n) : dim3((unsigned)row, (unsigned)((n + row - 1) / row));
}

}  // namespace

extern "C" {

size_t rdf_labels_prune_workspace_bytes(int n_trees, int max_depth, int n_classes)
{
    if (bad_forest_shape(n_trees, max_depth, n_classes)) return 0;
    const size_t nodes = ForestShape{n_trees, max_depth, n_classes}.nodes();
    return state_bytes(nodes) + nodes * (size_t)n_classes * sizeof(uint64_t) + nodes * sizeof(Meta);
}

int rdf_labels_prune_plan(const float *forest, int n_trees, int max_depth, int n_classes, const uint64_t *counts,
                          uint64_t cost_per_leaf, uint64_t min_count, int max_levels, void *workspace, uint64_t *report,
                          void *stream)
{
    if (bad_forest_shape(n_trees, max_depth, n_classes) || cost_per_leaf >= (1ull << 32) || max_levels < 1 || max_levels > max_depth)
        return RDF_ERR_BAD_ARG;
    if (!forest || !counts || !workspace || !report) return RDF_ERR_NULL_PTR;
    if (misaligned(forest, 4) || misaligned(counts, 8) || misaligned(workspace, 8) || misaligned(report, 8)) return RDF_ERR_BAD_ARG;

    PruneArgs a = {{n_trees, max_depth, n_classes}};
    a.forest = const_cast<float *>(forest);             // (no kernel of the plan writes through it)
    a.counts = reinterpret_cast<u64 *>(const_cast<uint64_t *>(counts));
    a.report = reinterpret_cast<u64 *>(report);
    a.max_levels = max_levels;
    a.cost = cost_per_leaf;
    a.min_count = min_count;
    carve(a, workspace);
    hipStream_t s = S(stream);
    hipError_t err = hipMemsetAsync(report, 0, 8 * sizeof(uint64_t), s);
    if (err != hipSuccess) return (int)err;
    err = hipMemsetAsync(a.state, 0, state_bytes(a.nodes()), s);
    if (err != hipSuccess) return (int)err;
    const bool deep = a.top < max_depth;
    const dim3 roots = grid_of((size_t)n_trees << a.top);
    hipLaunchKernelGGL(k_prune_top_reach, dim3(1), dim3(kTopThreads), 0, s, a);
    if (deep) hipLaunchKernelGGL(k_prune_deep_up, roots, dim3(kThreads), 0, s, a);
    hipLaunchKernelGGL(k_prune_top_plan, dim3(1), dim3(kTopThreads), 0, s, a);
    if (deep) hipLaunchKernelGGL(k_prune_deep_after, roots, dim3(kThreads), 0, s, a);
    return (int)hipGetLastError();
}

int rdf_labels_prune_apply(float *forest, int n_trees, int max_depth, int n_classes, uint64_t *counts, const void *workspace,
                           void *stream)
{
    if (bad_forest_shape(n_trees, max_depth, n_classes)) return RDF_ERR_BAD_ARG;
    if (!forest || !counts || !workspace) return RDF_ERR_NULL_PTR;
    if (misaligned(forest, 4) || misaligned(counts, 8) || misaligned(workspace, 8)) return RDF_ERR_BAD_ARG;

    PruneArgs a = {{n_trees, max_depth, n_classes}};     // (report, cost and min_count, the plan's: zero)
    a.forest = forest;
    a.counts = reinterpret_cast<u64 *>(counts);
    a.max_levels = max_depth;
    carve(a, const_cast<void *>(workspace));
    hipStream_t s = S(stream);
    if (max_depth > 1)
        hipLaunchKernelGGL(k_prune_fold, grid_of(((a.N() >> 1) * (size_t)n_trees + kThreads - 1) / kThreads), dim3(kThreads), 0, s, a);
    hipLaunchKernelGGL(k_prune_clear, grid_of((a.nodes() + kThreads - 1) / kThreads), dim3(kThreads), 0, s, a);
    return (int)hipGetLastError();
}

}  // extern "C"
