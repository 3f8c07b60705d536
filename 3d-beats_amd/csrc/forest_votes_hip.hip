// forest_votes_hip.hip -- joint votes: a second use of a trained forest's structure.  Every leaf slot stores, per joint, a
// depth-normalised offset towards that joint; every hand pixel of a frame, whatever its label, casts its leaves' votes into a
// coarse accumulator per (frame, joint), and the joint is the accumulator's mode.  rdf_labels_votes_count walks labelled frames
// and sums offsets per (tree, node, side, joint) in 64-bit integers, rdf_labels_votes_fit turns the sums into a vote table,
// rdf_labels_votes_cast casts the table's votes for any number of frames and finds the modes.  Built into librdf_labels.so.
// The forest's layout, the flag rule and the walk (walk_tree) are in rdf_forest_ref.hpp, shared with the refit, the pruning and
// the posterior.  The contract (rules V) is in include/rdf_labels.h and tests/votes_numpy.py restates it; everything is integer
// arithmetic, so no result depends on the order in which pixels are visited and two runs give the same bytes.
//
// k_votes_count: one lane per pixel, a wave takes 64 consecutive pixels and leaves at once when none of them carries a label,
// as k_refit_count.  A lane walks the trees one after the other; at_leaf only records the slot, the per-joint sums follow the
// walk: five 64-bit atomics per (pixel, tree, joint in reach), straight into sums.  totals stay in lane registers and are summed
// once per wave.
// k_votes_fit: a lane owns a node, learns whether it is reachable by climbing to the root (at most D - 1 flags), and writes the
// 2 J entries of the node with one 16-byte store each: one launch whatever the depth, no workspace.
// k_votes_cast: one lane per label pixel, as k_posterior: a wave leaves at once when none of its pixels takes part.  After each
// tree's walk a lane reads the J votes of its slot, one 16-byte load each, and adds w and w * vz to the cell the vote lands in:
// two global atomics a vote.  (Merging the equal cells of a wave with wave_key_group before the atomics gives the same bytes; it
// was measured and does not pay with the tables the default fit makes: DESIGN.md, profiles/joint_votes_merge_ab.txt.)
// k_votes_modes: one workgroup per (frame, joint).  Thread t takes cells t, t + 256, ... in ascending order, sums each cell's
// box straight from acc and keeps the first largest sum; a tree reduction in LDS keeps the lowest index among equal sums;
// thread 0 then takes the centroid over the winner's box (81 cells at most).  Every thread meets the same barriers.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/rdf_labels.h"
#include "rdf_forest_ref.hpp"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxBlocks = 1024;      // count and fit: larger calls stride over the grid
constexpr int kMaxModeBlocks = 65536; // modes: more (frame, joint) pairs than this stride over the grid

__device__ __forceinline__ long long floordiv64(long long a, long long b)      // b > 0
{
    long long q = a / b;
    if (a % b != 0 && a < 0) --q;
    return q;
}

__device__ __forceinline__ bool joint_absent(int tz) { return tz <= 0 || tz >= 65535; }

// ---- V1 ----
struct VoteCountArgs : ForestShape {
    const uint16_t *depth, *labels;
    const int32_t *targets;
    uint32_t n_px, pix;               // all pixels (< 2^31), pixels of one image
    int W, H, J, radius;
    const float *forest;
    float scale;
    u64 *sums, *totals;
};

__global__ void __launch_bounds__(kThreads) k_votes_count(const VoteCountArgs a)
{
    const int tid = threadIdx.x, lane = tid & 63;
    const int J = a.J;
    uint32_t n_walked = 0u, n_no_depth = 0u, n_fell = 0u, n_added = 0u;
    // (no bound depends on the lane: every lane of a wave makes the same trips, as the ballots and shuffles need)
    for (uint32_t i0 = (blockIdx.x * (uint32_t)kThreads + (uint32_t)tid) - (uint32_t)lane; i0 < a.n_px;
         i0 += gridDim.x * (uint32_t)kThreads) {
        const uint32_t i = i0 + (uint32_t)lane;
        const uint32_t l = i < a.n_px ? (uint32_t)a.labels[i] : 0u;
        if (__ballot(l != 0u) == 0ull) continue;                    // (most of a frame is no hand)
        bool live = false;
        uint32_t d = 1u;
        if (l != 0u) {
            d = a.depth[i];
            if (d == 0u || d == kNoPixel) {
                ++n_no_depth;
            } else {
                live = true;
                ++n_walked;
            }
        }
        if (__ballot(live) == 0ull) continue;
        const uint32_t img = i < a.n_px ? i / a.pix : 0u, rem = i < a.n_px ? i - img * a.pix : 0u;
        const int y = (int)(rem / (uint32_t)a.W), x = (int)(rem - (uint32_t)y * (uint32_t)a.W);
        const WalkPixel p = {a.depth + (size_t)img * a.pix, a.W, a.H, x, y, (float)d, a.scale};
        const int32_t *__restrict__ tg = a.targets + (size_t)img * (size_t)J * 3;

        for (int t = 0; t < a.T; ++t) {
            uint32_t slot = 0u;
            bool has = false;
            walk_tree(a.forest + a.rec(t, 0), a.D, a.E(), p, live,
                      [&](int, uint32_t n, uint32_t side, const float *) {
                          has = true;
                          slot = n * 2u + side;
                      },
                      [&] { ++n_fell; });
            if (has) {
                u64 *__restrict__ cell = a.sums + (a.at(t, 0) * 2 + slot) * (size_t)J * 5;
                for (int j = 0; j < J; ++j) {
                    const int tx = tg[3 * j], ty = tg[3 * j + 1], tz = tg[3 * j + 2];
                    if (joint_absent(tz)) continue;
                    const long long dx = (long long)tx - x, dy = (long long)ty - y;
                    if (dx < -a.radius || dx > a.radius || dy < -a.radius || dy > a.radius) continue;
                    // |dx d| < 2^24; an arithmetic shift is the floor division by 64
                    const int ox = ((int)dx * (int)d) >> 6, oy = ((int)dy * (int)d) >> 6, oz = tz - (int)d;
                    u64 *__restrict__ w = cell + (size_t)j * 5;
                    atomicAdd(w + 0, 1ull);
                    atomicAdd(w + 1, (u64)(long long)ox);           // two's complement: the add wraps as the signed sum does
                    atomicAdd(w + 2, (u64)(long long)oy);
                    atomicAdd(w + 3, (u64)(long long)oz);
                    atomicAdd(w + 4, (u64)((long long)ox * ox + (long long)oy * oy));
                    ++n_added;
                }
            }
        }
    }
    const uint32_t w = wave_sum(n_walked), z = wave_sum(n_no_depth), o = wave_sum(n_fell), s = wave_sum(n_added);
    if (lane == 0) {
        if (w) atomicAdd(a.totals + 0, (u64)w);
        if (z) atomicAdd(a.totals + 1, (u64)z);
        if (o) atomicAdd(a.totals + 2, (u64)o);
        if (s) atomicAdd(a.totals + 3, (u64)s);
    }
}

// ---- V2 ----
struct VoteFitArgs : ForestShape {
    const float *forest;
    const u64 *sums;
    int4 *votes;
    u64 *report;
    int J;
    u64 min_count, max_var;
};

__global__ void __launch_bounds__(kThreads) k_votes_fit(const VoteFitArgs a)
{
    const int tid = threadIdx.x, lane = tid & 63;
    const int J = a.J;
    const size_t nodes = a.nodes(), N = a.N();
    uint32_t n_slots = 0u, n_votes = 0u, n_support = 0u, n_spread = 0u;
    // (no bound depends on the lane: the wave sums below take all 64)
    for (size_t i0 = ((size_t)blockIdx.x * kThreads + (size_t)tid) - (size_t)lane; i0 < nodes; i0 += (size_t)gridDim.x * kThreads) {
        const size_t idx = i0 + (size_t)lane;
        if (idx >= nodes) continue;
        const size_t t = idx / N, n = idx - t * N;
        const float *__restrict__ rec = a.forest + a.rec(t, n);
        bool reachable = true;
        for (size_t c = n; c != 0 && reachable;) {                  // up to the root: every flag on the way says "go on"
            const size_t parent = (c - 1) >> 1;
            reachable = !is_leaf_slot(a.forest + a.rec(t, parent), (uint32_t)(c - 1) & 1u);
            c = parent;
        }
        for (uint32_t s = 0; s < 2u; ++s) {
            const bool leaf = reachable && is_leaf_slot(rec, s);
            if (leaf) ++n_slots;
            const u64 *__restrict__ src = a.sums + (idx * 2 + s) * (size_t)J * 5;
            int4 *__restrict__ dst = a.votes + (idx * 2 + s) * (size_t)J;
            for (int j = 0; j < J; ++j) {
                int4 e = make_int4(0, 0, 0, 0);
                if (leaf) {
                    const u64 cnt = src[5 * j];
                    if (cnt < a.min_count || cnt >= (1ull << 26)) {
                        ++n_support;
                    } else {
                        const long long mx = floordiv64((long long)src[5 * j + 1], (long long)cnt);
                        const long long my = floordiv64((long long)src[5 * j + 2], (long long)cnt);
                        const long long mz = floordiv64((long long)src[5 * j + 3], (long long)cnt);
                        const u64 q = src[5 * j + 4] / cnt, m2 = (u64)mx * (u64)mx + (u64)my * (u64)my;
                        const u64 var = q > m2 ? q - m2 : 0ull;
                        if (var > a.max_var) {
                            ++n_spread;
                        } else {
                            ++n_votes;
                            e = make_int4((int)mx, (int)my, (int)mz, 256 - (int)((var * 256ull) / (a.max_var + 1ull)));
                        }
                    }
                }
                dst[j] = e;
            }
        }
    }
    const uint32_t ls = wave_sum(n_slots), v = wave_sum(n_votes), su = wave_sum(n_support), sp = wave_sum(n_spread);
    if (lane == 0) {
        if (ls) atomicAdd(a.report + 0, (u64)ls);
        if (v) atomicAdd(a.report + 1, (u64)v);
        if (su) atomicAdd(a.report + 2, (u64)su);
        if (sp) atomicAdd(a.report + 3, (u64)sp);
    }
}

// ---- V3, V4 ----
struct VoteCastArgs : ForestShape {
    const uint16_t *depth, *gate;
    const float *forest;
    const int4 *votes;
    uint32_t *acc;
    u64 *zacc;
    uint32_t n_lpx, lpix, pix;        // label pixels of the call (< 2^31) and of one image, depth pixels of one image
    int W, H, Wl, r, J, shift, Wa, Ha;
    float scale;
};

// floordiv(128 m + d, 2 d): the inverse of V1's normalisation, rounded half up.  A table that rdf_labels_votes_fit made has
// |m| < 2^18, so the 32-bit division is the one taken; any int32 m is divided correctly.
__device__ __forceinline__ long long vote_pixels(int m, int d)
{
    const long long num = 128ll * m + d;
    const int den = 2 * d;
    if (num >= -2147483647ll && num <= 2147483647ll) {
        const int n32 = (int)num;
        int q = n32 / den;
        if (n32 % den != 0 && n32 < 0) --q;
        return q;
    }
    return floordiv64(num, den);
}

__global__ void __launch_bounds__(kThreads) k_votes_cast(const VoteCastArgs a)
{
    const uint32_t i = blockIdx.x * (uint32_t)kThreads + threadIdx.x;
    const bool inside = i < a.n_lpx;
    const uint32_t img = inside ? i / a.lpix : 0u, rem = inside ? i - img * a.lpix : 0u;
    const uint32_t yl = rem / (uint32_t)a.Wl, xl = rem - yl * (uint32_t)a.Wl;
    const int x = (int)(xl * (uint32_t)a.r), y = (int)(yl * (uint32_t)a.r);
    const uint16_t *__restrict__ frame = a.depth + (size_t)img * a.pix;
    // V3: the gate first, then the pixel's own depth
    bool live = inside;
    if (live && a.gate) {
        const uint32_t g = a.gate[i];
        live = g != 0u && g != kNoPixel;
    }
    uint32_t d = 1u;
    if (live) {
        d = frame[(uint32_t)y * (uint32_t)a.W + (uint32_t)x];
        live = d != 0u && d != kNoPixel;
    }
    if (__ballot(live) == 0ull) return;                             // (most of a frame is no hand)

    const int J = a.J;
    const size_t plane = (size_t)a.Ha * (size_t)a.Wa;
    const WalkPixel p = {frame, a.W, a.H, x, y, (float)d, a.scale};
    for (int t = 0; t < a.T; ++t) {
        uint32_t slot = 0u;
        bool has = false;
        walk_tree(a.forest + a.rec(t, 0), a.D, a.E(), p, live,
                  [&](int, uint32_t n, uint32_t side, const float *) {
                      has = true;
                      slot = n * 2u + side;
                  },
                  [] {});
        if (!has) continue;
        const int4 *__restrict__ v = a.votes + (a.at(t, 0) * 2 + slot) * (size_t)J;
        for (int j = 0; j < J; ++j) {
            const int4 e = v[j];                                    // (mx, my, mz, w): one 16-byte load
            if (e.w < 1 || e.w > 256) continue;
            const long long vx = (long long)x + vote_pixels(e.x, (int)d), vy = (long long)y + vote_pixels(e.y, (int)d);
            const long long vz = (long long)d + e.z;
            if (vx < 0 || vx >= a.W || vy < 0 || vy >= a.H || vz < 1 || vz > 65534) continue;
            const size_t cell = ((size_t)img * (size_t)J + (size_t)j) * plane +
                                (size_t)((uint32_t)vy >> a.shift) * (size_t)a.Wa + (size_t)((uint32_t)vx >> a.shift);
            atomicAdd(a.acc + cell, (uint32_t)e.w);
            atomicAdd(a.zacc + cell, (u64)(uint32_t)e.w * (u64)vz);
        }
    }
}

// ---- V5 ----
struct VoteModesArgs {
    const uint32_t *acc;
    const u64 *zacc;
    int4 *out;
    uint32_t n_pairs;                 // (frame, joint) pairs
    int Wa, Ha, shift, box;
    uint32_t min_support;
};

__global__ void __launch_bounds__(kThreads) k_votes_modes(const VoteModesArgs a)
{
    __shared__ u64 s_best[kThreads];
    __shared__ uint32_t s_at[kThreads];
    const int tid = threadIdx.x;
    const int Wa = a.Wa, Ha = a.Ha, b = a.box;
    const uint32_t cells = (uint32_t)Wa * (uint32_t)Ha;             // < 2^32: both dimensions are below 2^16
    // (the bounds are the workgroup's: every thread makes the same trips and meets the same barriers)
    for (uint32_t pair = blockIdx.x; pair < a.n_pairs; pair += gridDim.x) {
        const uint32_t *__restrict__ acc = a.acc + (size_t)pair * cells;
        u64 best = 0ull;
        uint32_t at = 0xffffffffu;
        for (uint32_t c = (uint32_t)tid; c < cells; c += (uint32_t)kThreads) {     // ascending: the first largest stays
            const int cy = (int)(c / (uint32_t)Wa), cx = (int)(c - (uint32_t)cy * (uint32_t)Wa);
            const int y0 = cy - b < 0 ? 0 : cy - b, y1 = cy + b > Ha - 1 ? Ha - 1 : cy + b;
            const int x0 = cx - b < 0 ? 0 : cx - b, x1 = cx + b > Wa - 1 ? Wa - 1 : cx + b;
            u64 S = 0ull;
            for (int yy = y0; yy <= y1; ++yy)
                for (int xx = x0; xx <= x1; ++xx) S += acc[(size_t)yy * Wa + xx];
            if (S > best) {
                best = S;
                at = c;
            }
        }
        s_best[tid] = best;
        s_at[tid] = at;
        __syncthreads();
        for (int s = kThreads / 2; s > 0; s >>= 1) {
            if (tid < s) {
                const u64 ob = s_best[tid + s];
                const uint32_t oa = s_at[tid + s];
                if (ob > s_best[tid] || (ob == s_best[tid] && oa < s_at[tid])) {
                    s_best[tid] = ob;
                    s_at[tid] = oa;
                }
            }
            __syncthreads();
        }
        if (tid == 0) {
            best = s_best[0];
            at = s_at[0];
            int4 e = make_int4(-1, -1, 0, 0);
            if (best >= (u64)(a.min_support > 1u ? a.min_support : 1u)) {
                const u64 *__restrict__ zacc = a.zacc + (size_t)pair * cells;
                const int cy = (int)(at / (uint32_t)Wa), cx = (int)(at - (uint32_t)cy * (uint32_t)Wa);
                const int y0 = cy - b < 0 ? 0 : cy - b, y1 = cy + b > Ha - 1 ? Ha - 1 : cy + b;
                const int x0 = cx - b < 0 ? 0 : cx - b, x1 = cx + b > Wa - 1 ? Wa - 1 : cx + b;
                const u64 half = 8ull << a.shift;                   // a cell's centre, in 1/16 pixel
                u64 sx = 0ull, sy = 0ull, sz = 0ull;
                for (int yy = y0; yy <= y1; ++yy)
                    for (int xx = x0; xx <= x1; ++xx) {
                        const u64 w = acc[(size_t)yy * Wa + xx];
                        sx += w * (16ull * ((u64)xx << a.shift) + half);
                        sy += w * (16ull * ((u64)yy << a.shift) + half);
                        sz += zacc[(size_t)yy * Wa + xx];
                    }
                e = make_int4((int)(sx / best), (int)(sy / best), (int)(sz / best), best > 2147483647ull ? 2147483647 : (int)best);
            }
            a.out[pair] = e;
        }
        __syncthreads();                                            // s_best[0] is read before the next pair writes it
    }
}

inline bool bad_joints(int n_joints) { return n_joints < 1 || n_joints > RDF_VOTES_MAX_JOINTS; }
inline bool sums_too_large(const ForestShape &f, int n_joints) { return (u64)f.N() * 2ull * (u64)n_joints * 5ull >= (1ull << 32); }

}  // namespace

extern "C" {

int rdf_labels_votes_count(const uint16_t *depth, const uint16_t *labels, const int32_t *targets, int n_img, int dim_x, int dim_y,
                           const float *forest, int n_trees, int max_depth, int n_classes, float scale_factor, int n_joints,
                           int radius, uint64_t *sums, uint64_t *totals, void *stream)
{
    if (n_img < 0 || dim_x < 0 || dim_y < 0 || bad_forest_shape(n_trees, max_depth, n_classes) || bad_joints(n_joints) ||
        radius < 0 || radius > RDF_VOTES_MAX_RADIUS)
        return RDF_ERR_BAD_ARG;
    VoteCountArgs a = {{n_trees, max_depth, n_classes}};
    if (sums_too_large(a, n_joints)) return RDF_ERR_TOO_LARGE;
    if (n_img == 0 || dim_x == 0 || dim_y == 0) return RDF_OK;
    if (!depth || !labels || !targets || !forest || !sums || !totals) return RDF_ERR_NULL_PTR;
    const long long pix = (long long)dim_x * dim_y;
    if (pix >= (1ll << 31) || pix * n_img >= (1ll << 31)) return RDF_ERR_TOO_LARGE;
    if (misaligned(depth, 2) || misaligned(labels, 2) || misaligned(targets, 4) || misaligned(forest, 4) || misaligned(sums, 8) ||
        misaligned(totals, 8))
        return RDF_ERR_BAD_ARG;

    a.depth = depth;
    a.labels = labels;
    a.targets = targets;
    a.n_px = (uint32_t)(pix * n_img);
    a.pix = (uint32_t)pix;
    a.W = dim_x;
    a.H = dim_y;
    a.J = n_joints;
    a.radius = radius;
    a.forest = forest;
    a.scale = scale_factor;
    a.sums = reinterpret_cast<u64 *>(sums);
    a.totals = reinterpret_cast<u64 *>(totals);
    unsigned grid = blocks(a.n_px, kThreads);
    grid = grid > (unsigned)kMaxBlocks ? (unsigned)kMaxBlocks : grid;
    hipLaunchKernelGGL(k_votes_count, dim3(grid), dim3(kThreads), 0, S(stream), a);
    return (int)hipGetLastError();
}

int rdf_labels_votes_fit(const float *forest, int n_trees, int max_depth, int n_classes, int n_joints, const uint64_t *sums,
                         uint64_t min_count, uint64_t max_var, int32_t *votes, uint64_t *report, void *stream)
{
    if (bad_forest_shape(n_trees, max_depth, n_classes) || bad_joints(n_joints) || min_count < 1 || max_var > (1ull << 38))
        return RDF_ERR_BAD_ARG;
    VoteFitArgs a = {{n_trees, max_depth, n_classes}};
    if (sums_too_large(a, n_joints)) return RDF_ERR_TOO_LARGE;
    if (!forest || !sums || !votes || !report) return RDF_ERR_NULL_PTR;
    if (misaligned(forest, 4) || misaligned(sums, 8) || misaligned(votes, 16) || misaligned(report, 8)) return RDF_ERR_BAD_ARG;

    a.forest = forest;
    a.sums = reinterpret_cast<const u64 *>(sums);
    a.votes = reinterpret_cast<int4 *>(votes);
    a.report = reinterpret_cast<u64 *>(report);
    a.J = n_joints;
    a.min_count = min_count;
    a.max_var = max_var;
    hipStream_t s = S(stream);
    hipError_t err = hipMemsetAsync(report, 0, 4 * sizeof(uint64_t), s);
    if (err != hipSuccess) return (int)err;
    const size_t want = (a.nodes() + kThreads - 1) / kThreads;
    hipLaunchKernelGGL(k_votes_fit, dim3(want > (size_t)kMaxBlocks ? (unsigned)kMaxBlocks : (unsigned)want), dim3(kThreads), 0, s, a);
    return (int)hipGetLastError();
}

size_t rdf_labels_votes_workspace_bytes(int n_img, int dim_x, int dim_y, int n_joints, int cell_shift)
{
    if (n_img < 0 || dim_x < 0 || dim_y < 0 || dim_x > 65535 || dim_y > 65535 || bad_joints(n_joints) || cell_shift < 0 ||
        cell_shift > RDF_VOTES_MAX_CELL_SHIFT)
        return 0;
    const size_t Wa = (size_t)(((dim_x - 1) >> cell_shift) + 1), Ha = (size_t)(((dim_y - 1) >> cell_shift) + 1);
    const size_t cells = (size_t)n_img * (size_t)n_joints * Ha * Wa;
    return cells * sizeof(uint64_t) + ((cells * sizeof(uint32_t) + 7) & ~(size_t)7);
}

int rdf_labels_votes_cast(const uint16_t *depth, int n_img, int dim_x, int dim_y, const uint16_t *gate, int labels_reduce,
                          const float *forest, int n_trees, int max_depth, int n_classes, float scale_factor, const int32_t *votes,
                          int n_joints, int cell_shift, int box, uint32_t min_support, void *workspace, int32_t *joints_out,
                          void *stream)
{
    if (n_img < 0 || dim_x < 0 || dim_y < 0 || labels_reduce < 1 || bad_forest_shape(n_trees, max_depth, n_classes) ||
        bad_joints(n_joints) || cell_shift < 0 || cell_shift > RDF_VOTES_MAX_CELL_SHIFT || box < 0 || box > RDF_VOTES_MAX_BOX)
        return RDF_ERR_BAD_ARG;
    if (misaligned(depth, 2) || misaligned(gate, 2) || misaligned(forest, 4) || misaligned(votes, 16) || misaligned(workspace, 8) ||
        misaligned(joints_out, 16))
        return RDF_ERR_BAD_ARG;
    const long long pix = (long long)dim_x * dim_y;
    const long long Wl = dim_x / labels_reduce, Hl = dim_y / labels_reduce;
    if (dim_x > 65535 || dim_y > 65535 || pix * n_img >= (1ll << 31) || (long long)n_img * n_joints >= (1ll << 31) ||
        (u64)Hl * (u64)Wl * (u64)n_trees * 256ull >= (1ull << 32))
        return RDF_ERR_TOO_LARGE;
    if (n_img == 0) return RDF_OK;
    if (!depth || !forest || !votes || !workspace || !joints_out) return RDF_ERR_NULL_PTR;

    VoteCastArgs a = {{n_trees, max_depth, n_classes}};
    a.Wa = dim_x > 0 ? ((dim_x - 1) >> cell_shift) + 1 : 0;
    a.Ha = dim_y > 0 ? ((dim_y - 1) >> cell_shift) + 1 : 0;
    const size_t cells = (size_t)n_img * (size_t)n_joints * (size_t)a.Ha * (size_t)a.Wa;
    a.zacc = reinterpret_cast<u64 *>(workspace);
    a.acc = reinterpret_cast<uint32_t *>(a.zacc + cells);
    hipStream_t s = S(stream);
    const size_t bytes = rdf_labels_votes_workspace_bytes(n_img, dim_x, dim_y, n_joints, cell_shift);
    if (bytes) {
        hipError_t err = hipMemsetAsync(workspace, 0, bytes, s);
        if (err != hipSuccess) return (int)err;
    }
    a.depth = depth;
    a.gate = gate;
    a.forest = forest;
    a.votes = reinterpret_cast<const int4 *>(votes);
    a.lpix = (uint32_t)(Wl * Hl);
    a.n_lpx = a.lpix * (uint32_t)n_img;
    a.pix = (uint32_t)pix;
    a.W = dim_x;
    a.H = dim_y;
    a.Wl = (int)Wl;
    a.r = labels_reduce;
    a.J = n_joints;
    a.shift = cell_shift;
    a.scale = scale_factor;
    if (a.n_lpx) hipLaunchKernelGGL(k_votes_cast, dim3(blocks(a.n_lpx, kThreads)), dim3(kThreads), 0, s, a);

    VoteModesArgs m;
    m.acc = a.acc;
    m.zacc = a.zacc;
    m.out = reinterpret_cast<int4 *>(joints_out);
    m.n_pairs = (uint32_t)n_img * (uint32_t)n_joints;               // < 2^31: checked above
    m.Wa = a.Wa;
    m.Ha = a.Ha;
    m.shift = cell_shift;
    m.box = box;
    m.min_support = min_support;
    const unsigned grid = m.n_pairs > (uint32_t)kMaxModeBlocks ? (unsigned)kMaxModeBlocks : (unsigned)m.n_pairs;
    hipLaunchKernelGGL(k_votes_modes, dim3(grid), dim3(kThreads), 0, s, m);
    return (int)hipGetLastError();
}

}  // extern "C"
