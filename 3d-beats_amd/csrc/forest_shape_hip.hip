// forest_shape_hip.hip -- the hand's shape from the forest's pooled votes: where rdf_labels_forest_posterior writes a pixel's
// class sums to a map, rdf_labels_shape_pool turns them into 16-bit shares of the pixel's vote and adds the shares of all the
// pixels of a frame into one row of 64-bit words; rdf_labels_shape_decide names the class with the greatest pooled share and
// keeps a decision that changes only after `hold` agreeing frames.  Built into librdf_labels.so.  The contract (rules G) is in
// include/rdf_labels.h and tests/shape_numpy.py restates it: a pixel's sums are made in a stated order, everything that is
// added across pixels is an integer, so the pool is the same bytes in any visiting order.
//
// k_shape_pool: k_posterior's front -- one lane per label pixel, a wave takes 64 consecutive label pixels and leaves at once
// when none of them is to be evaluated, walk_tree of rdf_forest_ref.hpp, the C sums in registers through the class-capacity
// template (4, 8, 16; every class loop unrolled and guarded by c < C, nothing in scratch).  Behind the walk the wave reduces
// before it touches memory: the lanes of one image (a wave-uniform group, wave_key_group of rdf_kernel_util.hpp; one group
// unless the wave straddles two images, then one group an image) sum each class's shares with the xor-shuffle wave_sum -- 64
// shares of at most 65535 fit 32 bits -- and count the hard votes and the live and dead pixels with ballots; lane w of the
// wave keeps word w of the row, and the lanes whose word is not zero add it with one 64-bit integer atomic each: 2C + 2
// consecutive words, one vector atomic instruction a wave and image.  No LDS, no floating-point atomics.
//
// k_shape_decide: one lane.  The frames of a call are a sequence (rule G7's state runs from frame to frame) and few.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/rdf_labels.h"
#include "rdf_forest_ref.hpp"

namespace {

constexpr int kThreads = 256;

struct PoolArgs : ForestShape {
    const uint16_t *depth, *filter;
    const float *forest;
    u64 *pool;
    uint32_t n_lpx, lpix, pix;        // label pixels of the call (< 2^31) and of one image, depth pixels of one image
    int W, H, Wl, r;
    int filter_class;
    float scale;
};

template <int CAP>
__global__ void __launch_bounds__(kThreads) k_shape_pool(const PoolArgs a)
{
    const uint32_t i = blockIdx.x * (uint32_t)kThreads + threadIdx.x;
    const int lane = (int)(threadIdx.x & 63u);
    const bool inside = i < a.n_lpx;
    const uint32_t img = inside ? i / a.lpix : 0u, rem = inside ? i - img * a.lpix : 0u;
    const uint32_t yl = rem / (uint32_t)a.Wl, xl = rem - yl * (uint32_t)a.Wl;
    const int x = (int)(xl * (uint32_t)a.r), y = (int)(yl * (uint32_t)a.r);
    const uint16_t *__restrict__ frame = a.depth + (size_t)img * a.pix;
    // G1: the filter first, then the pixel's own depth
    bool live = inside;
    if (live && a.filter_class != -1) live = (int)a.filter[i] == a.filter_class;
    uint32_t d = 1u;
    if (live) {
        d = frame[(uint32_t)y * (uint32_t)a.W + (uint32_t)x];
        live = d != 0u && d != kNoPixel;
    }
    if (__ballot(live) == 0ull) return;                             // (most of a frame is background)

    const int C = a.C;
    const WalkPixel p = {frame, a.W, a.H, x, y, (float)d, a.scale};
    float acc[CAP];
#pragma unroll
    for (int c = 0; c < CAP; ++c) acc[c] = 0.f;

    // G2: rule Q2's sums
    for (int t = 0; t < a.T; ++t)
        walk_tree(a.forest + a.rec(t, 0), a.D, a.E(), p, live,
                  [&](int, uint32_t, uint32_t side, const float *__restrict__ rec) {
                      const float *__restrict__ pdf = rec + 7 + side * (uint32_t)C;
#pragma unroll
                      for (int c = 0; c < CAP; ++c)
                          if (c < C) acc[c] = acc[c] + pdf[c];
                  },
                  [] {});

    // Q3's label and Q4's S
    float best = 0.f, S = 0.f;
    int label = 0;
#pragma unroll
    for (int c = 0; c < CAP; ++c) {
        if (c < C) {
            if (acc[c] > best) {
                best = acc[c];
                label = c;
            }
            S = S + acc[c];
        }
    }
    // G3: the shares; a lane without a pixel and a dead pixel hold zeros
    const bool counted = live, voting = live && S > 0.f;
    uint32_t q[CAP];
#pragma unroll
    for (int c = 0; c < CAP; ++c) {
        q[c] = 0u;
        if (c < C && voting) {
            const int v = floor_i32((acc[c] / S) * 65535.0f);
            q[c] = (uint32_t)(v < 0 ? 0 : v > 65535 ? 65535 : v);
        }
    }

    // G4: one group of lanes an image (wave-uniform: every lane of the wave is here and takes every trip)
    u64 pending = __ballot(counted);
    while (pending != 0ull) {
        const KeyGroup g = wave_key_group(pending, (int)img, counted);
        const bool mine = (g.lanes >> lane) & 1ull;
        const u64 votes = __ballot(mine && voting);
        uint32_t word = 0u;                                         // lane w: word w of the row, w < 2C + 2
#pragma unroll
        for (int c = 0; c < CAP; ++c) {
            if (c < C) {
                const uint32_t sum = wave_sum(mine ? q[c] : 0u);
                const uint32_t hard = (uint32_t)__popcll(__ballot(mine && voting && label == c));
                if (lane == c) word = sum;
                if (lane == C + c) word = hard;
            }
        }
        if (lane == 2 * C) word = (uint32_t)__popcll(votes);
        if (lane == 2 * C + 1) word = (uint32_t)__popcll(g.lanes & ~votes);
        if (lane < 2 * C + 2 && word != 0u) atomicAdd(a.pool + (size_t)g.key * (size_t)(2 * C + 2) + lane, (u64)word);
        pending &= ~g.lanes;
    }
}

struct DecideArgs {
    const u64 *pool;
    int32_t *state, *out;
    int n_frames, C, min_pixels, min_conf, hold, release;
};

__global__ void __launch_bounds__(64) k_shape_decide(const DecideArgs a)
{
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const int C = a.C;
    int held = a.state[0], candidate = a.state[1], run = a.state[2], miss = a.state[3];
    for (int f = 0; f < a.n_frames; ++f) {
        const u64 *__restrict__ row = a.pool + (size_t)f * (size_t)(2 * C + 2);
        // G6
        u64 total = 0ull, best = row[0];
        int raw = 0;
        for (int c = 0; c < C; ++c) {
            const u64 v = row[c];
            total += v;
            if (v > best) {
                best = v;
                raw = c;
            }
        }
        int conf = 0;
        if (row[2 * C] < (u64)a.min_pixels || total == 0ull)
            raw = -1;
        else
            conf = (int)(best * 65535ull / total);
        // G7
        int changed = 0;
        if (raw != -1 && conf >= a.min_conf) {
            miss = 0;
            if (raw == held) {
                candidate = -1;
                run = 0;
            } else {
                if (raw == candidate) {
                    ++run;
                } else {
                    candidate = raw;
                    run = 1;
                }
                if (run >= a.hold) {
                    held = raw;
                    candidate = -1;
                    run = 0;
                    changed = 1;
                }
            }
        } else {
            candidate = -1;
            run = 0;
            if (miss < 0x7fffffff) ++miss;
            if (a.release > 0 && miss >= a.release && held != -1) {
                held = -1;
                changed = 1;
            }
        }
        int32_t *__restrict__ o = a.out + (size_t)f * 4;
        o[0] = raw;
        o[1] = conf;
        o[2] = held;
        o[3] = changed;
    }
    a.state[0] = held;
    a.state[1] = candidate;
    a.state[2] = run;
    a.state[3] = miss;
}

}  // namespace

extern "C" {

int rdf_labels_shape_pool(const uint16_t *depth, int n_img, int dim_x, int dim_y, const float *forest, int n_trees, int max_depth,
                          int n_classes, const uint16_t *filter, int filter_class, int labels_reduce, float scale_factor,
                          uint64_t *pool, void *stream)
{
    // G5
    if (n_trees < 1 || max_depth < 1 || max_depth > kMaxDepth || n_classes < 1 || n_classes > RDF_POSTERIOR_MAX_CLASSES ||
        labels_reduce < 1 || n_img < 0 || dim_x < 0 || dim_y < 0 || filter_class < -1 || filter_class > 65535)
        return RDF_ERR_BAD_ARG;
    if (misaligned(depth, 2) || misaligned(filter, 2) || misaligned(forest, 4) || misaligned(pool, 8)) return RDF_ERR_BAD_ARG;
    const long long pix = (long long)dim_x * dim_y;
    if (n_img > 0 && (pix >= (1ll << 31) || pix * n_img >= (1ll << 31))) return RDF_ERR_TOO_LARGE;
    const long long Wl = dim_x / labels_reduce, Hl = dim_y / labels_reduce;
    if (n_img == 0 || Wl == 0 || Hl == 0) return RDF_OK;
    if (!depth || !forest || !pool || (!filter && filter_class != -1)) return RDF_ERR_NULL_PTR;

    PoolArgs a = {{n_trees, max_depth, n_classes}};
    a.depth = depth;
    a.filter = filter;
    a.forest = forest;
    a.pool = reinterpret_cast<u64 *>(pool);
    a.lpix = (uint32_t)(Wl * Hl);
    a.n_lpx = a.lpix * (uint32_t)n_img;
    a.pix = (uint32_t)pix;
    a.W = dim_x;
    a.H = dim_y;
    a.Wl = (int)Wl;
    a.r = labels_reduce;
    a.filter_class = filter_class;
    a.scale = scale_factor;
    const dim3 grid(blocks(a.n_lpx, kThreads)), block(kThreads);
    if (n_classes <= 4)
        hipLaunchKernelGGL(k_shape_pool<4>, grid, block, 0, S(stream), a);
    else if (n_classes <= 8)
        hipLaunchKernelGGL(k_shape_pool<8>, grid, block, 0, S(stream), a);
    else
        hipLaunchKernelGGL(k_shape_pool<16>, grid, block, 0, S(stream), a);
    return (int)hipGetLastError();
}

int rdf_labels_shape_decide(const uint64_t *pool, int n_frames, int n_classes, int min_pixels, int min_conf, int hold,
                            int release, int32_t *state, int32_t *out, void *stream)
{
    if (n_frames < 0 || n_classes < 1 || n_classes > RDF_POSTERIOR_MAX_CLASSES || min_pixels < 0 || min_conf < 0 ||
        min_conf > 65535 || hold < 1 || release < 0)
        return RDF_ERR_BAD_ARG;
    if (misaligned(pool, 8) || misaligned(state, 4) || misaligned(out, 4)) return RDF_ERR_BAD_ARG;
    if (n_frames == 0) return RDF_OK;
    if (!pool || !state || !out) return RDF_ERR_NULL_PTR;
    DecideArgs a;
    a.pool = reinterpret_cast<const u64 *>(pool);
    a.state = state;
    a.out = out;
    a.n_frames = n_frames;
    a.C = n_classes;
    a.min_pixels = min_pixels;
    a.min_conf = min_conf;
    a.hold = hold;
    a.release = release;
    hipLaunchKernelGGL(k_shape_decide, dim3(1), dim3(64), 0, S(stream), a);
    return (int)hipGetLastError();
}

}  // extern "C"
