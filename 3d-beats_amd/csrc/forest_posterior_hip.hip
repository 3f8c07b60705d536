// forest_posterior_hip.hip -- forest posteriors: where rdf_eval_forest keeps the winning class of a pixel's summed leaf
// distributions and discards the rest, rdf_labels_forest_posterior also writes how much of the vote the winner took (a 16-bit
// confidence) and, on request, the sums themselves, and leaves a pixel whose confidence is below min_conf out of the label map.
// rdf_labels_confidence_counts bins (prediction, confidence, truth) maps into a reliability histogram.  Built into
// librdf_labels.so.  The contract (rules Q) is in include/rdf_labels.h and tests/posterior_numpy.py restates it: the sums are
// made in a stated order, so the posterior is the same bytes from run to run, and the counts are integers.
//
// k_posterior: one lane per label pixel, a wave takes 64 consecutive label pixels and leaves at once when none of them is to
// be evaluated (background, holes, filtered out: most of a live frame).  A lane walks the trees of the reference-layout
// forest one after the other with walk_tree of rdf_forest_ref.hpp, the walk that k_refit_count takes; the level loop runs while
// any lane of the wave still walks.  The C sums live in registers: the kernel is instantiated for class capacities 4, 8 and 16 and
// every class loop is unrolled over the capacity and guarded by c < C, so no register array is indexed by a runtime value
// and nothing goes to scratch.  No LDS, no atomics.  Which outputs are present is a wave-uniform test of three pointers
// (an absent output costs no store); stores are 2 bytes a lane for the two maps and one dword a lane per class plane.
//
// k_confidence_counts: one lane per label pixel and trip, a capped grid that strides over the maps; a wave whose 64 pixels
// carry no truth does nothing.  `labelled` and `unclassified` stay in lane registers and are summed once per wave; the bins go
// to a 32-bit LDS histogram (a workgroup sees < 2^31 pixels) and a workgroup adds each non-zero cell to counts once.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/rdf_labels.h"
#include "rdf_forest_ref.hpp"

namespace {

constexpr int kThreads = 256;
constexpr int kCountBlocks = 512;     // the counts kernel: larger calls stride over the grid (two workgroups a compute unit)
constexpr int kMaxBins = 1024;

struct PosteriorArgs : ForestShape {
    const uint16_t *depth, *filter;
    const float *forest;
    uint16_t *labels, *conf;
    float *sums;
    uint32_t n_lpx, lpix, pix;        // label pixels of the call (< 2^31) and of one image, depth pixels of one image
    int W, H, Wl, r;
    int filter_class, min_conf;
    float scale;
};

template <int CAP>
__global__ void __launch_bounds__(kThreads) k_posterior(const PosteriorArgs a)
{
    const uint32_t i = blockIdx.x * (uint32_t)kThreads + threadIdx.x;
    const bool inside = i < a.n_lpx;
    const uint32_t img = inside ? i / a.lpix : 0u, rem = inside ? i - img * a.lpix : 0u;
    const uint32_t yl = rem / (uint32_t)a.Wl, xl = rem - yl * (uint32_t)a.Wl;
    const int x = (int)(xl * (uint32_t)a.r), y = (int)(yl * (uint32_t)a.r);
    const uint16_t *__restrict__ frame = a.depth + (size_t)img * a.pix;
    // Q1: the filter first, then the pixel's own depth
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

    // Q2: rule R2's walk; a leaf slot's PDF is added class by class, trees in index order; a walk that falls off adds nothing
    for (int t = 0; t < a.T; ++t)
        walk_tree(a.forest + a.rec(t, 0), a.D, a.E(), p, live,
                  [&](int, uint32_t, uint32_t side, const float *__restrict__ rec) {
                      const float *__restrict__ pdf = rec + 7 + side * (uint32_t)C;
#pragma unroll
                      for (int c = 0; c < CAP; ++c)
                          if (c < C) acc[c] = acc[c] + pdf[c];
                  },
                  [] {});
    if (!live) return;

    // Q3: the inference argmax.  Q4: the winner's share of the vote
    float best = 0.f, S = 0.f;
    uint32_t label = 0u;
#pragma unroll
    for (int c = 0; c < CAP; ++c) {
        if (c < C) {
            if (acc[c] > best) {
                best = acc[c];
                label = (uint32_t)c;
            }
            S = S + acc[c];
        }
    }
    int conf = 0;
    if (S > 0.f) {
        const int v = floor_i32((best / S) * 65535.0f);
        conf = v < 0 ? 0 : v > 65535 ? 65535 : v;
    }
    // Q5
    if (a.conf) a.conf[i] = (uint16_t)conf;
    if (a.labels && conf >= a.min_conf) a.labels[i] = (uint16_t)label;
    if (a.sums) {
        float *__restrict__ plane = a.sums + (size_t)img * (size_t)C * a.lpix + rem;
#pragma unroll
        for (int c = 0; c < CAP; ++c)
            if (c < C) plane[(size_t)c * a.lpix] = acc[c];
    }
}

struct CountsArgs {
    const uint16_t *pred, *conf, *truth;
    u64 *counts;
    uint32_t n_lpx, lpix, pix_t;      // label pixels of the call and of one image, truth pixels of one image
    uint32_t Wl, W, r;
    uint32_t bins;
};

__global__ void __launch_bounds__(kThreads) k_confidence_counts(const CountsArgs a)
{
    __shared__ uint32_t hist[2 * kMaxBins];
    const int tid = threadIdx.x, lane = tid & 63;
    const uint32_t cells = 2u * a.bins;
    for (uint32_t i = tid; i < cells; i += kThreads) hist[i] = 0u;
    __syncthreads();

    uint32_t n_labelled = 0u, n_unclassified = 0u;
    // (no bound depends on the lane: every lane of a wave makes the same trips, as the ballot and the wave sums need)
    for (uint32_t i0 = (blockIdx.x * (uint32_t)kThreads + (uint32_t)tid) - (uint32_t)lane; i0 < a.n_lpx;
         i0 += gridDim.x * (uint32_t)kThreads) {
        const uint32_t i = i0 + (uint32_t)lane;
        uint32_t t = 0u;
        if (i < a.n_lpx) {
            const uint32_t img = i / a.lpix, rem = i - img * a.lpix;
            const uint32_t yl = rem / a.Wl, xl = rem - yl * a.Wl;
            t = a.truth[img * a.pix_t + yl * a.r * a.W + xl * a.r];     // < 2^31: the entry point checks
        }
        if (__ballot(t != 0u) == 0ull) continue;                    // (most of a frame carries no truth)
        if (t == 0u) continue;
        ++n_labelled;
        const uint32_t p = a.pred[i];
        if (p == kNoPixel) {
            ++n_unclassified;
        } else {
            const uint32_t b = ((uint32_t)a.conf[i] * a.bins) >> 16;    // < bins
            atomicAdd(&hist[2u * b + (p == t ? 1u : 0u)], 1u);
        }
    }
    const uint32_t l = wave_sum(n_labelled), u = wave_sum(n_unclassified);
    if (lane == 0) {
        if (u) atomicAdd(a.counts + cells, (u64)u);
        if (l) atomicAdd(a.counts + cells + 1, (u64)l);
    }
    __syncthreads();
    for (uint32_t i = tid; i < cells; i += kThreads) {
        const uint32_t v = hist[i];
        if (v) atomicAdd(a.counts + i, (u64)v);
    }
}

}  // namespace

extern "C" {

int rdf_labels_forest_posterior(const uint16_t *depth, int n_img, int dim_x, int dim_y, const float *forest, int n_trees,
                                int max_depth, int n_classes, const uint16_t *filter, int filter_class, int labels_reduce,
                                float scale_factor, int min_conf, uint16_t *labels_out, uint16_t *conf_out, float *sums_out,
                                void *stream)
{
    // (rule Q6, not bad_forest_shape: too many classes are RDF_ERR_TOO_LARGE here, after the alignment checks)
    if (n_trees < 1 || max_depth < 1 || max_depth > kMaxDepth || n_classes < 1 || labels_reduce < 1 || n_img < 0 || dim_x < 0 ||
        dim_y < 0 || filter_class < -1 || filter_class > 65535 || min_conf < 0 || min_conf > 65535)
        return RDF_ERR_BAD_ARG;
    if (misaligned(depth, 2) || misaligned(filter, 2) || misaligned(labels_out, 2) || misaligned(conf_out, 2) ||
        misaligned(forest, 4) || misaligned(sums_out, 4))
        return RDF_ERR_BAD_ARG;
    const long long pix = (long long)dim_x * dim_y;
    if (n_classes > RDF_POSTERIOR_MAX_CLASSES || (n_img > 0 && (pix >= (1ll << 31) || pix * n_img >= (1ll << 31))))
        return RDF_ERR_TOO_LARGE;
    const long long Wl = dim_x / labels_reduce, Hl = dim_y / labels_reduce;
    if (n_img == 0 || Wl == 0 || Hl == 0) return RDF_OK;
    if (!depth || !forest || (!labels_out && !conf_out && !sums_out) || (!filter && filter_class != -1)) return RDF_ERR_NULL_PTR;

    PosteriorArgs a = {{n_trees, max_depth, n_classes}};
    a.depth = depth;
    a.filter = filter;
    a.forest = forest;
    a.labels = labels_out;
    a.conf = conf_out;
    a.sums = sums_out;
    a.lpix = (uint32_t)(Wl * Hl);
    a.n_lpx = a.lpix * (uint32_t)n_img;
    a.pix = (uint32_t)pix;
    a.W = dim_x;
    a.H = dim_y;
    a.Wl = (int)Wl;
    a.r = labels_reduce;
    a.filter_class = filter_class;
    a.min_conf = min_conf;
    a.scale = scale_factor;
    const dim3 grid(blocks(a.n_lpx, kThreads)), block(kThreads);
    if (n_classes <= 4)
        hipLaunchKernelGGL(k_posterior<4>, grid, block, 0, S(stream), a);
    else if (n_classes <= 8)
        hipLaunchKernelGGL(k_posterior<8>, grid, block, 0, S(stream), a);
    else
        hipLaunchKernelGGL(k_posterior<16>, grid, block, 0, S(stream), a);
    return (int)hipGetLastError();
}

int rdf_labels_confidence_counts(int n_img, int dim_x, int dim_y, int labels_reduce, int bins, const uint16_t *pred,
                                 const uint16_t *conf, const uint16_t *truth, uint64_t *counts, void *stream)
{
    if (bins < 1 || bins > kMaxBins || labels_reduce < 1 || n_img < 0 || dim_x < 0 || dim_y < 0) return RDF_ERR_BAD_ARG;
    const long long Wl = dim_x / labels_reduce, Hl = dim_y / labels_reduce;
    if (n_img == 0 || Wl == 0 || Hl == 0) return RDF_OK;
    if (!pred || !conf || !truth || !counts) return RDF_ERR_NULL_PTR;
    const long long pix_t = (long long)dim_x * dim_y;
    if (pix_t >= (1ll << 31) || pix_t * n_img >= (1ll << 31)) return RDF_ERR_TOO_LARGE;
    if (misaligned(pred, 2) || misaligned(conf, 2) || misaligned(truth, 2) || misaligned(counts, 8)) return RDF_ERR_BAD_ARG;

    CountsArgs a;
    a.pred = pred;
    a.conf = conf;
    a.truth = truth;
    a.counts = reinterpret_cast<u64 *>(counts);
    a.lpix = (uint32_t)(Wl * Hl);
    a.n_lpx = a.lpix * (uint32_t)n_img;
    a.pix_t = (uint32_t)pix_t;
    a.Wl = (uint32_t)Wl;
    a.W = (uint32_t)dim_x;
    a.r = (uint32_t)labels_reduce;
    a.bins = (uint32_t)bins;
    unsigned grid = blocks(a.n_lpx, kThreads);
    grid = grid > (unsigned)kCountBlocks ? (unsigned)kCountBlocks : grid;
    hipLaunchKernelGGL(k_confidence_counts, dim3(grid), dim3(kThreads), 0, S(stream), a);
    return (int)hipGetLastError();
}

}  // extern "C"
