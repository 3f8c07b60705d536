// score_hip.hip -- predicted label maps against truth label maps on the device: one pass over the two maps gives the
// confusion matrix and the two sums of the reference's `pct. matching pixels` (src/train_model.py:104-107, 131-135,
// src/test_on_saved_model.py), where the host path copies both maps down and compares them in numpy.  Built into
// librdf_labels.so.  The contract is in include/rdf_labels.h; it is integer arithmetic, so no result depends on the order
// in which pixels are visited and two runs give the same bytes.
//
// k_score: the prediction map is one contiguous run of label pixels whatever labels_reduce is, so a lane takes eight of them
// with one 16-byte load; the up to seven pixels in front of the first 16-byte boundary and behind the last full group are
// taken one per lane by the first workgroup.  At labels_reduce 1 the truth is the same run (a second 16-byte load when it
// is aligned like the prediction, else the loads the compiler makes of a 2-byte aligned copy); above 1 a lane works out
// the (image, row, column) of its first pixel once and steps from there, gathering the truth at (x * r, y * r).
// Counts: the cell (truth 0, prediction none) -- most of a live frame --, `equal` and `labelled` stay in lane registers and
// are summed once per wave at the end; a wave whose 512 pixels are all of that cell does nothing else.  Every other pixel
// goes to a 32-bit histogram in LDS with one LDS add, one histogram per wave while four of them fit the 65 x 65 block (up
// to 31 classes), else one per workgroup.  A workgroup adds each non-zero cell to global memory once.
// per_image (a template argument: without it none of this is compiled in): a wave whose lanes all sit in one image keeps
// that image's two sums in registers and adds them when it moves on to another image; only a wave-iteration that has an
// image boundary inside adds per pixel.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/rdf_labels.h"
#include "rdf_kernel_util.hpp"

namespace {

// Two workgroups a compute unit: measured on 64 frames of 848x480, 512 workgroups take 34 us where 1024 take 37 and 2048
// take 45, and on 8 frames 12 us against 19 and 26 (every workgroup ends with one global atomic per non-zero cell, all
// onto the same few addresses).
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxBlocks = 512;       // larger calls stride over the grid
constexpr int kMaxChunk = 16;
constexpr int kMaxCells = (RDF_SCORE_MAX_CLASSES + 1) * (RDF_SCORE_MAX_CLASSES + 1);
constexpr uint32_t kNoImage = 0xffffffffu;

// label map [n][Hl][Wl] against truth [n][H][W] sampled at (x * r, y * r)
struct Geometry {
    uint32_t total;             // label pixels = head + 8 * n_groups + tail, head < 8 and tail < 8
    uint32_t head;              // pred + head is 16-byte aligned
    uint32_t n_groups;
    uint32_t chunk;             // >= 1: the sets of kThreads groups a workgroup takes in a row
    uint32_t Wl, Hl, pix_l;     // pix_l = Hl * Wl
    uint32_t row_step;          // r * W: truth elements from one label row to the next
    uint32_t pix_t;             // H * W
    uint32_t r;
};

struct LaneSums {
    uint32_t dominant, equal, labelled;
};

struct ImageSums {          // the image a wave is in (uniform) and, per lane, what it has seen of it
    uint32_t image, equal, labelled;
};

__device__ __forceinline__ void flush_image(ImageSums &w, uint32_t *__restrict__ per_image)
{
    if (w.image == kNoImage) return;                    // uniform
    const uint32_t e = wave_sum(w.equal), l = wave_sum(w.labelled);
    if ((threadIdx.x & 63) == 0) {
        if (e) atomicAdd(per_image + 2 * (size_t)w.image, e);
        if (l) atomicAdd(per_image + 2 * (size_t)w.image + 1, l);
    }
    w.equal = w.labelled = 0u;
}

// n (0..8) pixels of this lane, the first at label-map index idx0.  Called by every lane of a wave together.
template <bool PER_IMAGE>
__device__ __forceinline__ void consume(int n, uint32_t idx0, const uint32_t p[8], const uint32_t t[8], int C,
                                        uint32_t *__restrict__ hist, LaneSums &s, ImageSums &w, const Geometry &geo,
                                        uint32_t *__restrict__ per_image)
{
    const uint32_t stride = (uint32_t)C + 1u, dominant = (uint32_t)C;      // cell (0, C)
    // a wave that sees nothing but (truth 0, prediction none) -- most waves of a live frame -- is done here: such a pixel is
    // neither equal (the prediction is >= C >= 1) nor labelled
    const uint32_t any_t = ((t[0] | t[1]) | (t[2] | t[3])) | ((t[4] | t[5]) | (t[6] | t[7]));
    const uint32_t min_p = min(min(min(p[0], p[1]), min(p[2], p[3])), min(min(p[4], p[5]), min(p[6], p[7])));
    if (__ballot(n > 0 && (n < 8 || any_t != 0u || min_p < (uint32_t)C)) == 0ull) {
        s.dominant += (uint32_t)n;
        return;
    }
    uint32_t eq_mask = 0u, lab_mask = 0u;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const bool have = k < n;
        eq_mask |= (uint32_t)(have && p[k] == t[k]) << k;
        lab_mask |= (uint32_t)(have && t[k] > 0u) << k;
        const uint32_t cell = min(t[k], (uint32_t)C) * stride + min(p[k], (uint32_t)C);
        const bool other = have && cell != dominant;
        s.dominant += (uint32_t)(have && cell == dominant);
        if (other) atomicAdd(hist + cell, 1u);
    }
    s.equal += __popc(eq_mask);
    s.labelled += __popc(lab_mask);

    if (PER_IMAGE) {
        const u64 active = __ballot(n > 0);
        if (active == 0ull) return;
        const uint32_t img0 = idx0 / geo.pix_l, rem0 = idx0 - img0 * geo.pix_l;
        const uint32_t first = (uint32_t)__shfl((int)img0, __ffsll((long long)active) - 1, 64);
        const bool apart = n > 0 && (rem0 + (uint32_t)n > geo.pix_l || img0 != first);
        if (__ballot(apart) == 0ull) {
            if (first != w.image) {
                flush_image(w, per_image);
                w.image = first;
            }
            w.equal += __popc(eq_mask);
            w.labelled += __popc(lab_mask);
        } else {
            uint32_t img = img0, rem = rem0;
            for (int k = 0; k < n; ++k) {
                if ((eq_mask >> k) & 1u) atomicAdd(per_image + 2 * (size_t)img, 1u);
                if ((lab_mask >> k) & 1u) atomicAdd(per_image + 2 * (size_t)img + 1, 1u);
                if (++rem == geo.pix_l) {
                    rem = 0u;
                    ++img;
                }
            }
        }
    }
}

// the truth of n pixels from label-map index idx0 on, sampled at (x * r, y * r)
__device__ __forceinline__ void gather_truth(int n, uint32_t idx0, const uint16_t *__restrict__ truth, const Geometry &geo,
                                             uint32_t t[8])
{
    const uint32_t q = idx0 / geo.Wl;                   // label row over all images
    uint32_t x = idx0 - q * geo.Wl;
    uint32_t img = q / geo.Hl, y = q - img * geo.Hl;
    uint32_t row = img * geo.pix_t + y * geo.row_step;
    uint32_t at[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        at[k] = row + x * geo.r;
        if (++x == geo.Wl) {
            x = 0u;
            row += geo.row_step;
            if (++y == geo.Hl) {
                y = 0u;
                ++img;
                row = img * geo.pix_t;
            }
        }
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) t[k] = k < n ? (uint32_t)truth[at[k]] : 0u;
}

// R1: labels_reduce == 1 (the truth is indexed as the prediction).  TRUTH_VEC: truth + head is 16-byte aligned too.
template <bool R1, bool TRUTH_VEC, bool PER_IMAGE>
__global__ void __launch_bounds__(kThreads) k_score(Geometry geo, int C, const uint16_t *__restrict__ pred,
                                                    const uint16_t *__restrict__ truth,
                                                    u64 *__restrict__ counts, uint32_t *__restrict__ per_image)
{
    __shared__ uint32_t hist_all[kMaxCells];
    __shared__ uint32_t tail_sums[3];
    const int tid = threadIdx.x;
    const uint32_t total = geo.total, head = geo.head, n_groups = geo.n_groups, chunk = geo.chunk;
    const int cells = (C + 1) * (C + 1);
    const int copies = cells * kWaves <= kMaxCells ? kWaves : 1;
    for (int i = tid; i < cells * copies; i += kThreads) hist_all[i] = 0u;
    if (tid < 3) tail_sums[tid] = 0u;
    __syncthreads();
    uint32_t *hist = hist_all + (copies == 1 ? 0 : (tid >> 6) * cells);

    LaneSums s = {0u, 0u, 0u};
    ImageSums w = {kNoImage, 0u, 0u};
    uint32_t p[8], t[8];

    if (blockIdx.x == 0) {      // the pixels in front of and behind the full groups, one per lane (at most 14)
        const uint32_t tail = total - head - 8u * n_groups;
        const bool mine = (uint32_t)tid < head + tail;
        const uint32_t idx = (uint32_t)tid < head ? (uint32_t)tid : head + 8u * n_groups + ((uint32_t)tid - head);
        if (tid < 64) {
            const int n = mine ? 1 : 0;
#pragma unroll
            for (int k = 0; k < 8; ++k) p[k] = t[k] = 0u;
            if (mine) {
                p[0] = pred[idx];
                if (R1) t[0] = truth[idx];
            }
            if (!R1) gather_truth(n, mine ? idx : 0u, truth, geo, t);
            consume<PER_IMAGE>(n, idx, p, t, C, hist, s, w, geo, per_image);
        }
    }

    const uint4 *__restrict__ pred_v = reinterpret_cast<const uint4 *>(pred + head);
    const uint16_t *__restrict__ truth_b = truth + head;
    auto load = [&](uint32_t base, uint4 &pv, uint4 &tv) {
        const uint32_t g = base + (uint32_t)tid;
        pv = tv = make_uint4(0u, 0u, 0u, 0u);
        if (g >= n_groups) return;
        pv = pred_v[g];
        if (R1) {
            if (TRUTH_VEC)
                tv = reinterpret_cast<const uint4 *>(truth_b)[g];
            else
                __builtin_memcpy(&tv, truth_b + 8 * (size_t)g, 16);
        }
    };
    // A workgroup takes `chunk` consecutive sets of kThreads groups, then strides over the grid: chunk > 1 only when every
    // workgroup makes that many trips anyway, and then its waves stay inside one image for longer (PER_IMAGE).  The
    // groups of the trip after this one are loaded before this one is counted.
    // (no bound depends on the lane: every lane of a wave makes the same trips, as the wave sums need)
    const uint32_t tile = chunk * (uint32_t)kThreads;
    uint32_t k = 0u, tile_base = blockIdx.x * tile, base = tile_base;
    uint4 pv, tv, pv_next, tv_next;
    load(base, pv, tv);
    while (base < n_groups) {
        uint32_t k_next = k + 1u, tile_next = tile_base;
        if (k_next == chunk) {
            k_next = 0u;
            tile_next += gridDim.x * tile;
        }
        const uint32_t base_next = tile_next + k_next * (uint32_t)kThreads;     // rising, so the first one past the end ends it
        load(base_next, pv_next, tv_next);
        const uint32_t g = base + (uint32_t)tid;
        const bool mine = g < n_groups;
        const uint32_t idx0 = head + 8u * (mine ? g : 0u);
        const int n = mine ? 8 : 0;
        unpack8(pv, p);
        if (R1)
            unpack8(tv, t);
        else
            gather_truth(n, idx0, truth, geo, t);
        consume<PER_IMAGE>(n, idx0, p, t, C, hist, s, w, geo, per_image);
        pv = pv_next;
        tv = tv_next;
        base = base_next;
        k = k_next;
        tile_base = tile_next;
    }
    if (PER_IMAGE) flush_image(w, per_image);

    const uint32_t d = wave_sum(s.dominant), e = wave_sum(s.equal), l = wave_sum(s.labelled);
    if ((tid & 63) == 0) {
        if (d) atomicAdd(&tail_sums[0], d);
        if (e) atomicAdd(&tail_sums[1], e);
        if (l) atomicAdd(&tail_sums[2], l);
    }
    __syncthreads();
    for (int i = tid; i < cells; i += kThreads) {
        uint32_t v = i == C ? tail_sums[0] : 0u;
        for (int c = 0; c < copies; ++c) v += hist_all[c * cells + i];
        if (v) atomicAdd(counts + i, (u64)v);
    }
    if (tid < 2 && tail_sums[1 + tid]) atomicAdd(counts + cells + tid, (u64)tail_sums[1 + tid]);
}

template <bool R1, bool TRUTH_VEC>
void launch(unsigned grid, hipStream_t stream, const Geometry &geo, int C, const uint16_t *pred, const uint16_t *truth,
            u64 *counts, uint32_t *per_image)
{
    if (per_image)
        hipLaunchKernelGGL((k_score<R1, TRUTH_VEC, true>), dim3(grid), dim3(kThreads), 0, stream, geo, C, pred, truth, counts,
                           per_image);
    else
        hipLaunchKernelGGL((k_score<R1, TRUTH_VEC, false>), dim3(grid), dim3(kThreads), 0, stream, geo, C, pred, truth, counts,
                           per_image);
}

}  // namespace

extern "C" {

size_t rdf_score_counts_bytes(int num_classes)
{
    if (num_classes < 1 || num_classes > RDF_SCORE_MAX_CLASSES) return 0;
    return sizeof(uint64_t) * ((size_t)(num_classes + 1) * (num_classes + 1) + 2);
}

int rdf_score_labels(int n_img, int dim_x, int dim_y, int labels_reduce, int num_classes, const uint16_t *pred,
                     const uint16_t *truth, uint64_t *counts, uint32_t *per_image, void *stream)
{
    if (num_classes < 1 || num_classes > RDF_SCORE_MAX_CLASSES || labels_reduce < 1 || n_img < 0 || dim_x < 0 || dim_y < 0)
        return RDF_ERR_BAD_ARG;
    const long long Wl = dim_x / labels_reduce, Hl = dim_y / labels_reduce;
    if (n_img == 0 || Wl == 0 || Hl == 0) return RDF_OK;
    if (!pred || !truth || !counts) return RDF_ERR_NULL_PTR;
    const long long pix_t = (long long)dim_x * dim_y;
    if (pix_t >= (1ll << 31) || pix_t * n_img >= (1ll << 31)) return RDF_ERR_TOO_LARGE;
    if (misaligned(pred, 2) || misaligned(truth, 2) || misaligned(counts, 8) || misaligned(per_image, 4))
        return RDF_ERR_BAD_ARG;

    Geometry geo;
    geo.total = (uint32_t)(Wl * Hl * n_img);
    geo.head = (uint32_t)(((16u - (unsigned)(reinterpret_cast<uintptr_t>(pred) & 15u)) & 15u) / 2u);
    if (geo.head > geo.total) geo.head = geo.total;
    geo.n_groups = (geo.total - geo.head) / 8u;
    geo.Wl = (uint32_t)Wl;
    geo.Hl = (uint32_t)Hl;
    geo.pix_l = (uint32_t)(Wl * Hl);
    geo.row_step = (uint32_t)labels_reduce * (uint32_t)dim_x;
    geo.pix_t = (uint32_t)pix_t;
    geo.r = (uint32_t)labels_reduce;
    unsigned grid = (geo.n_groups + kThreads - 1) / kThreads;
    grid = grid < 1u ? 1u : grid > (unsigned)kMaxBlocks ? (unsigned)kMaxBlocks : grid;
    geo.chunk = geo.n_groups / ((uint32_t)kThreads * grid);         // the trips every workgroup makes
    geo.chunk = geo.chunk < 1u ? 1u : geo.chunk > (uint32_t)kMaxChunk ? (uint32_t)kMaxChunk : geo.chunk;
    hipStream_t s = S(stream);
    u64 *c = reinterpret_cast<u64 *>(counts);
    if (labels_reduce != 1)
        launch<false, false>(grid, s, geo, num_classes, pred, truth, c, per_image);
    else if (!misaligned(truth + geo.head, 16))
        launch<true, true>(grid, s, geo, num_classes, pred, truth, c, per_image);
    else
        launch<true, false>(grid, s, geo, num_classes, pred, truth, c, per_image);
    return (int)hipGetLastError();
}

}  // extern "C"
