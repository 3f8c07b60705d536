// soft_modes_hip.hip -- soft modes: the fingertip mean shift weighted by the forest's confidence.  Where rdf_mean_shift lets
// every pixel of a class pull equally, rdf_labels_weighted_modes gives each pixel an integer weight, and
// rdf_labels_composite_weights makes that weight for a layered stack: the product of the confidences of the layers that
// rdf_composite's walk visits.  Built into librdf_labels.so.  The contract (rules S) is in include/rdf_labels.h and
// tests/soft_modes_numpy.py restates it.
//
// k_composite_weights: one lane per pixel, a wave leaves at once when none of its 64 pixels starts a path (layer 0 says 0 or
// 65535: most of a frame).  Integer arithmetic, no LDS, no atomics: the bytes do not depend on anything but the inputs.
//
// k_weighted_modes: the weighted policy of modes_body (rdf_modes.hpp), the body that k_mean_shift_fused (mean_shift_hip.hip)
// runs unweighted: one workgroup of 1024 threads per (class, frame), the class's counted pixels listed once in LDS with a
// 16-bit weight each, every round on that list with fixed-order sums.  A pixel of weight 0 takes no slot; a class with more
// than Weighted::kListCap counted pixels is not listed, its rounds rescan the label and weight maps.

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/rdf_labels.h"
#include "rdf_modes.hpp"

namespace {

constexpr uint32_t kNoLabel = 65535u;
constexpr int kFlatThreads = 256;

// ---- composite weights (rules S1-S3) ----
__global__ void __launch_bounds__(kFlatThreads) k_composite_weights(const uint16_t *const *__restrict__ labels,
                                                                    const uint16_t *const *__restrict__ conf, int n_layers,
                                                                    uint32_t n_px, uint32_t dim_x, uint32_t lpix,
                                                                    const int2 *__restrict__ cond, int n_cond, int flip_x,
                                                                    uint16_t *__restrict__ out)
{
    const uint32_t p = blockIdx.x * (uint32_t)kFlatThreads + threadIdx.x;
    const bool inside = p < n_px;
    uint32_t l = inside ? (uint32_t)labels[0][p] : 0u;
    if (__ballot(l != 0u && l != kNoLabel) == 0ull) return;          // (most of a frame starts no path)
    if (!inside) return;
    long long off = 0;
    uint32_t w = 65535u;
    for (int j = 0; j < n_layers; ++j) {
        if (j > 0) l = labels[j][p];
        if (l == 0u || l == kNoLabel) return;                        // S1: nothing is written
        const long long e = off + (long long)l - 1;
        if (e < 0 || e >= n_cond) return;
        w = (w * (uint32_t)conf[j][p] + 32767u) / 65535u;            // S2: 65535^2 + 32767 < 2^32
        const int2 tv = cond[e];
        if (tv.x == 0) {
            uint32_t q = p;
            if (flip_x) {                                            // S3: the mirror of rdf_layered_run_hand's composite
                const uint32_t img = p / lpix, rem = p - img * lpix;
                const uint32_t y = rem / dim_x, x = rem - y * dim_x;
                q = img * lpix + y * dim_x + (dim_x - 1u - x);
            }
            out[q] = (uint16_t)w;
            return;
        }
        off = tv.y;
    }
}

// ---- weighted modes (rules S4-S7) ----
template <bool HEIGHTS>
__global__ __launch_bounds__(kModesThreads) void k_weighted_modes(const uint16_t *labels, const uint16_t *weights, int dim_x,
                                                                  int dim_y, int L, const float *variances, int num_rounds,
                                                                  double *means_out, const HeightArgs hp)
{
    modes_body<Weighted, HEIGHTS>(labels, weights, dim_x, dim_y, L, variances, num_rounds, means_out, hp);
}

constexpr long long kMaxElems = 1ll << 31;

}  // namespace

extern "C" {

int rdf_labels_composite_weights(const uint16_t *const *layer_labels, const uint16_t *const *layer_conf, int n_layers, int n_img,
                                 int dim_x, int dim_y, const int32_t *cond, int n_cond, int flip_x, uint16_t *weights_out,
                                 void *stream)
{
    if (n_layers < 1 || n_img < 0 || dim_x < 0 || dim_y < 0 || n_cond < 0 || dim_x > 65535 || dim_y > 65535) return RDF_ERR_BAD_ARG;
    if (misaligned(layer_labels, 8) || misaligned(layer_conf, 8) || misaligned(cond, 4) || misaligned(weights_out, 2))
        return RDF_ERR_BAD_ARG;
    const long long n_px = (long long)n_img * dim_x * dim_y;
    if (n_px >= kMaxElems) return RDF_ERR_TOO_LARGE;
    if (n_px == 0) return RDF_OK;
    if (!layer_labels || !layer_conf || !weights_out || (n_cond > 0 && !cond)) return RDF_ERR_NULL_PTR;
    hipLaunchKernelGGL(k_composite_weights, dim3(blocks(n_px, kFlatThreads)), dim3(kFlatThreads), 0, S(stream), layer_labels,
                       layer_conf, n_layers, (uint32_t)n_px, (uint32_t)dim_x, (uint32_t)dim_x * (uint32_t)dim_y,
                       reinterpret_cast<const int2 *>(cond), n_cond, flip_x ? 1 : 0, weights_out);
    return (int)hipGetLastError();
}

uint32_t rdf_labels_weighted_modes_list_cap(void) { return Weighted::kListCap; }

int rdf_labels_weighted_modes(const uint16_t *labels, const uint16_t *weights, int n_img, int dim_x, int dim_y, int num_classes,
                              const float *variances, int num_rounds, double *means_out, const int *class_ids, int n_ids,
                              const uint16_t *depth, int depth_dim_x, int depth_dim_y, int labels_reduce, float fx, float fy,
                              float ppx, float ppy, const float *plane, double *heights_out, int heights_stride, void *stream)
{
    if (n_img < 0 || dim_x < 0 || dim_y < 0 || dim_x > 65535 || dim_y > 65535 || num_classes < 1 || num_classes > kModesMaxClasses ||
        num_rounds < 0 || n_ids < 0 || n_ids > kModesThreads)
        return RDF_ERR_BAD_ARG;
    if (n_ids > 0 && (depth_dim_x < 0 || depth_dim_y < 0 || labels_reduce < 1 || heights_stride < n_ids)) return RDF_ERR_BAD_ARG;
    if (misaligned(labels, 2) || misaligned(weights, 2) || misaligned(variances, 4) || misaligned(means_out, 8))
        return RDF_ERR_BAD_ARG;
    if (n_ids > 0 && (misaligned(class_ids, 4) || misaligned(depth, 2) || misaligned(plane, 4) || misaligned(heights_out, 8)))
        return RDF_ERR_BAD_ARG;
    const long long n_px = (long long)n_img * dim_x * dim_y;
    if (n_px >= kMaxElems || n_img > 65535) return RDF_ERR_TOO_LARGE;          // (the frame is the grid's y)
    if (n_ids > 0 && (long long)n_img * depth_dim_x * depth_dim_y >= kMaxElems) return RDF_ERR_TOO_LARGE;
    if (n_px == 0) return RDF_OK;
    if (!labels || !variances || !means_out) return RDF_ERR_NULL_PTR;
    if (n_ids > 0 && (!class_ids || !depth || !plane || !heights_out)) return RDF_ERR_NULL_PTR;

    const bool heights = n_ids > 0;
    const int lds_bytes = modes_lds_bytes<Weighted>();
    static LdsAllowance allowed[2];
    const int rc = allowed[heights ? 1 : 0].allow(heights ? reinterpret_cast<const void *>(k_weighted_modes<true>)
                                                          : reinterpret_cast<const void *>(k_weighted_modes<false>),
                                                  lds_bytes, (int)hipErrorNoDevice);
    if (rc != RDF_OK) return rc;
    // (a null `weights` stays on this policy: every weight 1, the same cap)
    const dim3 grid((unsigned)num_classes, (unsigned)n_img), block(kModesThreads);
    if (heights) {
        const HeightArgs h = {class_ids, n_ids, depth, depth_dim_x, depth_dim_y, labels_reduce, fx, fy, ppx, ppy, plane,
                              heights_out, heights_stride};
        hipLaunchKernelGGL(k_weighted_modes<true>, grid, block, lds_bytes, S(stream), labels, weights, dim_x, dim_y, num_classes,
                           variances, num_rounds, means_out, h);
    } else {
        hipLaunchKernelGGL(k_weighted_modes<false>, grid, block, lds_bytes, S(stream), labels, weights, dim_x, dim_y, num_classes,
                           variances, num_rounds, means_out, HeightArgs{});
    }
    return (int)hipGetLastError();
}

}  // extern "C"
