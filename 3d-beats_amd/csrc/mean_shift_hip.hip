// mean_shift_hip.hip -- gfx950 kernels for the consumer of the composite label map:
// per-class 2-D mean-shift mode finding and fingertip heights.
//
// Reference: src/cuda/mean_shift.cu:3-48 driven by the host loop of src/cuda/mean_shift.py:35-59; heights:
// src/3d_bz.py:503-522 on the host.  Here everything stays on the device, in ONE launch, and is bitwise reproducible:
// k_mean_shift_fused is the unweighted policy of modes_body (rdf_modes.hpp), where the how and the why are written down.

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/rdf_hip.h"
#include "rdf_modes.hpp"

namespace {

template <bool HEIGHTS>
__global__ __launch_bounds__(kModesThreads) void k_mean_shift_fused(const uint16_t *labels, int dim_x, int dim_y, int L,
                                                                    const float *variances, int num_rounds, double *means_out,
                                                                    const HeightArgs hp)
{
    modes_body<Unweighted, HEIGHTS>(labels, nullptr, dim_x, dim_y, L, variances, num_rounds, means_out, hp);
}

// Heights of the requested classes' modes above the calibrated plane (height_of_mode, rdf_modes.hpp) where the means are
// already there; rdf_mean_shift_heights has them ride on the mean shift's launch.
__global__ void k_fingertip_heights(const double *means, int L, const HeightArgs h)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= h.n_ids) return;
    const int c = h.class_ids[i];
    h.heights[i] = (c >= 1 && c <= L) ? height_of_mode(means[(c - 1) * 2], means[(c - 1) * 2 + 1], h) : nan("");
}

} // namespace

extern "C" {

size_t rdf_mean_shift_workspace_bytes(int num_classes, int num_rounds)
{
    (void)num_classes; (void)num_rounds;
    return 0;      // every class iterates inside one workgroup: nothing is handed between workgroups any more
}

static int mean_shift_launch(const uint16_t *labels, int dim_x, int dim_y, int num_classes, const float *variances,
                             int num_rounds, double *means_out, const HeightArgs *heights, void *stream, int n_frames = 1)
{
    if (dim_x < 0 || dim_y < 0 || dim_x > 65535 || dim_y > 65535 || num_classes < 0 || num_classes > kModesMaxClasses ||
        num_rounds < 0)
        return RDF_ERR_BAD_ARG;
    if (num_classes == 0) return RDF_OK;
    if ((long long)dim_x * dim_y >= (1ll << 31)) return RDF_ERR_TOO_LARGE;
    // the kernel lists every class's pixels and reads variances[0 .. num_classes) whatever the number of rounds
    if (!means_out || (((long long)dim_x * dim_y > 0) && !labels) || !variances) return RDF_ERR_NULL_PTR;
    const int lds_bytes = modes_lds_bytes<Unweighted>();
    static LdsAllowance allowed[2];
    const int rc = allowed[heights ? 1 : 0].allow(heights ? reinterpret_cast<const void *>(k_mean_shift_fused<true>)
                                                          : reinterpret_cast<const void *>(k_mean_shift_fused<false>),
                                                  lds_bytes, RDF_ERR_NO_DEVICE);
    if (rc != RDF_OK) return rc;
    if (heights)
        hipLaunchKernelGGL(k_mean_shift_fused<true>, dim3((unsigned)num_classes, (unsigned)n_frames), dim3(kModesThreads),
                           lds_bytes, reinterpret_cast<hipStream_t>(stream), labels, dim_x, dim_y, num_classes, variances,
                           num_rounds, means_out, *heights);
    else
        hipLaunchKernelGGL(k_mean_shift_fused<false>, dim3((unsigned)num_classes, (unsigned)n_frames), dim3(kModesThreads),
                           lds_bytes, reinterpret_cast<hipStream_t>(stream), labels, dim_x, dim_y, num_classes, variances,
                           num_rounds, means_out, HeightArgs{});
    return (int)hipGetLastError();
}

int rdf_mean_shift(const uint16_t *labels, int dim_x, int dim_y, int num_classes, const float *variances,
                   int num_rounds, double *means_out, void *workspace, void *stream)
{
    (void)workspace;
    return mean_shift_launch(labels, dim_x, dim_y, num_classes, variances, num_rounds, means_out, nullptr, stream);
}

int rdf_fingertip_heights(const double *means, int num_classes, const int *class_ids, int n_ids,
                          const uint16_t *depth, int dim_x, int dim_y, int labels_reduce, float fx, float fy,
                          float ppx, float ppy, const float *plane, double *heights_out, void *stream)
{
    if (num_classes < 0 || n_ids < 0 || dim_x < 0 || dim_y < 0 || labels_reduce < 1) return RDF_ERR_BAD_ARG;
    if (n_ids == 0) return RDF_OK;
    if (!means || !class_ids || !depth || !plane || !heights_out) return RDF_ERR_NULL_PTR;
    const HeightArgs h = {class_ids, n_ids, depth, dim_x, dim_y, labels_reduce, fx, fy, ppx, ppy, plane, heights_out, 0};
    hipLaunchKernelGGL(k_fingertip_heights, dim3((n_ids + 63) / 64), dim3(64), 0, reinterpret_cast<hipStream_t>(stream),
                       means, num_classes, h);
    return (int)hipGetLastError();
}

int rdf_mean_shift_heights(const uint16_t *labels, int dim_x, int dim_y, int num_classes, const float *variances,
                           int num_rounds, double *means_out, const int *class_ids, int n_ids, const uint16_t *depth,
                           int depth_dim_x, int depth_dim_y, int labels_reduce, float fx, float fy, float ppx, float ppy,
                           const float *plane, double *heights_out, void *stream)
{
    if (n_ids < 0 || n_ids > kModesThreads || depth_dim_x < 0 || depth_dim_y < 0 || labels_reduce < 1) return RDF_ERR_BAD_ARG;
    if (n_ids == 0 || num_classes == 0) {
        // nothing to fuse: the two calls, one of which does nothing (no class at all: every id is "reset")
        int rc = mean_shift_launch(labels, dim_x, dim_y, num_classes, variances, num_rounds, means_out, nullptr, stream);
        if (rc != RDF_OK || n_ids == 0) return rc;
        return rdf_fingertip_heights(means_out, num_classes, class_ids, n_ids, depth, depth_dim_x, depth_dim_y,
                                     labels_reduce, fx, fy, ppx, ppy, plane, heights_out, stream);
    }
    if (!class_ids || !depth || !plane || !heights_out) return RDF_ERR_NULL_PTR;
    const HeightArgs h = {class_ids, n_ids, depth, depth_dim_x, depth_dim_y, labels_reduce, fx, fy, ppx, ppy, plane,
                          heights_out, 0};
    return mean_shift_launch(labels, dim_x, dim_y, num_classes, variances, num_rounds, means_out, &h, stream);
}

int rdf_mean_shift_heights_batch(const uint16_t *labels, int n, int dim_x, int dim_y, int num_classes, const float *variances,
                                 int num_rounds, double *means_out, const int *class_ids, int n_ids, const uint16_t *depth,
                                 int depth_dim_x, int depth_dim_y, int labels_reduce, float fx, float fy, float ppx, float ppy,
                                 const float *plane, double *heights_out, int heights_stride, void *stream)
{
    // (no two-call fallback here: a batch without ids or classes is refused)
    if (n < 0 || n_ids <= 0 || n_ids > kModesThreads || num_classes <= 0 || depth_dim_x < 0 || depth_dim_y < 0 ||
        labels_reduce < 1 || heights_stride < n_ids)
        return RDF_ERR_BAD_ARG;
    if (dim_x < 0 || dim_y < 0 || dim_x > 65535 || dim_y > 65535 || num_classes > kModesMaxClasses || num_rounds < 0)
        return RDF_ERR_BAD_ARG;
    if (n > 65535) return RDF_ERR_TOO_LARGE;      // (the frame is the grid's y)
    if (n == 0) return RDF_OK;
    // the depth lookup indexes one frame with a long long; a frame of 2^31 pixels or more is refused like the labels'
    if ((long long)depth_dim_x * depth_dim_y >= (1ll << 31)) return RDF_ERR_TOO_LARGE;
    if (!class_ids || !depth || !plane || !heights_out) return RDF_ERR_NULL_PTR;
    const HeightArgs h = {class_ids, n_ids, depth, depth_dim_x, depth_dim_y, labels_reduce, fx, fy, ppx, ppy, plane,
                          heights_out, heights_stride};
    return mean_shift_launch(labels, dim_x, dim_y, num_classes, variances, num_rounds, means_out, &h, stream, n);
}

} // extern "C"
