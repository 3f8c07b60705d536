// labels_hip.hip -- colour-glove recordings to training labels on the device: the reference's split_pixels_by_nearest_color,
// apply_point_mapping and depths_from_points (src/cuda/points_ops.cu:207-255, 167-205, 39-63), its make_color_mapping loop
// (src/live_data_convert.py:156-204) and the per-frame labelling of its tick() (:413-458).  Built into its own
// librdf_labels.so.  The contract is in include/rdf_labels.h; all of it is integer arithmetic, so no result depends on the
// order in which pixels are visited.
//
// k_accum is the hot path.  The reference issues five 64-bit global atomics per pixel onto at most 5 K addresses and runs
// tries x iterations passes with a host round trip between them.  Here one pass serves every try: a lane loads 4 pixels as
// three dwords, finds each pixel's nearest colour per try, and per (try, colour) the wave sums its lanes with three packed
// 32-bit butterflies (r | g << 16, b | count << 16, cost: 256 pixels per wave keep every field in range).  Five lanes add
// the five sums to the workgroup's LDS block in one ds_add_u64, and the workgroup adds each non-zero entry of that block to
// global memory once.  k_update (one small workgroup) turns the sums into the next colours; the launches of one call are
// ordered by the stream, so no workgroup ever waits for another.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/rdf_labels.h"
#include "rdf_kernel_util.hpp"

namespace {

constexpr int kMaxK = RDF_LABELS_MAX_COLORS;
constexpr int kMaxTries = RDF_LABELS_MAX_TRIES;
constexpr int kAccThreads = 512;
constexpr int kAccMaxBlocks = 512;
constexpr int kUpdThreads = kMaxK * kMaxTries;      // one lane per (try, colour)
constexpr int kFlatThreads = 256;

// 4 pixels of group g as r | g << 8 | b << 16 each; pixels past the end read as black (skipped everywhere).
// A full group is three aligned dwords; only the image's last, partial group is read by bytes.
__device__ __forceinline__ void load_group(const uint8_t *__restrict__ image, long long g, int n_px, uint32_t px[4])
{
    const long long p0 = g * 4;
    px[0] = px[1] = px[2] = px[3] = 0u;
    if (p0 + 4 <= n_px) {
        const uint32_t *w = reinterpret_cast<const uint32_t *>(image) + g * 3;
        const uint32_t a = w[0], b = w[1], c = w[2];
        px[0] = a & 0xffffffu;
        px[1] = (a >> 24) | ((b & 0xffffu) << 8);
        px[2] = (b >> 16) | ((c & 0xffu) << 16);
        px[3] = c >> 8;
        return;
    }
    for (int p = 0; p < 4 && p0 + p < n_px; ++p) {
        const uint8_t *q = image + (p0 + p) * 3;
        px[p] = (uint32_t)q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16);
    }
}

__device__ __forceinline__ void store_group(uint8_t *__restrict__ image, long long g, int n_px, const uint32_t px[4])
{
    const long long p0 = g * 4;
    if (p0 + 4 <= n_px) {
        uint32_t *w = reinterpret_cast<uint32_t *>(image) + g * 3;
        w[0] = px[0] | (px[1] << 24);
        w[1] = (px[1] >> 8) | (px[2] << 16);
        w[2] = (px[2] >> 16) | (px[3] << 8);
        return;
    }
    for (int p = 0; p < 4 && p0 + p < n_px; ++p) {
        uint8_t *q = image + (p0 + p) * 3;
        q[0] = (uint8_t)px[p];
        q[1] = (uint8_t)(px[p] >> 8);
        q[2] = (uint8_t)(px[p] >> 16);
    }
}

// nearest of K colours (col: r, g, b as int, K rows): colour 0 first, then strictly smaller wins.  *cost = its distance.
__device__ __forceinline__ int nearest(const int *col, int K, uint32_t px, uint32_t *cost)
{
    const int r = (int)(px & 0xffu), g = (int)((px >> 8) & 0xffu), b = (int)(px >> 16);
    int best = 0;
    uint32_t bd = 0u;
    for (int i = 0; i < K; ++i) {
        const int dr = r - col[i * 3], dg = g - col[i * 3 + 1], db = b - col[i * 3 + 2];
        const uint32_t d = (uint32_t)(dr * dr + dg * dg + db * db);
        if (i == 0 || d < bd) {
            bd = d;
            best = i;
        }
    }
    *cost = bd;
    return best;
}

// sums[t][k][5] += {pixels, sum r, sum g, sum b, sum cost} of the pixels nearest to colour k of try t.  DOUBLE_COST: word 4
// of the destination holds a double (the reference's counts), else an integer (the mapping's workspace).
template <bool DOUBLE_COST>
__global__ void __launch_bounds__(kAccThreads) k_accum(int n_px, const uint8_t *__restrict__ image, int tries, int K,
                                                       const uint8_t *__restrict__ colors, u64 *__restrict__ sums)
{
    __shared__ int col[kMaxTries * kMaxK * 3];
    __shared__ u64 acc[kMaxTries * kMaxK * 5];
    const int tid = threadIdx.x, lane = tid & 63;
    for (int i = tid; i < tries * K * 3; i += kAccThreads) col[i] = colors[i];
    for (int i = tid; i < tries * K * 5; i += kAccThreads) acc[i] = 0;
    __syncthreads();

    const long long n_groups = ((long long)n_px + 3) / 4;
    // (the bound does not depend on the lane: every lane of a wave makes the same trips, as the butterflies need)
    for (long long base = (long long)blockIdx.x * kAccThreads; base < n_groups; base += (long long)gridDim.x * kAccThreads) {
        uint32_t px[4];
        load_group(image, base + tid, n_px, px);        // groups past the end read as black
        if (__ballot((px[0] | px[1] | px[2] | px[3]) != 0u) == 0ull) continue;
        for (int t = 0; t < tries; ++t) {
            const int *c = col + t * K * 3;
            int best[4];
            uint32_t cost[4];
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                best[p] = nearest(c, K, px[p], &cost[p]);
                if (px[p] == 0u) best[p] = -1;
            }
            for (int k = 0; k < K; ++k) {
                uint32_t rg = 0u, bn = 0u, cs = 0u;
#pragma unroll
                for (int p = 0; p < 4; ++p) {
                    if (best[p] != k) continue;
                    rg += (px[p] & 0xffu) | ((px[p] & 0xff00u) << 8);
                    bn += (px[p] >> 16) | 0x10000u;
                    cs += cost[p];
                }
                if (__ballot(bn != 0u) == 0ull) continue;
                rg = wave_sum(rg);
                bn = wave_sum(bn);
                cs = wave_sum(cs);
                if (lane < 5) {
                    const uint32_t v = lane == 0 ? bn >> 16 : lane == 1 ? rg & 0xffffu : lane == 2 ? rg >> 16
                                     : lane == 3 ? bn & 0xffffu : cs;
                    atomicAdd(&acc[(t * K + k) * 5 + lane], (u64)v);
                }
            }
        }
    }
    __syncthreads();
    for (int i = tid; i < tries * K * 5; i += kAccThreads) {
        const u64 v = acc[i];
        if (v == 0) continue;
        if (DOUBLE_COST && i % 5 == 4)
            atomicAdd(reinterpret_cast<double *>(sums + i), (double)v);     // an integer below 2^53: exact in any order
        else
            atomicAdd(sums + i, v);
    }
}

__global__ void __launch_bounds__(kFlatThreads) k_mapping_init(int tries, int K, const uint8_t *__restrict__ init,
                                                               uint8_t *__restrict__ colors, u64 *__restrict__ sums)
{
    for (int i = threadIdx.x; i < tries * K * 3; i += kFlatThreads) colors[i] = init[i];
    for (int i = threadIdx.x; i < tries * K * 5; i += kFlatThreads) sums[i] = 0;
}

// the sums of one pass -> the next colours (sum / pixels truncated, an empty group -> 0, 0, 0), sums zeroed for the next
// pass; after the last pass, the cost of every try and the first cheapest try.
__global__ void __launch_bounds__(kUpdThreads) k_mapping_update(int tries, int K, uint8_t *__restrict__ colors,
                                                                u64 *__restrict__ sums, int last, uint8_t *__restrict__ best,
                                                                RdfColorMappingResult *__restrict__ result)
{
    __shared__ u64 cost[kUpdThreads];
    __shared__ uint8_t next[kUpdThreads * 3];
    const int i = threadIdx.x;
    if (i < tries * K) {
        u64 *s = sums + i * 5;
        const u64 n = s[0];
        for (int j = 0; j < 3; ++j) {
            const uint8_t c = n ? (uint8_t)(s[1 + j] / n) : (uint8_t)0;
            next[i * 3 + j] = c;
            colors[i * 3 + j] = c;
        }
        cost[i] = s[4];
        for (int j = 0; j < 5; ++j) s[j] = 0;
    }
    __syncthreads();
    if (!last) return;
    __shared__ int win;
    if (i == 0) {
        int bt = 0;
        double bc = 0.;
        for (int t = 0; t < tries; ++t) {
            u64 c = 0;
            for (int k = 0; k < K; ++k) c += cost[t * K + k];
            const double d = (double)c;
            if (t == 0 || d < bc) {
                bc = d;
                bt = t;
            }
            if (result) result->cost[t] = d;
        }
        if (result) {
            for (int t = tries; t < kMaxTries; ++t) result->cost[t] = 0.;
            result->best_try = bt;
            result->tries = tries;
            result->best_cost = bc;
        }
        win = bt;
    }
    __syncthreads();
    if (i < K * 3) best[i] = next[win * K * 3 + i];
}

// mask, snap, label, RGBA, depth: 4 pixels per lane.  Every pointer but image may be NULL; K == 0 (no mapping) only masks.
__global__ void __launch_bounds__(kFlatThreads) k_label(int n_px, int K, const uint8_t *__restrict__ mapping,
                                                        uint8_t *__restrict__ image, const uint16_t *__restrict__ mask,
                                                        int mask_label, uint16_t *__restrict__ depth,
                                                        uint16_t *__restrict__ labels, uint32_t *__restrict__ rgba)
{
    __shared__ int col[kMaxK * 3];
    if ((int)threadIdx.x < K * 3) col[threadIdx.x] = mapping[threadIdx.x];
    __syncthreads();
    const long long g = (long long)blockIdx.x * kFlatThreads + threadIdx.x;
    const long long p0 = g * 4;
    if (p0 >= n_px) return;
    const int n = (int)(n_px - p0 < 4 ? n_px - p0 : 4);
    uint32_t px[4];
    load_group(image, g, n_px, px);
    for (int p = 0; p < n; ++p) {
        const long long at = p0 + p;
        uint32_t v = px[p];
        if (mask && (int)mask[at] != mask_label) v = 0u;
        if (v != 0u && K > 0) {
            uint32_t cost;
            const int b = nearest(col, K, v, &cost);
            v = (uint32_t)col[b * 3] | ((uint32_t)col[b * 3 + 1] << 8) | ((uint32_t)col[b * 3 + 2] << 16);
        }
        px[p] = v;
        if (labels) {
            int lab = 0;
            for (int i = 0; i < K; ++i)
                if (((uint32_t)col[i * 3] | ((uint32_t)col[i * 3 + 1] << 8) | ((uint32_t)col[i * 3 + 2] << 16)) == v) lab = i + 1;
            labels[at] = (uint16_t)lab;
        }
        if (rgba) rgba[at] = v ? v | 0xff000000u : 0u;
        if (depth && depth[at] == 0) depth[at] = 65535;
    }
    store_group(image, g, n_px, px);
}

__global__ void __launch_bounds__(kFlatThreads) k_depths_from_points(long long n, uint16_t *__restrict__ depth,
                                                                     const float4 *__restrict__ pts)
{
    const long long i = (long long)blockIdx.x * kFlatThreads + threadIdx.x;
    if (i >= n) return;
    const float4 p = pts[i];
    if (!(p.w > 0.f)) return;
    const float z = truncf(p.z);
    depth[i] = !(z > 0.f) ? (uint16_t)0 : z >= 65535.f ? (uint16_t)65535 : (uint16_t)(uint32_t)z;
}

constexpr long long kMaxElems = 1ll << 31;

inline unsigned accum_blocks(long long n_px)
{
    const unsigned b = blocks((n_px + 3) / 4, kAccThreads);
    return b < (unsigned)kAccMaxBlocks ? b : (unsigned)kAccMaxBlocks;
}

inline size_t colors_bytes(int tries, int K) { return ((size_t)tries * K * 3 + 7) & ~(size_t)7; }

int label_launch(int dim_x, int dim_y, int K, const uint8_t *mapping, uint8_t *image, const uint16_t *mask, int mask_label,
                 uint16_t *depth, uint16_t *labels, uint8_t *rgba, void *stream)
{
    if (dim_x < 0 || dim_y < 0 || K < 0 || K > kMaxK) return RDF_ERR_BAD_ARG;
    const long long n_px = (long long)dim_x * dim_y;
    if (n_px == 0) return RDF_OK;
    if ((K > 0 && !mapping) || !image) return RDF_ERR_NULL_PTR;
    if (n_px >= kMaxElems) return RDF_ERR_TOO_LARGE;
    if (misaligned(image, 4) || misaligned(rgba, 4) || misaligned(depth, 2) || misaligned(labels, 2) || misaligned(mask, 2))
        return RDF_ERR_BAD_ARG;
    hipLaunchKernelGGL(k_label, dim3(blocks((n_px + 3) / 4, kFlatThreads)), dim3(kFlatThreads), 0, S(stream), (int)n_px, K,
                       mapping, image, mask, mask_label, depth, labels, reinterpret_cast<uint32_t *>(rgba));
    return (int)hipGetLastError();
}

}  // namespace

extern "C" {

int rdf_split_pixels_by_nearest_color(int dim_x, int dim_y, int num_colors, const uint8_t *colors, const uint8_t *image,
                                      uint64_t *counts, void *stream)
{
    if (dim_x < 0 || dim_y < 0 || num_colors < 1 || num_colors > kMaxK) return RDF_ERR_BAD_ARG;
    const long long n_px = (long long)dim_x * dim_y;
    if (n_px == 0) return RDF_OK;
    if (!colors || !image || !counts) return RDF_ERR_NULL_PTR;
    if (n_px >= kMaxElems) return RDF_ERR_TOO_LARGE;
    if (misaligned(image, 4) || misaligned(counts, 8)) return RDF_ERR_BAD_ARG;
    hipLaunchKernelGGL((k_accum<true>), dim3(accum_blocks(n_px)), dim3(kAccThreads), 0, S(stream), (int)n_px, image, 1,
                       num_colors, colors, reinterpret_cast<u64 *>(counts));
    return (int)hipGetLastError();
}

int rdf_apply_point_mapping(int dim_x, int dim_y, int num_colors, const uint8_t *colors, uint8_t *image, void *stream)
{
    if (num_colors < 1) return RDF_ERR_BAD_ARG;
    return label_launch(dim_x, dim_y, num_colors, colors, image, nullptr, 0, nullptr, nullptr, nullptr, stream);
}

int rdf_depths_from_points(int n_img, int dim_x, int dim_y, uint16_t *depth, const float *pts, void *stream)
{
    if (n_img < 0 || dim_x < 0 || dim_y < 0) return RDF_ERR_BAD_ARG;
    const long long n = (long long)n_img * dim_x * dim_y;
    if (n == 0) return RDF_OK;
    if (!depth || !pts) return RDF_ERR_NULL_PTR;
    if (n >= kMaxElems) return RDF_ERR_TOO_LARGE;
    hipLaunchKernelGGL(k_depths_from_points, dim3(blocks(n, kFlatThreads)), dim3(kFlatThreads), 0, S(stream), n, depth,
                       reinterpret_cast<const float4 *>(pts));
    return (int)hipGetLastError();
}

size_t rdf_color_mapping_workspace_bytes(int tries, int num_colors)
{
    if (tries < 1 || tries > kMaxTries || num_colors < 1 || num_colors > kMaxK) return 0;
    return colors_bytes(tries, num_colors) + (size_t)tries * num_colors * 5 * sizeof(u64);
}

int rdf_make_color_mapping(int n_px, const uint8_t *image, int tries, int iterations, int num_colors, const uint8_t *init,
                           void *workspace, uint8_t *best, RdfColorMappingResult *result, void *stream)
{
    if (n_px < 0 || tries < 1 || tries > kMaxTries || iterations < 1 || num_colors < 1 || num_colors > kMaxK)
        return RDF_ERR_BAD_ARG;
    if (!init || !workspace || !best || (n_px > 0 && !image)) return RDF_ERR_NULL_PTR;
    if (misaligned(image, 4) || misaligned(workspace, 8) || misaligned(result, 8)) return RDF_ERR_BAD_ARG;
    uint8_t *colors = static_cast<uint8_t *>(workspace);
    u64 *sums = reinterpret_cast<u64 *>(colors + colors_bytes(tries, num_colors));
    hipLaunchKernelGGL(k_mapping_init, dim3(1), dim3(kFlatThreads), 0, S(stream), tries, num_colors, init, colors, sums);
    for (int it = 0; it < iterations; ++it) {
        if (n_px > 0)
            hipLaunchKernelGGL((k_accum<false>), dim3(accum_blocks(n_px)), dim3(kAccThreads), 0, S(stream), n_px, image, tries,
                               num_colors, colors, sums);
        hipLaunchKernelGGL(k_mapping_update, dim3(1), dim3(kUpdThreads), 0, S(stream), tries, num_colors, colors, sums,
                           it == iterations - 1 ? 1 : 0, best, result);
    }
    return (int)hipGetLastError();
}

int rdf_label_frame(int dim_x, int dim_y, int num_colors, const uint8_t *mapping, uint8_t *image,
                    const uint16_t *mask_labels, int mask_label, uint16_t *depth, uint16_t *labels, uint8_t *labels_rgba,
                    void *stream)
{
    if (num_colors < 1) return RDF_ERR_BAD_ARG;
    if ((long long)dim_x * dim_y > 0 && !labels) return RDF_ERR_NULL_PTR;
    return label_launch(dim_x, dim_y, num_colors, mapping, image, mask_labels, mask_label, depth, labels, labels_rgba, stream);
}

int rdf_mask_color_image(int dim_x, int dim_y, uint8_t *image, const uint16_t *mask_labels, int mask_label, void *stream)
{
    if ((long long)dim_x * dim_y > 0 && !mask_labels) return RDF_ERR_NULL_PTR;
    return label_launch(dim_x, dim_y, 0, nullptr, image, mask_labels, mask_label, nullptr, nullptr, nullptr, stream);
}

int rdf_labels_abi_version(void) { return RDF_LABELS_ABI_VERSION; }

#ifndef RDF_BUILD_ID
#define RDF_BUILD_ID "unknown"
#endif
// (the marker in front lets a build script find the id in the file without loading it)
static const char kLabelsBuildIdMarker[] = "rdf-build-id:" RDF_BUILD_ID;
const char *rdf_labels_build_id(void) { return kLabelsBuildIdMarker + 13; }

const char *rdf_labels_error_string(int code)
{
    switch (code) {
    case RDF_OK: return "ok";
    case RDF_ERR_BAD_ARG: return "rdf_labels: bad argument (colours outside 1..16, tries outside 1..8, iterations < 1, a misaligned pointer; a score with classes outside 1..64 or labels_reduce < 1; a re-render with a matrix that is not affine, f <= 0 or an empty depth range)";
    case RDF_ERR_NULL_PTR: return "rdf_labels: required pointer is NULL";
    case RDF_ERR_TOO_LARGE: return "rdf_labels: call addresses >= 2^31 elements";
    default: return code > 0 ? hipGetErrorString(static_cast<hipError_t>(code)) : "rdf_labels: unknown error";
    }
}

}  // extern "C"
