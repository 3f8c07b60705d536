// frontend_hip.hip -- the depth front end on the device: the RANSAC table plane (CalibratedPlane, src/calibrated_plane.py,
// src/cuda/calibrated_plane.cu) and the per-frame chain raw depth -> table-free depth (src/3d_bz.py:163-212).  Built into
// its own librdf_frontend.so.  The contract, and its deviations from the reference, are in include/rdf_frontend.h.
//
// Every fp32 operation order that comes from glm 0.9.9 lives in the four device functions below (mat4_row, dot3,
// normalize3, cross3); -ffp-contract=off keeps each multiply and add separate.
//
// k_plane_inliers is the hot path: ~1.0e10 point-plane tests per calibration at 848x480 x 25 000 candidates.  A workgroup
// of 1024 lanes holds kPtsPerLane points per lane in VGPRs (invalid points as NaN, which no candidate counts) and walks a
// chunk of kCandChunk candidates whose z-rows are wave-uniform scalar loads.  Per point and candidate: 3 mul + 3 add +
// 1 compare -> the wave mask -> s_bcnt1 into a scalar count.  One LDS atomic per (wave, candidate), then at most one
// global atomic per (workgroup, candidate), and none for a zero count.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/rdf_frontend.h"
#include "rdf_kernel_util.hpp"

namespace {

constexpr int kCandThreads = 64;
constexpr int kInlThreads = 1024;
constexpr int kInlWaves = kInlThreads / 64;
constexpr int kPtsPerLane = 16;
constexpr int kPtsPerBlock = kInlThreads * kPtsPerLane;
constexpr int kCandChunk = 64;
constexpr int kSelThreads = 256;
constexpr int kTileX = 32, kTileY = 8;
constexpr int kMaxK = RDF_FRONTEND_MAX_FILTER;
constexpr int kHaloW = kTileX + kMaxK - 1, kHaloH = kTileY + kMaxK - 1;
constexpr int kFlatThreads = 256;

struct Mat4 {
    float m[16];
};

// ---- glm 0.9.9's arithmetic, in its order ----
// mat4 * vec4, row i of the row-major M: (Mul0 + Mul1) + (Mul2 + Mul3)
__device__ __forceinline__ float mat4_row(const float *r, float x, float y, float z, float w)
{
    return (r[0] * x + r[1] * y) + (r[2] * z + r[3] * w);
}
__device__ __forceinline__ float dot3(float3 v) { return (v.x * v.x + v.y * v.y) + v.z * v.z; }
__device__ __forceinline__ float3 normalize3(float3 v)
{
    const float s = 1.f / sqrtf(dot3(v));
    return make_float3(v.x * s, v.y * s, v.z * s);
}
__device__ __forceinline__ float3 cross3(float3 a, float3 b)
{
    return make_float3(a.y * b.z - b.y * a.z, a.z * b.x - b.z * a.x, a.x * b.y - b.x * a.y);
}

// ---- the per-pixel chain (points_ops.cu:5-36, 63-73; calibrated_plane.cu:31-46; points_ops.cu:131-146) ----
__device__ __forceinline__ float4 deproject(uint16_t d, int x, int y, float ppx, float ppy, float f)
{
    const float df = (float)d;
    return make_float4((df * ((float)x - ppx)) / f, (df * ((float)y - ppy)) / f, df, 1.f);
}

__device__ __forceinline__ float4 transform(const float *M, float4 p)
{
    return make_float4(mat4_row(M, p.x, p.y, p.z, p.w), mat4_row(M + 4, p.x, p.y, p.z, p.w),
                       mat4_row(M + 8, p.x, p.y, p.z, p.w), mat4_row(M + 12, p.x, p.y, p.z, p.w));
}

__device__ __forceinline__ bool filtered_by_plane(float4 p, float T) { return p.w == 1.f && p.z > -T; }

// the cleaned depth of one pixel; *pt = its plane-space point, or zeros where the depth or the point was removed
__device__ __forceinline__ uint16_t front_pixel(uint16_t d, int x, int y, float ppx, float ppy, float f, const float *M,
                                                float T, float4 *pt)
{
    *pt = make_float4(0.f, 0.f, 0.f, 0.f);
    if (d == 0) return 0;
    const float4 p = transform(M, deproject(d, x, y, ppx, ppy, f));
    if (filtered_by_plane(p, T)) return 0;
    *pt = p;
    return p.w == 0.f ? (uint16_t)0 : d;
}

// __float2uint_rd: floor, saturate to [0, 2^32 - 1], NaN -> 0
__device__ __forceinline__ uint32_t float2uint_rd(float v)
{
    const float q = floorf(v);
    if (!(q > 0.f)) return 0u;
    if (q >= 4294967296.f) return 0xffffffffu;
    return (uint32_t)q;
}

// ---- plane candidates: one lane per candidate (calibrated_plane.cu:51-90) ----
__global__ void __launch_bounds__(kCandThreads) k_plane_candidates(int G, int dim_x, int dim_y, const float *__restrict__ rand,
                                                                   const float4 *__restrict__ pts, const float *__restrict__ start_mat,
                                                                   float *__restrict__ cand, int32_t *__restrict__ counts)
{
    const int i = blockIdx.x * kCandThreads + threadIdx.x;
    if (i >= G) return;
    float *out = cand + (size_t)i * 16;
    if (i == 0 && start_mat) {
        for (int k = 0; k < 16; ++k) out[k] = start_mat[k];
        if (counts) counts[0] = 0;
        return;
    }
    const long long N = (long long)dim_x * dim_y;
    const float fx = (float)dim_x, fy = (float)dim_y;
    float3 P[3];
    int set = 0;
    for (int j = 0; j < 32 && set < 3; ++j) {
        const float v = floorf((rand[(size_t)i * 32 + j] * fx) * fy);
        if (!(v >= 0.f) || (double)v >= (double)N) continue;      // r outside [0, N): a miss (the reference reads out of bounds)
        const float4 p = pts[(long long)v];
        if (p.z > 0.f) P[set++] = make_float3(p.x, p.y, p.z);
    }
    if (set < 3) {
        for (int k = 0; k < 16; ++k) out[k] = __builtin_nanf("");
        if (counts) counts[i] = -1;
        return;
    }
    const float3 v0 = normalize3(make_float3(P[1].x - P[0].x, P[1].y - P[0].y, P[1].z - P[0].z));
    const float3 v1 = normalize3(make_float3(P[2].x - P[0].x, P[2].y - P[0].y, P[2].z - P[0].z));
    const float3 za = normalize3(cross3(v0, v1));
    const float3 xa = v0;
    const float3 ya = normalize3(cross3(za, xa));
    const float M[16] = {xa.x, ya.x, za.x, -P[0].x,
                         xa.y, ya.y, za.y, -P[0].y,
                         xa.z, ya.z, za.z, -P[0].z,
                         0.f, 0.f, 0.f, 1.f};
    for (int k = 0; k < 16; ++k) out[k] = M[k];
    if (counts) counts[i] = 0;
}

// ---- inlier counts: points x candidates, the hot path ----
__global__ void __launch_bounds__(kInlThreads) k_plane_inliers(int G, float T, int n_pts, const float4 *__restrict__ pts,
                                                               const float *__restrict__ cand, int32_t *__restrict__ counts)
{
    __shared__ int32_t part[kCandChunk];
    const int tid = threadIdx.x;
    const int c0 = blockIdx.y * kCandChunk;
    const int nc = min(kCandChunk, G - c0);
    if (tid < kCandChunk) part[tid] = 0;

    float px[kPtsPerLane], py[kPtsPerLane], pz[kPtsPerLane];
    const long long base = (long long)blockIdx.x * kPtsPerBlock + tid;
#pragma unroll
    for (int k = 0; k < kPtsPerLane; ++k) {
        const long long idx = base + (long long)k * kInlThreads;
        float4 p = make_float4(__builtin_nanf(""), 0.f, 0.f, 0.f);
        if (idx < n_pts) p = pts[idx];
        const bool ok = p.w == 1.f;                    // w == 1; a NaN x makes z' NaN for every candidate: never an inlier
        px[k] = ok ? p.x : __builtin_nanf("");
        py[k] = p.y;
        pz[k] = p.z;
    }
    __syncthreads();

    for (int c = 0; c < nc; ++c) {
        const float *r = cand + (size_t)(c0 + c) * 16 + 8;    // row 2, wave-uniform
        const float m0 = r[0], m1 = r[1], m2 = r[2], m3 = r[3];
        int cnt = 0;
#pragma unroll
        for (int k = 0; k < kPtsPerLane; ++k) {
            const float z = (m0 * px[k] + m1 * py[k]) + (m2 * pz[k] + m3 * 1.f);
            cnt += __popcll(__ballot(fabsf(z) < T));        // z < T && z > -T
        }
        if (cnt && (tid & 63) == 0) atomicAdd(&part[c], cnt);
    }
    __syncthreads();
    if (tid < nc && part[tid]) atomicAdd(&counts[c0 + tid], part[tid]);
}

// ---- winner and recentring: one workgroup (calibrated_plane.py:70-87) ----
__global__ void __launch_bounds__(kSelThreads) k_plane_select(int G, const float *__restrict__ cand,
                                                              const int32_t *__restrict__ counts, float *__restrict__ plane,
                                                              RdfPlaneResult *__restrict__ result)
{
    __shared__ unsigned long long best;
    if (threadIdx.x == 0) best = 0;
    __syncthreads();
    unsigned long long mine = 0;
    for (int i = threadIdx.x; i < G; i += kSelThreads) {
        // highest count first, then the lowest index: (count + 2^31) << 32 | ~i
        const unsigned long long key = ((unsigned long long)((uint32_t)counts[i] ^ 0x80000000u) << 32) | (uint32_t)~(uint32_t)i;
        mine = key > mine ? key : mine;
    }
    atomicMax(&best, mine);
    __syncthreads();
    if (threadIdx.x != 0) return;
    const int bi = (int)~(uint32_t)best;
    const int bc = (int)((uint32_t)(best >> 32) ^ 0x80000000u);
    float M[16];
    for (int k = 0; k < 16; ++k) M[k] = cand[(size_t)bi * 16 + k];
    const float t = (-M[11]) / M[10];
    double c[4];
    for (int r = 0; r < 4; ++r)
        c[r] = (((double)M[r * 4] * 0.0 + (double)M[r * 4 + 1] * 0.0) + (double)M[r * 4 + 2] * (double)t) + (double)M[r * 4 + 3] * 1.0;
    const bool ok = bc > 0 && fabs(c[2]) < 0.001;
    if (ok) {
        M[3] = M[3] + -(float)c[0];
        M[7] = M[7] + -(float)c[1];
        for (int k = 0; k < 16; ++k) plane[k] = M[k];
    }
    if (result) {
        for (int k = 0; k < 16; ++k) result->plane[k] = ok ? M[k] : plane[k];
        result->best_index = bi;
        result->best_count = bc;
        for (int r = 0; r < 4; ++r) result->c[r] = c[r];
        result->status = ok ? RDF_PLANE_OK : RDF_PLANE_NONE;
        result->reserved = 0;
    }
}

// ---- the per-frame chain, tiled; the Gaussian reads a halo of cleaned depth from LDS ----
// CLEAN: depth -> cleaned depth (+ points); GAUSS: then the Gaussian filter of the cleaned image.  CLEAN = false, GAUSS =
// true is the stand-alone gaussian_depth_filter.
template <bool CLEAN, bool GAUSS>
__global__ void __launch_bounds__(kTileX * kTileY) k_frame_front(const uint16_t *__restrict__ depth, int W, int H, float ppx,
                                                                 float ppy, float f, const float *__restrict__ plane, float T,
                                                                 const float *__restrict__ gauss, int k,
                                                                 uint16_t *__restrict__ out, float4 *__restrict__ pts_out)
{
    __shared__ uint16_t tile[GAUSS ? kHaloW * kHaloH : 1];
    __shared__ float wk[GAUSS ? kMaxK * kMaxK : 1];
    __shared__ float Ms[16];
    const int tid = threadIdx.y * kTileX + threadIdx.x;
    const size_t frame = (size_t)blockIdx.z * W * H;
    const uint16_t *d_in = depth + frame;
    const int x = blockIdx.x * kTileX + threadIdx.x, y = blockIdx.y * kTileY + threadIdx.y;
    if (CLEAN && tid < 16) Ms[tid] = plane[tid];
    if (GAUSS)
        for (int i = tid; i < k * k; i += kTileX * kTileY) wk[i] = gauss[i];
    __syncthreads();
    float4 pt;
    if (!GAUSS) {
        if (x >= W || y >= H) return;
        const size_t i = frame + (size_t)y * W + x;
        out[i] = front_pixel(d_in[(size_t)y * W + x], x, y, ppx, ppy, f, Ms, T, &pt);
        if (pts_out) pts_out[i] = pt;
        return;
    }
    const int h = k / 2, lw = kTileX + k - 1, lh = kTileY + k - 1;
    const int ox = blockIdx.x * kTileX - h, oy = blockIdx.y * kTileY - h;
    for (int i = tid; i < lw * lh; i += kTileX * kTileY) {
        const int gx = ox + i % lw, gy = oy + i / lw;
        uint16_t v = 0;
        if (gx >= 0 && gy >= 0 && gx < W && gy < H) {
            v = d_in[(size_t)gy * W + gx];
            if (CLEAN) v = front_pixel(v, gx, gy, ppx, ppy, f, Ms, T, &pt);
        }
        tile[i] = v;
    }
    __syncthreads();
    if (x >= W || y >= H) return;
    float w0 = 0.f, wn = 0.f, sum = 0.f;
    for (int dy = 0; dy < k; ++dy) {
        const int cy = y + dy - h;
        if (cy < 0 || cy >= H) continue;
        for (int dx = 0; dx < k; ++dx) {
            const int cx = x + dx - h;
            if (cx < 0 || cx >= W) continue;
            const uint16_t d = tile[(threadIdx.y + dy) * lw + threadIdx.x + dx];
            const float w = wk[dy * k + dx];
            if (d == 0) {
                w0 += w;
            } else {
                wn += w;
                sum += (float)d * w;
            }
        }
    }
    const size_t i = frame + (size_t)y * W + x;
    out[i] = w0 > wn ? (uint16_t)0 : (uint16_t)float2uint_rd(sum / wn);
    if (CLEAN && pts_out) {
        front_pixel(d_in[(size_t)y * W + x], x, y, ppx, ppy, f, Ms, T, &pt);
        pts_out[i] = pt;
    }
}

// ---- the reference's stand-alone kernels ----
__global__ void k_deproject(int n, int W, int H, float ppx, float ppy, float f, const uint16_t *__restrict__ depth,
                            float4 *__restrict__ pts)
{
    const size_t i = (size_t)blockIdx.x * kFlatThreads + threadIdx.x;
    if (i >= (size_t)n * W * H) return;
    const int x = (int)(i % W), y = (int)((i / W) % H);
    const uint16_t d = depth[i];
    if (d > 0) pts[i] = deproject(d, x, y, ppx, ppy, f);
}

__global__ void k_transform(int n, float4 *__restrict__ pts, Mat4 M)
{
    const int i = blockIdx.x * kFlatThreads + threadIdx.x;
    if (i >= n) return;
    const float4 p = pts[i];
    if (p.w != 1.f) return;
    pts[i] = transform(M.m, p);
}

__global__ void k_filter(int n, float T, float4 *__restrict__ pts)
{
    const int i = blockIdx.x * kFlatThreads + threadIdx.x;
    if (i >= n) return;
    if (filtered_by_plane(pts[i], T)) pts[i] = make_float4(0.f, 0.f, 0.f, 0.f);
}

__global__ void k_remove_missing(int n, const float4 *__restrict__ pts, uint16_t *__restrict__ depth)
{
    const int i = blockIdx.x * kFlatThreads + threadIdx.x;
    if (i >= n) return;
    if (pts[i].w == 0.f) depth[i] = 0;
}

constexpr long long kMaxElems = 1ll << 31;

}  // namespace

extern "C" {

int rdf_make_plane_candidates(int G, int dim_x, int dim_y, const float *rand, const float *pts, const float *start_mat,
                              float *candidates, int32_t *counts, void *stream)
{
    if (G < 0 || dim_x < 0 || dim_y < 0) return RDF_ERR_BAD_ARG;
    if (G == 0) return RDF_OK;
    if (!rand || !pts || !candidates) return RDF_ERR_NULL_PTR;
    if ((long long)dim_x * dim_y >= kMaxElems || (long long)G * 32 >= kMaxElems) return RDF_ERR_TOO_LARGE;
    hipLaunchKernelGGL(k_plane_candidates, dim3(blocks(G, kCandThreads)), dim3(kCandThreads), 0, S(stream), G, dim_x, dim_y,
                       rand, reinterpret_cast<const float4 *>(pts), start_mat, candidates, counts);
    return (int)hipGetLastError();
}

int rdf_plane_inliers(int G, float threshold, int n_pts, const float *pts, const float *candidates, int32_t *counts,
                      void *stream)
{
    if (G < 0 || n_pts < 0) return RDF_ERR_BAD_ARG;
    if (G == 0 || n_pts == 0) return RDF_OK;
    if (!pts || !candidates || !counts) return RDF_ERR_NULL_PTR;
    if (blocks(G, kCandChunk) > 65535u) return RDF_ERR_TOO_LARGE;
    hipLaunchKernelGGL(k_plane_inliers, dim3(blocks(n_pts, kPtsPerBlock), blocks(G, kCandChunk)), dim3(kInlThreads), 0,
                       S(stream), G, threshold, n_pts, reinterpret_cast<const float4 *>(pts), candidates, counts);
    return (int)hipGetLastError();
}

int rdf_plane_select(int G, const float *candidates, const int32_t *counts, float *plane_inout, RdfPlaneResult *result,
                     void *stream)
{
    if (G <= 0) return RDF_ERR_BAD_ARG;
    if (!candidates || !counts || !plane_inout) return RDF_ERR_NULL_PTR;
    hipLaunchKernelGGL(k_plane_select, dim3(1), dim3(kSelThreads), 0, S(stream), G, candidates, counts, plane_inout, result);
    return (int)hipGetLastError();
}

size_t rdf_calibrate_plane_workspace_bytes(int G)
{
    if (G <= 0) return 0;
    return (size_t)G * 64 + (((size_t)G * 4 + 15) & ~(size_t)15);
}

int rdf_calibrate_plane(int G, float threshold, int dim_x, int dim_y, const float *rand, const float *pts,
                        const float *start_mat, void *workspace, float *plane_inout, RdfPlaneResult *result, void *stream)
{
    if (G <= 0 || dim_x <= 0 || dim_y <= 0) return RDF_ERR_BAD_ARG;
    if (!rand || !pts || !workspace || !plane_inout) return RDF_ERR_NULL_PTR;
    if (misaligned(workspace, 16)) return RDF_ERR_BAD_ARG;
    float *cand = static_cast<float *>(workspace);
    int32_t *counts = reinterpret_cast<int32_t *>(static_cast<char *>(workspace) + (size_t)G * 64);
    int rc = rdf_make_plane_candidates(G, dim_x, dim_y, rand, pts, start_mat, cand, counts, stream);
    if (rc == RDF_OK) rc = rdf_plane_inliers(G, threshold, dim_x * dim_y, pts, cand, counts, stream);
    if (rc == RDF_OK) rc = rdf_plane_select(G, cand, counts, plane_inout, result, stream);
    return rc;
}

int rdf_frame_front(const uint16_t *depth, int n, int dim_x, int dim_y, float ppx, float ppy, float f, const float *plane,
                    float threshold, const float *gauss, int k, uint16_t *depth_out, float *pts_out, void *stream)
{
    if (n < 0 || dim_x < 0 || dim_y < 0) return RDF_ERR_BAD_ARG;
    if (gauss && (k < 1 || k > kMaxK || k % 2 == 0)) return RDF_ERR_BAD_ARG;
    if ((long long)n * dim_x * dim_y == 0) return RDF_OK;
    if (!depth || !plane || !depth_out) return RDF_ERR_NULL_PTR;
    if (gauss && depth_out == depth) return RDF_ERR_BAD_ARG;
    if ((long long)n * dim_x * dim_y >= kMaxElems || n > 65535) return RDF_ERR_TOO_LARGE;
    const dim3 grid(blocks(dim_x, kTileX), blocks(dim_y, kTileY), (unsigned)n), block(kTileX, kTileY);
    float4 *po = reinterpret_cast<float4 *>(pts_out);
    if (gauss)
        hipLaunchKernelGGL((k_frame_front<true, true>), grid, block, 0, S(stream), depth, dim_x, dim_y, ppx, ppy, f, plane,
                           threshold, gauss, k, depth_out, po);
    else
        hipLaunchKernelGGL((k_frame_front<true, false>), grid, block, 0, S(stream), depth, dim_x, dim_y, ppx, ppy, f, plane,
                           threshold, gauss, 0, depth_out, po);
    return (int)hipGetLastError();
}

int rdf_deproject_points(int n, int dim_x, int dim_y, float ppx, float ppy, float f, const uint16_t *depth, float *pts,
                         void *stream)
{
    if (n < 0 || dim_x < 0 || dim_y < 0) return RDF_ERR_BAD_ARG;
    const long long total = (long long)n * dim_x * dim_y;
    if (total == 0) return RDF_OK;
    if (!depth || !pts) return RDF_ERR_NULL_PTR;
    if (total >= kMaxElems) return RDF_ERR_TOO_LARGE;
    hipLaunchKernelGGL(k_deproject, dim3(blocks(total, kFlatThreads)), dim3(kFlatThreads), 0, S(stream), n, dim_x, dim_y, ppx,
                       ppy, f, depth, reinterpret_cast<float4 *>(pts));
    return (int)hipGetLastError();
}

int rdf_transform_points(int n_pts, float *pts, const float *plane_host, void *stream)
{
    if (n_pts < 0) return RDF_ERR_BAD_ARG;
    if (n_pts == 0) return RDF_OK;
    if (!pts || !plane_host) return RDF_ERR_NULL_PTR;
    Mat4 M;
    for (int k = 0; k < 16; ++k) M.m[k] = plane_host[k];
    hipLaunchKernelGGL(k_transform, dim3(blocks(n_pts, kFlatThreads)), dim3(kFlatThreads), 0, S(stream), n_pts,
                       reinterpret_cast<float4 *>(pts), M);
    return (int)hipGetLastError();
}

int rdf_filter_points_by_plane(int n_pts, float threshold, float *pts, void *stream)
{
    if (n_pts < 0) return RDF_ERR_BAD_ARG;
    if (n_pts == 0) return RDF_OK;
    if (!pts) return RDF_ERR_NULL_PTR;
    hipLaunchKernelGGL(k_filter, dim3(blocks(n_pts, kFlatThreads)), dim3(kFlatThreads), 0, S(stream), n_pts, threshold,
                       reinterpret_cast<float4 *>(pts));
    return (int)hipGetLastError();
}

int rdf_remove_missing_3d_points_from_depth_image(int n_pts, const float *pts, uint16_t *depth, void *stream)
{
    if (n_pts < 0) return RDF_ERR_BAD_ARG;
    if (n_pts == 0) return RDF_OK;
    if (!pts || !depth) return RDF_ERR_NULL_PTR;
    hipLaunchKernelGGL(k_remove_missing, dim3(blocks(n_pts, kFlatThreads)), dim3(kFlatThreads), 0, S(stream), n_pts,
                       reinterpret_cast<const float4 *>(pts), depth);
    return (int)hipGetLastError();
}

int rdf_gaussian_depth_filter(int dim_x, int dim_y, int k, const float *gauss, const uint16_t *d_in, uint16_t *d_out,
                              void *stream)
{
    if (dim_x < 0 || dim_y < 0 || k < 1 || k > kMaxK || k % 2 == 0) return RDF_ERR_BAD_ARG;
    if ((long long)dim_x * dim_y == 0) return RDF_OK;
    if (!gauss || !d_in || !d_out) return RDF_ERR_NULL_PTR;
    if (d_in == d_out) return RDF_ERR_BAD_ARG;
    if ((long long)dim_x * dim_y >= kMaxElems) return RDF_ERR_TOO_LARGE;
    const dim3 grid(blocks(dim_x, kTileX), blocks(dim_y, kTileY), 1), block(kTileX, kTileY);
    hipLaunchKernelGGL((k_frame_front<false, true>), grid, block, 0, S(stream), d_in, dim_x, dim_y, 0.f, 0.f, 1.f, nullptr,
                       0.f, gauss, k, d_out, nullptr);
    return (int)hipGetLastError();
}

int rdf_frontend_abi_version(void) { return RDF_FRONTEND_ABI_VERSION; }

#ifndef RDF_BUILD_ID
#define RDF_BUILD_ID "unknown"
#endif
// (the marker in front lets a build script find the id in the file without loading it)
static const char kFrontendBuildIdMarker[] = "rdf-build-id:" RDF_BUILD_ID;
const char *rdf_frontend_build_id(void) { return kFrontendBuildIdMarker + 13; }

const char *rdf_frontend_error_string(int code)
{
    switch (code) {
    case RDF_OK: return "ok";
    case RDF_ERR_BAD_ARG: return "rdf_frontend: bad argument";
    case RDF_ERR_NULL_PTR: return "rdf_frontend: required pointer is NULL";
    case RDF_ERR_CAPTURE: return "rdf_frontend: the stream is being captured into a graph and this call cannot be recorded";
    case RDF_ERR_TOO_LARGE: return "rdf_frontend: call addresses >= 2^31 elements (or too many candidates / frames for one grid)";
    default: return code > 0 ? hipGetErrorString(static_cast<hipError_t>(code)) : "rdf_frontend: unknown error";
    }
}

}  // extern "C"
