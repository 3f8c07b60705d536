// rerender_hip.hip -- the converter's augmentation step on the device: the centre of a frame's points and the re-render of
// the reference's rerender_image (src/live_data_convert.py:207-282, 363-364), which goes through make_triangles
// (src/cuda/points_ops.cu:77-115) and an OpenGL draw of std_camera.vert / .frag.  There is no display on an MI355X node, so
// this is a software rasteriser.  Built into librdf_labels.so; the rules (mesh, vertex, projection, coverage, attributes,
// depth test) are in include/rdf_labels.h and restated in tests/rerender_numpy.py, and the numbering below is the header's.
//
// k_raster: a workgroup owns 64 x 4 quads.  Their 65 x 5 corner points are transformed, projected and snapped ONCE each into
// LDS (a corner is shared by four quads), then one lane per quad sets up its two triangles from LDS, walks their bounding
// boxes clipped to the frame (one to four pixels at the converter's variances) and issues one 64-bit atomicMin per covered
// pixel into the key buffer.  k_resolve: one lane per pixel takes the winning key, rebuilds that one triangle from global
// memory with the same arithmetic (so the same z), writes depth and colour and resets the key to empty.
// Everything that decides coverage is integer; the fp32 part is evaluated in the header's order and the library is built
// with -ffp-contract=off, so the second pass reproduces the first and the result does not depend on the order of arrival.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/rdf_labels.h"
#include "rdf_kernel_util.hpp"
#include "rdf_raster.hpp"

namespace {

constexpr int kTileX = 64, kTileY = 4;                  // quads per workgroup
constexpr int kVtxX = kTileX + 1, kVtxY = kTileY + 1;   // their corner points
constexpr int kRasterThreads = kTileX * kTileY;
constexpr int kFlatThreads = 256;
constexpr int kCenterThreads = 256, kCenterMaxBlocks = 1024;
constexpr uint32_t kHasPoint = 1u, kDrawable = 2u;      // vertex flags, bits 24 and 25 of Vtx::c

struct Camera {
    float m[12];                    // the first three rows of obj_tform
    Pinhole p;
};

struct Vtx {
    int X, Y;                       // snapped screen position, 1/256 pixel
    float z;                        // z'
    uint32_t c;                     // r | g << 8 | b << 16 | flags << 24
};

// rules 2 and 3, with the point's colour and what rules 1 and 3 ask of it packed beside them
__device__ __forceinline__ Vtx load_vertex(const float4 *__restrict__ pts, const uint8_t *__restrict__ color, long long at,
                                           const Camera &cam)
{
    const float4 p = pts[at];
    const uint8_t *c = color + at * 3;
    const Snapped v = project_point(cam.m, p.x, p.y, p.z, cam.p);
    const uint32_t flags = (p.w > 0.f ? kHasPoint : 0u) | (v.drawable ? kDrawable : 0u);
    return {v.X, v.Y, v.z, (uint32_t)c[0] | ((uint32_t)c[1] << 8) | ((uint32_t)c[2] << 16) | (flags << 24)};
}

__device__ __forceinline__ bool all_drawable(const Vtx &a, const Vtx &b, const Vtx &c)
{
    return (((a.c & b.c & c.c) >> 24) & kDrawable) != 0u;
}

__device__ __forceinline__ void raster_triangle(const Vtx &a, const Vtx &b, const Vtx &c, uint32_t id, int W, int H,
                                                const Camera &cam, u64 *__restrict__ keys)
{
    Tri t;
    if (!setup_triangle(a, b, c, all_drawable(a, b, c), t)) return;
    const PixelBox box = clipped_box(t, W, H);
    for (int j = box.j0; j <= box.j1; ++j)
        for (int i = box.i0; i <= box.i1; ++i) {
            float z, q[3], s;
            if (!fragment(t, i, j, cam.p, &z, q, &s)) continue;
            atomicMin(&keys[(long long)j * W + i], depth_key(z, id));       // rule 6
        }
}

__global__ void __launch_bounds__(kRasterThreads) k_raster(int W, int H, const float4 *__restrict__ pts,
                                                           const uint8_t *__restrict__ color, Camera cam,
                                                           u64 *__restrict__ keys)
{
    __shared__ Vtx vs[kVtxY * kVtxX];
    const int x0 = blockIdx.x * kTileX, y0 = blockIdx.y * kTileY;
    for (int v = threadIdx.x; v < kVtxY * kVtxX; v += kRasterThreads) {
        const int x = x0 + v % kVtxX, y = y0 + v / kVtxX;
        Vtx out = {0, 0, 0.f, 0u};
        if (x < W && y < H) out = load_vertex(pts, color, (long long)y * W + x, cam);
        vs[v] = out;
    }
    __syncthreads();
    const int lx = threadIdx.x % kTileX, ly = threadIdx.x / kTileX, x = x0 + lx, y = y0 + ly;
    if (x >= W - 1 || y >= H - 1) return;
    const Vtx p00 = vs[ly * kVtxX + lx], p01 = vs[ly * kVtxX + lx + 1];
    const Vtx p10 = vs[(ly + 1) * kVtxX + lx], p11 = vs[(ly + 1) * kVtxX + lx + 1];
    if ((((p00.c & p01.c & p10.c & p11.c) >> 24) & kHasPoint) == 0u) return;       // rule 1
    const uint32_t id = (uint32_t)(2ull * ((u64)y * (u64)(W - 1) + (u64)x));      // rule 1; below 2^32 at kMaxDim
    raster_triangle(p00, p01, p10, id, W, H, cam, keys);
    raster_triangle(p01, p10, p11, id + 1, W, H, cam, keys);
}

__device__ __forceinline__ uint32_t channel(const float q[3], float s, const uint32_t c[3], int shift)
{
    const float c0 = (float)((c[0] >> shift) & 0xffu), c1 = (float)((c[1] >> shift) & 0xffu), c2 = (float)((c[2] >> shift) & 0xffu);
    const float v = floorf(((q[0] * c0 + q[1] * c1) + q[2] * c2) / s + 0.5f);
    return v >= 255.f ? 255u : v > 0.f ? (uint32_t)v : 0u;
}

// A key that no call of k_raster can have left (a workspace that was not filled with 0xFF) names no triangle of this
// frame: it is treated as empty rather than followed out of the buffers.
__global__ void __launch_bounds__(kFlatThreads) k_resolve(int W, int H, const float4 *__restrict__ pts,
                                                          const uint8_t *__restrict__ color, Camera cam,
                                                          u64 *__restrict__ keys, uint16_t *__restrict__ depth_out,
                                                          uint8_t *__restrict__ color_out)
{
    const long long p = (long long)blockIdx.x * kFlatThreads + threadIdx.x;
    if (p >= (long long)W * H) return;
    const u64 key = keys[p];
    uint16_t d = 0;
    uint32_t r = 0u, g = 0u, b = 0u;
    if (key != kEmptyKey) {
        keys[p] = kEmptyKey;
        const u64 id = key_id(key);
        const u64 n_tri = W > 1 && H > 1 ? 2ull * (u64)(W - 1) * (u64)(H - 1) : 0ull;
        if (id < n_tri) {
            const long long quad = (long long)(id >> 1), x = quad % (W - 1), y = quad / (W - 1);
            const long long at = y * W + x;
            const int k = (int)(id & 1ull);
            const Vtx v0 = load_vertex(pts, color, k ? at + 1 : at, cam);
            const Vtx v1 = load_vertex(pts, color, k ? at + W : at + 1, cam);
            const Vtx v2 = load_vertex(pts, color, k ? at + W + 1 : at + W, cam);
            const uint32_t c[3] = {v0.c, v1.c, v2.c};
            Tri t;
            float z, q[3], s;
            if (setup_triangle(v0, v1, v2, all_drawable(v0, v1, v2), t) &&
                fragment(t, (int)(p % W), (int)(p / W), cam.p, &z, q, &s)) {
                d = depth_u16(z);
                r = channel(q, s, c, 0);
                g = channel(q, s, c, 8);
                b = channel(q, s, c, 16);
            }
        }
    }
    depth_out[p] = d;
    uint8_t *o = color_out + p * 3;
    o[0] = (uint8_t)r;
    o[1] = (uint8_t)g;
    o[2] = (uint8_t)b;
}

// the workgroup's sum of v[0..3] over its lanes, halving; valid in lane 0..3 as component `lane` after the call
__device__ __forceinline__ double block_sum4(double v[4], double (*sh)[kCenterThreads])
{
    const int t = threadIdx.x;
#pragma unroll
    for (int c = 0; c < 4; ++c) sh[c][t] = v[c];
    __syncthreads();
    for (int s = kCenterThreads / 2; s >= 1; s >>= 1) {
        if (t < s) {
#pragma unroll
            for (int c = 0; c < 4; ++c) sh[c][t] += sh[c][t + s];
        }
        __syncthreads();
    }
    return t < 4 ? sh[t][0] : 0.;
}

__global__ void __launch_bounds__(kCenterThreads) k_center_partial(long long n, const float4 *__restrict__ pts,
                                                                   double *__restrict__ partial)
{
    __shared__ double sh[4][kCenterThreads];
    double v[4] = {0., 0., 0., 0.};
    for (long long i = (long long)blockIdx.x * kCenterThreads + threadIdx.x; i < n; i += (long long)gridDim.x * kCenterThreads) {
        const float4 p = pts[i];
        v[0] += (double)p.x;
        v[1] += (double)p.y;
        v[2] += (double)p.z;
        v[3] += (double)p.w;
    }
    const double sum = block_sum4(v, sh);
    if (threadIdx.x < 4) partial[(long long)blockIdx.x * 4 + threadIdx.x] = sum;
}

__global__ void __launch_bounds__(kCenterThreads) k_center_final(int n_partial, const double *__restrict__ partial,
                                                                 double *__restrict__ sums)
{
    __shared__ double sh[4][kCenterThreads];
    double v[4] = {0., 0., 0., 0.};
    for (int i = threadIdx.x; i < n_partial; i += kCenterThreads) {
#pragma unroll
        for (int c = 0; c < 4; ++c) v[c] += partial[i * 4 + c];
    }
    const double sum = block_sum4(v, sh);
    if (threadIdx.x < 4) sums[threadIdx.x] = sum;
}

inline int center_blocks(long long n)
{
    const long long b = (n + kCenterThreads - 1) / kCenterThreads;
    return (int)(b < kCenterMaxBlocks ? b : kCenterMaxBlocks);
}

}  // namespace

extern "C" {

size_t rdf_points_center_workspace_bytes(int n_pts)
{
    if (n_pts < 0) return 0;
    const int b = center_blocks(n_pts);
    return (size_t)(b > 0 ? b : 1) * 4 * sizeof(double);
}

int rdf_points_center(int n_pts, const float *pts, void *workspace, double *sums, void *stream)
{
    if (n_pts < 0) return RDF_ERR_BAD_ARG;
    if (!workspace || !sums || (n_pts > 0 && !pts)) return RDF_ERR_NULL_PTR;
    if (misaligned(pts, 16) || misaligned(workspace, 8) || misaligned(sums, 8)) return RDF_ERR_BAD_ARG;
    const int b = center_blocks(n_pts);
    double *partial = static_cast<double *>(workspace);
    if (b > 0)
        hipLaunchKernelGGL(k_center_partial, dim3((unsigned)b), dim3(kCenterThreads), 0, S(stream), (long long)n_pts,
                           reinterpret_cast<const float4 *>(pts), partial);
    hipLaunchKernelGGL(k_center_final, dim3(1), dim3(kCenterThreads), 0, S(stream), b, partial, sums);
    return (int)hipGetLastError();
}

size_t rdf_rerender_workspace_bytes(int dim_x, int dim_y)
{
    if (dim_x < 0 || dim_y < 0 || dim_x > kMaxDim || dim_y > kMaxDim) return 0;
    return (size_t)dim_x * (size_t)dim_y * sizeof(u64);
}

int rdf_rerender(int dim_x, int dim_y, const float *pts, const uint8_t *color, const float *obj_tform_host, float f,
                 float ppx, float ppy, float zmin, float zmax, void *workspace, uint16_t *depth_out, uint8_t *color_out,
                 void *stream)
{
    if (dim_x < 0 || dim_y < 0) return RDF_ERR_BAD_ARG;
    if (dim_x > kMaxDim || dim_y > kMaxDim) return RDF_ERR_TOO_LARGE;
    Camera cam;
    cam.p = {f, ppx, ppy, zmin, zmax};
    if (!pinhole_ok(cam.p)) return RDF_ERR_BAD_ARG;
    const long long n_px = (long long)dim_x * dim_y;
    if (n_px == 0) return RDF_OK;
    if (!pts || !color || !obj_tform_host || !workspace || !depth_out || !color_out) return RDF_ERR_NULL_PTR;
    if (misaligned(pts, 16) || misaligned(workspace, 8) || misaligned(depth_out, 2) || color_out == color)
        return RDF_ERR_BAD_ARG;
    const float *m = obj_tform_host;
    if (m[12] != 0.f || m[13] != 0.f || m[14] != 0.f || m[15] != 1.f) return RDF_ERR_BAD_ARG;      // affine only
    for (int k = 0; k < 12; ++k) cam.m[k] = m[k];
    u64 *keys = static_cast<u64 *>(workspace);
    const float4 *p4 = reinterpret_cast<const float4 *>(pts);
    if (dim_x > 1 && dim_y > 1)
        hipLaunchKernelGGL(k_raster, dim3(blocks(dim_x - 1, kTileX), blocks(dim_y - 1, kTileY)), dim3(kRasterThreads), 0,
                           S(stream), dim_x, dim_y, p4, color, cam, keys);
    hipLaunchKernelGGL(k_resolve, dim3(blocks(n_px, kFlatThreads)), dim3(kFlatThreads), 0, S(stream), dim_x, dim_y, p4, color,
                       cam, keys, depth_out, color_out);
    return (int)hipGetLastError();
}

}  // extern "C"
