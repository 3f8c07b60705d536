// hand_scene_hip.hip -- labelled depth frames of an articulated triangle mesh (the hand of hand_model.py) over an analytic
// table plane, many frames per call: the package's own source of training sets and of raw camera sequences, in place of the
// Blender scenes of the reference's datagen/.  Built into librdf_labels.so; the rules are in include/rdf_labels.h under
// rdf_hand_scene_render and restated in tests/hand_scene_numpy.py.  Projection, snapping, coverage, fill rule, depth and
// depth test are rules 3 to 6 of rdf_rerender; the device helpers for them are restated here (rerender_hip.hip keeps its own
// in its own unnamed namespace), so that file's code and register counts do not move.
//
// k_hand_raster: kLanesPerTri lanes per (frame, triangle).  Each moves the triangle's three vertices by their parts' matrices
// (a vertex is shared by about six triangles; a separate vertex pass would save those multiplications at the price of a
// third launch and of a scratch region in a workspace that is otherwise keys only), sets the triangle up and walks every
// kLanesPerTri-th row of its bounding box clipped to the frame, with one 64-bit atomicMin per covered pixel in the frame's
// key plane.  A hand's triangles cover tens to hundreds of pixels at 848x480, far more than the re-render's one to four:
// sharing a triangle's rows among neighbouring lanes shortens the longest lane's walk, which is what a wave waits for.
// k_hand_resolve: one lane per pixel of the batch.  The key itself carries what the pixel needs -- z in its high word, the
// triangle (hence the flat label) in its low word -- so nothing is rebuilt.  The table's depth along the pixel's ray, the
// hole and noise hashes, both stores and the key reset are in this pass.
// Coverage is integer, the fp32 part has a stated operation order and the library is built with -ffp-contract=off: the images
// do not depend on the order in which fragments arrive.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/rdf_labels.h"

namespace {

typedef unsigned long long u64;
constexpr u64 kEmptyKey = ~0ull;
constexpr int kThreads = 256;
constexpr int kLanesPerTri = 8;                         // raster: lanes that share a triangle's rows
constexpr int kSubPixel = 256, kHalfPixel = 128;        // 8 sub-pixel bits
constexpr float kMaxSnapped = 1048576.f;                // 2^20
constexpr int kMaxDim = 32768;                          // per axis: keeps 256 * dim in an int, and a frame's pixels below 2^31
constexpr int kMaxNoise = 32767;
constexpr unsigned kMaxGridY = 65535u;

struct Scene {
    float f, ppx, ppy, zmin, zmax;
};

struct Vtx {
    int X, Y;                       // snapped screen position, 1/256 pixel
    float z;                        // z'
    bool drawable;
};

struct Tri {
    int X[3], Y[3];
    float z[3];
    int sgn;                        // the sign of the area
    int need[3];                    // e_k >= need[k]: 0 on a top or left edge, else 1
};

// the vertex rule, then rule 3 of rdf_rerender
__device__ __forceinline__ Vtx make_vertex(const float *__restrict__ p, const float *__restrict__ m, const Scene &sc)
{
    const float px = p[0], py = p[1], pz = p[2];
    const float x = ((m[0] * px + m[1] * py) + m[2] * pz) + m[3];
    const float y = ((m[4] * px + m[5] * py) + m[6] * pz) + m[7];
    const float z = ((m[8] * px + m[9] * py) + m[10] * pz) + m[11];
    Vtx v;
    v.X = v.Y = 0;
    v.z = z;
    v.drawable = false;
    if (z > 0.f) {
        const float fx = floorf(((sc.f * x) / z + sc.ppx) * (float)kSubPixel + 0.5f);
        const float fy = floorf(((sc.f * y) / z + sc.ppy) * (float)kSubPixel + 0.5f);
        if (fabsf(fx) <= kMaxSnapped && fabsf(fy) <= kMaxSnapped) {     // (false for NaN)
            v.X = (int)fx;
            v.Y = (int)fy;
            v.drawable = true;
        }
    }
    return v;
}

__device__ __forceinline__ long long edge(int ax, int ay, int bx, int by, long long px, long long py)
{
    return (long long)(bx - ax) * (py - ay) - (long long)(by - ay) * (px - ax);
}

// rule 4, the part that does not depend on the pixel.  False: the triangle is dropped.
__device__ __forceinline__ bool setup_triangle(const Vtx &a, const Vtx &b, const Vtx &c, Tri &t)
{
    if (!(a.drawable && b.drawable && c.drawable)) return false;
    t.X[0] = a.X, t.X[1] = b.X, t.X[2] = c.X;
    t.Y[0] = a.Y, t.Y[1] = b.Y, t.Y[2] = c.Y;
    t.z[0] = a.z, t.z[1] = b.z, t.z[2] = c.z;
    const long long area = edge(a.X, a.Y, b.X, b.Y, c.X, c.Y);
    if (area == 0) return false;
    t.sgn = area > 0 ? 1 : -1;
#pragma unroll
    for (int k = 0; k < 3; ++k) {       // edge k runs from vertex k + 1 to vertex k + 2, opposite vertex k
        const int i0 = (k + 1) % 3, i1 = (k + 2) % 3;
        const int dx = t.sgn * (t.X[i1] - t.X[i0]), dy = t.sgn * (t.Y[i1] - t.Y[i0]);
        t.need[k] = (dy < 0 || (dy == 0 && dx > 0)) ? 0 : 1;
    }
    return true;
}

// rules 4 and 5 at pixel (i, j).  False: not covered, or discarded by the depth range.
__device__ __forceinline__ bool fragment(const Tri &t, int i, int j, const Scene &sc, float *z)
{
    const long long px = (long long)i * kSubPixel + kHalfPixel, py = (long long)j * kSubPixel + kHalfPixel;
    float w[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int i0 = (k + 1) % 3, i1 = (k + 2) % 3;
        const long long e = t.sgn * edge(t.X[i0], t.Y[i0], t.X[i1], t.Y[i1], px, py);
        if (e < t.need[k]) return false;
        w[k] = (float)e;
    }
    const float s = (w[0] / t.z[0] + w[1] / t.z[1]) + w[2] / t.z[2];
    *z = ((w[0] + w[1]) + w[2]) / s;
    return *z >= sc.zmin && *z <= sc.zmax;
}

__device__ __forceinline__ int imin3(int a, int b, int c) { return min(a, min(b, c)); }
__device__ __forceinline__ int imax3(int a, int b, int c) { return max(a, max(b, c)); }

// Every index read from the mesh is checked before it is followed: a triangle with a vertex outside [0, n_verts) or a
// vertex whose part is outside [0, n_parts) is dropped.  Pixel addresses come from the clipped bounding box alone.
__global__ void __launch_bounds__(kThreads) k_hand_raster(int n_frames, int W, int H, int n_verts,
                                                          const float *__restrict__ verts,
                                                          const int32_t *__restrict__ vert_part, int n_tris,
                                                          const int32_t *__restrict__ tris, int n_parts,
                                                          const float *__restrict__ part_tforms, Scene sc,
                                                          u64 *__restrict__ keys)
{
    const long long lane = (long long)blockIdx.x * kThreads + threadIdx.x;
    const int sub = (int)(lane % kLanesPerTri);
    if (lane / kLanesPerTri >= n_tris) return;
    const int t = (int)(lane / kLanesPerTri);
    int vi[3], part[3];
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        vi[k] = tris[(long long)t * 3 + k];
        ok = ok && vi[k] >= 0 && vi[k] < n_verts;
    }
    if (!ok) return;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        part[k] = vert_part[vi[k]];
        ok = ok && part[k] >= 0 && part[k] < n_parts;
    }
    if (!ok) return;
    const long long n_px = (long long)W * H;
    for (int n = blockIdx.y; n < n_frames; n += gridDim.y) {
        const float *m = part_tforms + (long long)n * n_parts * 12;
        Vtx v[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) v[k] = make_vertex(verts + (long long)vi[k] * 3, m + (long long)part[k] * 12, sc);
        Tri tr;
        if (!setup_triangle(v[0], v[1], v[2], tr)) continue;
        // the pixels whose centre 256 i + 128 lies within [min, max] (>> floors, also below zero), clipped to the frame
        const int i0 = max(0, (imin3(v[0].X, v[1].X, v[2].X) - kHalfPixel + kSubPixel - 1) >> 8);
        const int i1 = min(W - 1, (imax3(v[0].X, v[1].X, v[2].X) - kHalfPixel) >> 8);
        const int j0 = max(0, (imin3(v[0].Y, v[1].Y, v[2].Y) - kHalfPixel + kSubPixel - 1) >> 8);
        const int j1 = min(H - 1, (imax3(v[0].Y, v[1].Y, v[2].Y) - kHalfPixel) >> 8);
        u64 *plane = keys + (long long)n * n_px;
        for (int j = j0 + sub; j <= j1; j += kLanesPerTri)
            for (int i = i0; i <= i1; ++i) {
                float z;
                if (!fragment(tr, i, j, sc, &z)) continue;
                atomicMin(&plane[(long long)j * W + i], ((u64)__float_as_uint(z) << 32) | (u64)(uint32_t)t);     // rule 6
            }
    }
}

__device__ __forceinline__ uint32_t mix32(uint32_t x)
{
    x ^= x >> 16;
    x *= 0x7feb352du;
    x ^= x >> 15;
    x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}

__device__ __forceinline__ uint16_t depth_u16(float z) { return z >= 65535.f ? (uint16_t)65535 : (uint16_t)(uint32_t)z; }

// A key that no call of k_hand_raster can have left (a workspace that was not filled with 0xFF) names no triangle of this
// mesh: it is treated as empty rather than followed out of tri_label.
__global__ void __launch_bounds__(kThreads) k_hand_resolve(long long n_total, int W, int H, int n_tris,
                                                           const uint16_t *__restrict__ tri_label,
                                                           const float *__restrict__ table, Scene sc, uint16_t empty_depth,
                                                           uint32_t seed, uint32_t hole_threshold, int noise_amp,
                                                           u64 *__restrict__ keys, uint16_t *__restrict__ depth_out,
                                                           uint16_t *__restrict__ labels_out)
{
    const long long at = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (at >= n_total) return;
    const long long n_px = (long long)W * H;
    const long long n = at / n_px;
    const uint32_t p = (uint32_t)(at - n * n_px);
    const int j = (int)(p / (uint32_t)W), i = (int)(p - (uint32_t)j * (uint32_t)W);

    const u64 key = keys[at];
    bool drawn = false;
    float z = 0.f;
    uint16_t label = 0;
    if (key != kEmptyKey) {
        keys[at] = kEmptyKey;
        const uint32_t id = (uint32_t)key;
        if (id < (uint32_t)n_tris) {
            drawn = true;
            z = __uint_as_float((uint32_t)(key >> 32));
            label = tri_label[id];
        }
    }
    if (table) {
        const float *tb = table + n * 4;
        const float rx = (((float)i + 0.5f) - sc.ppx) / sc.f, ry = (((float)j + 0.5f) - sc.ppy) / sc.f;
        const float t = (tb[0] * rx + tb[1] * ry) + tb[2];
        if (t > 0.f) {
            const float zt = tb[3] / t;
            if (zt >= sc.zmin && zt <= sc.zmax && !(drawn && z <= zt)) {
                drawn = true;
                z = zt;
                label = 0;
            }
        }
    }
    uint16_t d = empty_depth;
    if (drawn) {
        const uint32_t h = mix32(mix32(seed + (uint32_t)n * 0x9e3779b9u) ^ p);
        if (hole_threshold != 0u && h < hole_threshold) {
            drawn = false;
            label = 0;
        } else {
            d = depth_u16(z);
            if (noise_amp > 0) {
                const uint32_t h2 = mix32(h ^ 0x85ebca6bu);
                const int moved = (int)d + (int)(h2 % (uint32_t)(2 * noise_amp + 1)) - noise_amp;
                d = (uint16_t)min(max(moved, 1), 65534);
            }
        }
    }
    depth_out[at] = d;
    labels_out[at] = label;
}

inline hipStream_t S(void *s) { return reinterpret_cast<hipStream_t>(s); }
inline bool misaligned(const void *p, unsigned a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; }
inline bool finite_f(float v) { return fabsf(v) <= 3.0e38f; }

}  // namespace

extern "C" {

size_t rdf_hand_scene_workspace_bytes(int n_frames, int dim_x, int dim_y)
{
    if (n_frames < 1 || dim_x < 0 || dim_y < 0 || dim_x > kMaxDim || dim_y > kMaxDim) return 0;
    return (size_t)n_frames * (size_t)dim_x * (size_t)dim_y * sizeof(u64);
}

int rdf_hand_scene_render(int n_frames, int dim_x, int dim_y, int n_verts, const float *verts, const int32_t *vert_part,
                          int n_tris, const int32_t *tris, const uint16_t *tri_label, int n_parts, const float *part_tforms,
                          const float *table, float f, float ppx, float ppy, float zmin, float zmax, uint16_t empty_depth,
                          uint32_t seed, uint32_t hole_threshold, int noise_amp, void *workspace, uint16_t *depth_out,
                          uint16_t *labels_out, void *stream)
{
    if (n_frames < 1 || dim_x < 0 || dim_y < 0 || n_verts < 0 || n_tris < 0 || n_parts < 0) return RDF_ERR_BAD_ARG;
    if (dim_x > kMaxDim || dim_y > kMaxDim) return RDF_ERR_TOO_LARGE;
    if (!(f > 0.f) || !finite_f(f) || !finite_f(ppx) || !finite_f(ppy) || !(zmin > 0.f) || !(zmax >= zmin) || !finite_f(zmax))
        return RDF_ERR_BAD_ARG;
    if (noise_amp < 0 || noise_amp > kMaxNoise) return RDF_ERR_BAD_ARG;
    const long long n_px = (long long)dim_x * dim_y;
    if (n_px == 0) return RDF_OK;
    if (!workspace || !depth_out || !labels_out) return RDF_ERR_NULL_PTR;
    if (n_tris > 0 && (!verts || !vert_part || !tris || !tri_label || !part_tforms)) return RDF_ERR_NULL_PTR;
    if (misaligned(workspace, 8) || misaligned(depth_out, 2) || misaligned(labels_out, 2) || depth_out == labels_out ||
        misaligned(verts, 4) || misaligned(vert_part, 4) || misaligned(tris, 4) || misaligned(tri_label, 2) ||
        misaligned(part_tforms, 4) || misaligned(table, 4))
        return RDF_ERR_BAD_ARG;
    const long long n_total = (long long)n_frames * n_px;
    const long long resolve_blocks = (n_total + kThreads - 1) / kThreads;
    if (resolve_blocks > 0x7fffffffll) return RDF_ERR_TOO_LARGE;
    Scene sc;
    sc.f = f, sc.ppx = ppx, sc.ppy = ppy, sc.zmin = zmin, sc.zmax = zmax;
    u64 *keys = static_cast<u64 *>(workspace);
    if (n_tris > 0) {
        const unsigned gy = (unsigned)n_frames < kMaxGridY ? (unsigned)n_frames : kMaxGridY;
        hipLaunchKernelGGL(k_hand_raster, dim3((unsigned)(((long long)n_tris * kLanesPerTri + kThreads - 1) / kThreads), gy), dim3(kThreads), 0, S(stream),
                           n_frames, dim_x, dim_y, n_verts, verts, vert_part, n_tris, tris, n_parts, part_tforms, sc, keys);
    }
    hipLaunchKernelGGL(k_hand_resolve, dim3((unsigned)resolve_blocks), dim3(kThreads), 0, S(stream), n_total, dim_x, dim_y, n_tris,
                       tri_label, table, sc, empty_depth, seed, hole_threshold, noise_amp, keys, depth_out, labels_out);
    return (int)hipGetLastError();
}

}  // extern "C"
