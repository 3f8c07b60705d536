// rdf_raster.hpp -- the software rasteriser of librdf_labels.so, once: the vertex transform and rules 3 to 6 of rdf_rerender
// in include/rdf_labels.h (projection and snapping, coverage with the top-left fill rule, perspective-correct depth, the
// depth test's key), which rdf_hand_scene_render adopts unchanged.  rerender_hip.hip and hand_scene_hip.hip both draw with
// these functions, so the two entry points cannot drift apart; what differs between them (where vertices come from, colours
// against labels, how lanes share the pixels) stays in those files.  The images are bit-exact contracts: every fp32
// expression below is in the header's order and the library is built with -ffp-contract=off.
#ifndef RDF_RASTER_HPP
#define RDF_RASTER_HPP

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rdf_kernel_util.hpp"

namespace {

constexpr u64 kEmptyKey = ~0ull;
constexpr int kSubPixel = 256, kHalfPixel = 128;        // 8 sub-pixel bits
constexpr float kMaxSnapped = 1048576.f;                // 2^20
constexpr int kMaxDim = 32768;                          // per axis: keeps 256 * dim in an int, and a frame's pixels below 2^31

struct Pinhole {
    float f, ppx, ppy, zmin, zmax;
};

// what both entry points require of the camera: f > 0, 0 < zmin <= zmax, everything finite
inline bool pinhole_ok(const Pinhole &c)
{
    return c.f > 0.f && finite_f(c.f) && finite_f(c.ppx) && finite_f(c.ppy) && c.zmin > 0.f && c.zmax >= c.zmin && finite_f(c.zmax);
}

struct Snapped {
    int X, Y;                       // snapped screen position, 1/256 pixel
    float z;                        // z'
    bool drawable;                  // z' > 0 and |X|, |Y| <= 2^20
};

// rules 2 and 3: the point (x, y, z) moved by the affine m (three rows of four), projected and snapped
__device__ __forceinline__ Snapped project_point(const float *m, float px, float py, float pz, const Pinhole &cam)
{
    const float x = ((m[0] * px + m[1] * py) + m[2] * pz) + m[3];
    const float y = ((m[4] * px + m[5] * py) + m[6] * pz) + m[7];
    const float z = ((m[8] * px + m[9] * py) + m[10] * pz) + m[11];
    Snapped v;
    v.X = v.Y = 0;
    v.z = z;
    v.drawable = false;
    if (z > 0.f) {
        const float fx = floorf(((cam.f * x) / z + cam.ppx) * (float)kSubPixel + 0.5f);
        const float fy = floorf(((cam.f * y) / z + cam.ppy) * (float)kSubPixel + 0.5f);
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

struct Tri {
    int X[3], Y[3];
    float z[3];
    int sgn;                        // the sign of the area
    int need[3];                    // e_k >= need[k]: 0 on a top or left edge, else 1
};

// rule 4, the part that does not depend on the pixel, of three vertices (anything with X, Y and z); `drawable`: all three
// are (rules 2 and 3).  False: the triangle is dropped.  The drawable test sits here, in front of the copies, and not in
// the callers: tested in front of the call, k_hand_raster comes out with 75 VGPRs for 82 and another schedule, and the pose
// fit's render of 64 candidate windows measured 112 us against 109.5 ("One rasteriser, one set of kernel helpers").
template <typename V>
__device__ __forceinline__ bool setup_triangle(const V &a, const V &b, const V &c, bool drawable, Tri &t)
{
    if (!drawable) return false;
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

// rules 4 and 5 at pixel (i, j).  False: not covered, or discarded by the depth range.  A caller that interpolates nothing
// but z ignores q and s.
__device__ __forceinline__ bool fragment(const Tri &t, int i, int j, const Pinhole &cam, float *z, float q[3], float *s)
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
#pragma unroll
    for (int k = 0; k < 3; ++k) q[k] = w[k] / t.z[k];
    *s = (q[0] + q[1]) + q[2];
    *z = ((w[0] + w[1]) + w[2]) / *s;
    return *z >= cam.zmin && *z <= cam.zmax;
}

__device__ __forceinline__ int imin3(const int v[3]) { return min(v[0], min(v[1], v[2])); }
__device__ __forceinline__ int imax3(const int v[3]) { return max(v[0], max(v[1], v[2])); }

// the pixels whose centre 256 i + 128 lies within the triangle's [min, max] (>> floors, also below zero), clipped to the
// frame: i0 <= i <= i1, j0 <= j <= j1, possibly none
struct PixelBox {
    int i0, i1, j0, j1;
};

__device__ __forceinline__ PixelBox clipped_box(const Tri &t, int W, int H)
{
    PixelBox b;
    b.i0 = max(0, (imin3(t.X) - kHalfPixel + kSubPixel - 1) >> 8);
    b.i1 = min(W - 1, (imax3(t.X) - kHalfPixel) >> 8);
    b.j0 = max(0, (imin3(t.Y) - kHalfPixel + kSubPixel - 1) >> 8);
    b.j1 = min(H - 1, (imax3(t.Y) - kHalfPixel) >> 8);
    return b;
}

// rule 6: z > 0, so its bit pattern orders as its value; ties go to the lowest id
__device__ __forceinline__ u64 depth_key(float z, uint32_t id) { return ((u64)__float_as_uint(z) << 32) | id; }
__device__ __forceinline__ float key_z(u64 key) { return __uint_as_float((uint32_t)(key >> 32)); }
__device__ __forceinline__ uint32_t key_id(u64 key) { return (uint32_t)key; }

// rule 5's stored depth: z truncated to uint16, 65535 at most
__device__ __forceinline__ uint16_t depth_u16(float z) { return z >= 65535.f ? (uint16_t)65535 : (uint16_t)(uint32_t)z; }

}  // namespace

#endif  // RDF_RASTER_HPP
