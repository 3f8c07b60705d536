// hand_scene_hip.hip -- labelled depth frames of an articulated triangle mesh (the hand of hand_model.py) over an analytic
// table plane, many frames per call: the package's own source of training sets and of raw camera sequences, in place of the
// Blender scenes of the reference's datagen/.  Built into librdf_labels.so; the rules are in include/rdf_labels.h under
// rdf_hand_scene_render and restated in tests/hand_scene_numpy.py.  Projection, snapping, coverage, fill rule, depth and
// depth test are rules 3 to 6 of rdf_rerender and come from rdf_raster.hpp, the same functions rerender_hip.hip draws with;
// this file has the vertex rule's index checks, the way lanes share a triangle, and rules T, E and H.
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
#include "rdf_kernel_util.hpp"
#include "rdf_raster.hpp"

namespace {

constexpr int kThreads = 256;
constexpr int kLanesPerTri = 8;                         // raster: lanes that share a triangle's rows
constexpr int kMaxNoise = 32767;
constexpr unsigned kMaxGridY = 65535u;

// Every index read from the mesh is checked before it is followed: a triangle with a vertex outside [0, n_verts) or a
// vertex whose part is outside [0, n_parts) is dropped.  Pixel addresses come from the clipped bounding box alone.
__global__ void __launch_bounds__(kThreads) k_hand_raster(int n_frames, int W, int H, int n_verts,
                                                          const float *__restrict__ verts,
                                                          const int32_t *__restrict__ vert_part, int n_tris,
                                                          const int32_t *__restrict__ tris, int n_parts,
                                                          const float *__restrict__ part_tforms, Pinhole cam,
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
        Snapped v[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {       // rule V, then rule 3
            const float *p = verts + (long long)vi[k] * 3;
            v[k] = project_point(m + (long long)part[k] * 12, p[0], p[1], p[2], cam);
        }
        Tri tr;
        if (!setup_triangle(v[0], v[1], v[2], v[0].drawable && v[1].drawable && v[2].drawable, tr)) continue;
        const PixelBox box = clipped_box(tr, W, H);
        u64 *plane = keys + (long long)n * n_px;
        for (int j = box.j0 + sub; j <= box.j1; j += kLanesPerTri)
            for (int i = box.i0; i <= box.i1; ++i) {
                float z, q[3], s;
                if (!fragment(tr, i, j, cam, &z, q, &s)) continue;
                atomicMin(&plane[(long long)j * W + i], depth_key(z, (uint32_t)t));     // rule 6
            }
    }
}

// A key that no call of k_hand_raster can have left (a workspace that was not filled with 0xFF) names no triangle of this
// mesh: it is treated as empty rather than followed out of tri_label.
__global__ void __launch_bounds__(kThreads) k_hand_resolve(long long n_total, int W, int H, int n_tris,
                                                           const uint16_t *__restrict__ tri_label,
                                                           const float *__restrict__ table, Pinhole cam, uint16_t empty_depth,
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
        const uint32_t id = key_id(key);
        if (id < (uint32_t)n_tris) {
            drawn = true;
            z = key_z(key);
            label = tri_label[id];
        }
    }
    if (table) {
        const float *tb = table + n * 4;
        const float rx = (((float)i + 0.5f) - cam.ppx) / cam.f, ry = (((float)j + 0.5f) - cam.ppy) / cam.f;
        const float t = (tb[0] * rx + tb[1] * ry) + tb[2];
        if (t > 0.f) {
            const float zt = tb[3] / t;
            if (zt >= cam.zmin && zt <= cam.zmax && !(drawn && z <= zt)) {
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
    const Pinhole cam = {f, ppx, ppy, zmin, zmax};
    if (!pinhole_ok(cam)) return RDF_ERR_BAD_ARG;
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
    u64 *keys = static_cast<u64 *>(workspace);
    if (n_tris > 0) {
        const unsigned gy = (unsigned)n_frames < kMaxGridY ? (unsigned)n_frames : kMaxGridY;
        hipLaunchKernelGGL(k_hand_raster, dim3(blocks((long long)n_tris * kLanesPerTri, kThreads), gy), dim3(kThreads), 0,
                           S(stream), n_frames, dim_x, dim_y, n_verts, verts, vert_part, n_tris, tris, n_parts, part_tforms, cam,
                           keys);
    }
    hipLaunchKernelGGL(k_hand_resolve, dim3((unsigned)resolve_blocks), dim3(kThreads), 0, S(stream), n_total, dim_x, dim_y, n_tris,
                       tri_label, table, cam, empty_depth, seed, hole_threshold, noise_amp, keys, depth_out, labels_out);
    return (int)hipGetLastError();
}

}  // extern "C"
