// vote_tips_hip.hip -- voted fingertips: where the label route (mean shift or soft modes, then the height of the mode) and the
// joint votes (forest_votes_hip.hip) meet.  rdf_labels_vote_tips runs behind the mode launch of a hand's chain: per frame and
// fingertip it takes the mode of the tip's class and the voted position of the tip's joint, chooses between them by a policy,
// finds a depth for the chosen pixel and writes the height above the calibrated plane where the mode launch wrote it -- so a
// tip whose class has no pixel in the frame gets a height from its vote.  Built into librdf_labels.so.  The contract (rules T)
// is in include/rdf_labels.h and tests/vote_tips_numpy.py restates it.
//
// k_vote_tips: one lane per (frame, tip), 256-thread workgroups, at most kMaxBlocks of them striding over the pairs.  A lane
// reads two doubles, one 16-byte joint, one or two depth pixels and the plane's third row; no LDS, no atomics.  The bounds
// test of a mode and the deprojection are those of rdf_modes.hpp (mode_pixel, height_at_pixel), so a tip that keeps its mode
// keeps the height the mode launch gave it, bit for bit.

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/rdf_labels.h"
#include "rdf_modes.hpp"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxBlocks = 4;         // 1024 lanes: more (frame, tip) pairs than this stride over the grid

struct VoteTipsArgs {
    const double *means;              // [n_img][L][2]
    const int4 *joints;               // [n_img][J]
    const int *tip_joints;            // [n_ids]
    int4 *tips;                       // [n_img][n_ids] or null
    uint32_t n_pairs;                 // n_img * n_ids (< 2^31)
    int L, J, flip_x, policy, max_dist, z_tol;
    HeightArgs h;                     // class_ids, n_ids, depth of frame 0, the frame's size, the camera, heights of frame 0
};

__device__ __forceinline__ long long clampll(long long v, long long lo, long long hi) { return v < lo ? lo : (v > hi ? hi : v); }
__device__ __forceinline__ long long absll(long long v) { return v < 0 ? -v : v; }

__global__ void __launch_bounds__(kThreads) k_vote_tips(const VoteTipsArgs a)
{
    const uint32_t n_ids = (uint32_t)a.h.n_ids;
    for (uint32_t pair = blockIdx.x * (uint32_t)kThreads + threadIdx.x; pair < a.n_pairs; pair += gridDim.x * (uint32_t)kThreads) {
        const uint32_t f = pair / n_ids, i = pair - f * n_ids;
        const uint16_t *depth = a.h.depth + (size_t)f * (size_t)a.h.dim_x * (size_t)a.h.dim_y;

        // T1: the mode candidate
        long long pxm = 0, pym = 0;
        bool has_m = false;
        const int c = a.h.class_ids[i];
        if (c >= 1 && c <= a.L) {
            const double *m = a.means + ((size_t)f * (size_t)a.L + (size_t)(c - 1)) * 2;
            has_m = mode_pixel(m[0], m[1], a.h, &pxm, &pym);
        }

        // T2: the vote candidate
        long long pxv = 0, pyv = 0;
        int Z = 0;
        bool has_v = false;
        const int j = a.tip_joints[i];
        if (j >= 0 && j < a.J && a.h.dim_x > 0 && a.h.dim_y > 0) {
            const int4 v = a.joints[(size_t)f * (size_t)a.J + (size_t)j];
            if (v.w > 0) {
                const long long Xu = a.flip_x ? 16ll * a.h.dim_x - (long long)v.x : (long long)v.x;
                pxv = clampll(Xu >> 4, 0, a.h.dim_x - 1);          // (an arithmetic shift is the floor division by 16)
                pyv = clampll((long long)v.y >> 4, 0, a.h.dim_y - 1);
                Z = v.z;
                has_v = true;
            }
        }

        // T3: the choice
        bool use_m = has_m;
        if (has_m && has_v) {
            if (a.policy == RDF_TIPS_GUARD) {
                const long long dx = absll(pxm - pxv), dy = absll(pym - pyv);
                use_m = (dx > dy ? dx : dy) <= (long long)a.max_dist;
            } else if (a.policy == RDF_TIPS_VOTES) {
                use_m = false;
            }
        }

        // T4, T5: the depth and the height
        double height = nan("");
        int4 tip = make_int4(-1, -1, 0, 0);
        if (use_m) {
            const int z = (int)depth[pym * a.h.dim_x + pxm];
            height = height_at_pixel(pxm, pym, (float)z, a.h);
            tip = make_int4((int)pxm, (int)pym, z, 1);
        } else if (has_v) {
            const int zs = (int)depth[pyv * a.h.dim_x + pxv];
            const bool seen = zs != 0 && zs != 65535 && absll((long long)zs - (long long)Z) <= (long long)a.z_tol;
            const int z = seen ? zs : Z;
            height = height_at_pixel(pxv, pyv, (float)z, a.h);
            tip = make_int4((int)pxv, (int)pyv, z, seen ? 2 : 3);
        }
        a.h.heights[(size_t)f * (size_t)a.h.heights_stride + i] = height;
        if (a.tips) a.tips[pair] = tip;
    }
}

}  // namespace

extern "C" {

int rdf_labels_vote_tips(const double *means, int n_img, int num_classes, const int *class_ids, const int *tip_joints,
                         int n_ids, const int32_t *joints, int n_joints, int flip_x, const uint16_t *depth, int dim_x,
                         int dim_y, int labels_reduce, float fx, float fy, float ppx, float ppy, const float *plane,
                         int policy, int max_dist, int z_tol, double *heights_out, int heights_stride,
                         int32_t *tips_out, void *stream)
{
    if (n_img < 0 || num_classes < 1 || n_ids < 1 || n_joints < 1 || n_joints > RDF_VOTES_MAX_JOINTS || dim_x < 0 || dim_y < 0 ||
        dim_x > 65535 || dim_y > 65535 || labels_reduce < 1 || policy < RDF_TIPS_FILL || policy > RDF_TIPS_VOTES || max_dist < 0 ||
        max_dist > 65535 || z_tol < 0 || z_tol > 65535 || heights_stride < n_ids)
        return RDF_ERR_BAD_ARG;
    if (misaligned(means, 8) || misaligned(class_ids, 4) || misaligned(tip_joints, 4) || misaligned(joints, 16) ||
        misaligned(depth, 2) || misaligned(plane, 4) || misaligned(heights_out, 8) || misaligned(tips_out, 16))
        return RDF_ERR_BAD_ARG;
    if ((long long)n_img * n_ids >= (1ll << 31) || (long long)n_img * dim_x * dim_y >= (1ll << 31)) return RDF_ERR_TOO_LARGE;
    if (n_img == 0) return RDF_OK;
    if (!means || !class_ids || !tip_joints || !joints || !depth || !plane || !heights_out) return RDF_ERR_NULL_PTR;

    VoteTipsArgs a;
    a.means = means;
    a.joints = reinterpret_cast<const int4 *>(joints);
    a.tip_joints = tip_joints;
    a.tips = reinterpret_cast<int4 *>(tips_out);
    a.n_pairs = (uint32_t)n_img * (uint32_t)n_ids;
    a.L = num_classes;
    a.J = n_joints;
    a.flip_x = flip_x ? 1 : 0;
    a.policy = policy;
    a.max_dist = max_dist;
    a.z_tol = z_tol;
    a.h = HeightArgs{class_ids, n_ids, depth, dim_x, dim_y, labels_reduce, fx, fy, ppx, ppy, plane, heights_out, heights_stride};
    unsigned grid = blocks(a.n_pairs, kThreads);
    grid = grid > (unsigned)kMaxBlocks ? (unsigned)kMaxBlocks : grid;
    hipLaunchKernelGGL(k_vote_tips, dim3(grid), dim3(kThreads), 0, S(stream), a);
    return (int)hipGetLastError();
}

}  // extern "C"
