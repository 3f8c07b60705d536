// rdf_forest_ref.hpp -- the reference-layout forest, float32 [T][2^D - 1][7 + 2C] (what DecisionForest.forest_cu holds), as the
// forest tools of librdf_labels.so read it: the leaf refit, the pruning and the posterior (forest_refit_hip.hip,
// forest_prune_hip.hip, forest_posterior_hip.hip).  Four things, each written once: the shape and its addressing, the flag
// rule, rule R2's walk of one pixel down one tree, and the PDF of the nearest ancestor that holds enough pixels.  The rules
// are those of include/rdf_labels.h; tests/refit_numpy.py restates them (`walk`, which the other restatements import).
// The walks of librdf_hip.so are not this one: k_eval_forest reads packed tables, the trainer's has no scale.
#ifndef RDF_FOREST_REF_HPP
#define RDF_FOREST_REF_HPP

#include "rdf_device.hpp"
#include "rdf_kernel_util.hpp"

namespace {

// ---- 1. the shape ----
// A record is u.x u.y v.x v.y threshold flag[2] pdf[2][C]; the trees are in heap order.  The leaf refit's counts are
// uint64 [T][N][2][C], the subtree sums `sub` of the refit's apply and of the pruning uint64 [T][N][C].
constexpr int kMaxDepth = 30;

struct ForestShape {
    int T, D, C;
    __host__ __device__ int E() const { return 7 + 2 * C; }                      // floats per record
    __host__ __device__ size_t N() const { return ((size_t)1 << D) - 1; }        // nodes per tree
    __host__ __device__ size_t nodes() const { return (size_t)T * N(); }         // of the forest
    __host__ __device__ size_t at(size_t t, size_t n) const { return t * N() + n; }                      // node n of tree t
    __host__ __device__ size_t rec(size_t t, size_t n) const { return at(t, n) * E(); }                  // its record in the forest
    __host__ __device__ size_t cell(size_t t, size_t n, size_t s) const { return (at(t, n) * 2 + s) * C; }   // side s, class 0 in counts
    __host__ __device__ size_t row(size_t t, size_t n) const { return at(t, n) * C; }                    // class 0 in sub
};

inline bool bad_forest_shape(int T, int D, int C) { return T < 1 || D < 1 || D > kMaxDepth || C < 1 || C > 65535; }

// ---- 2. the flag rule ----
// A side of a record is a leaf slot when its flag does NOT floor to -1, with rule R2's floor (saturating, NaN -> 0: -1 and
// -0.5 say "go on", 0, -1.5 and NaN are leaf slots), at every level, D - 1 included.  So a child is reachable iff its parent
// is and the parent's flag towards it says "go on", and the root is.  Where a caller keeps what it knows of the parent is its
// own affair: parent_reached(at(t, parent)) answers.
__device__ __forceinline__ bool is_leaf_slot(const float *rec, uint32_t side) { return floor_i32(rec[5 + side]) != -1; }
template <typename Reached>
__device__ __forceinline__ bool is_reachable(const ForestShape &f, const float *forest, size_t t, size_t n, Reached parent_reached)
{
    if (n == 0) return true;
    const size_t parent = (n - 1) >> 1;
    return parent_reached(f.at(t, parent)) && !is_leaf_slot(forest + f.rec(t, parent), (uint32_t)(n - 1) & 1u);
}

// ---- 3. the walk ----
// Rule R2 for one pixel (x, y) of depth df in `frame` and one tree (`tree`: its root's record), one lane per pixel.  The level
// loop runs while any lane of the wave is still walking, so every lane of the wave calls this, a lane without a pixel with
// walking = false.  A walk ends in at_leaf(level, node, side, rec) at the first leaf slot, or in fell_off() when the flag
// says "go on" at level D - 1 and there is no level to go to.
struct WalkPixel { const uint16_t *__restrict__ frame; int W, H, x, y; float df, scale; };

template <typename AtLeaf, typename FellOff>
__device__ __forceinline__ void walk_tree(const float *__restrict__ tree, int D, int E, const WalkPixel &p, bool walking,
                                          AtLeaf at_leaf, FellOff fell_off)
{
    uint32_t g = 0u;                                                // the node's index in its level
    for (int j = 0; j < D && __ballot(walking) != 0ull; ++j) {
        if (!walking) continue;
        const uint32_t n = ((1u << j) - 1u) + g;
        const float *__restrict__ rec = tree + (size_t)n * E;
        const float s = p.scale;
        // `uv_scale * u.x / d_f`: one multiply and one IEEE divide, both rounded to nearest (no contraction, no
        // reciprocal: the library's flags); floor with saturation, NaN -> 0; a wrapping add
        const int ux = offset_coord(p.x, s * rec[0], p.df), uy = offset_coord(p.y, s * rec[1], p.df);
        const int vx = offset_coord(p.x, s * rec[2], p.df), vy = offset_coord(p.y, s * rec[3], p.df);
        const float f = depth_or_no_pixel<uint32_t>(p.frame, p.W, p.H, ux, uy) - depth_or_no_pixel<uint32_t>(p.frame, p.W, p.H, vx, vy);
        const uint32_t side = f < rec[4] ? 0u : 1u;                 // NaN goes right
        if (is_leaf_slot(rec, side)) {
            walking = false;
            at_leaf(j, n, side, rec);
        } else if (j == D - 1) {
            walking = false;
            fell_off();
        } else {
            g = g * 2u + side;
        }
    }
}

// ---- 4. the ancestor PDF ----
// The nearest of n (a node of level `level`), parent(n), ..., the root of tree t whose row of `sub` sums to at least `need`,
// and that sum; no row when not even the root's does.  (Levels counted, n == 0 not tested: the test cost the refit 0.6 %.)
struct SubRow { const u64 *row; u64 sum; };
__device__ __forceinline__ SubRow nearest_ancestor(const ForestShape &f, const u64 *sub, size_t t, size_t n, int level, u64 need)
{
    for (int lv = level; lv >= 0; --lv) {
        const u64 *cand = sub + f.row(t, n);
        u64 sum = 0ull;
        for (int c = 0; c < f.C; ++c) sum += cand[c];
        if (sum >= need) return {cand, sum};
        n = (n - 1) >> 1;                                           // (not followed at the root: lv ends the loop)
    }
    return {nullptr, 0ull};
}

// counts of a sum >= 1 to a PDF: uint64 -> fp32 (round to nearest even) on both sides of one IEEE divide
__device__ __forceinline__ void write_pdf(float *pdf, const u64 *counts, u64 sum, int C)
{
    const float den = (float)sum;
    for (int c = 0; c < C; ++c) pdf[c] = (float)counts[c] / den;
}

}  // namespace

#endif  // RDF_FOREST_REF_HPP
