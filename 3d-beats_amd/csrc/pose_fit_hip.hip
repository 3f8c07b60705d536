// pose_fit_hip.hip -- the hand of hand_model.py fitted to an observed depth frame and its labels on the device: the way back
// from what hand_scene_hip.hip draws.  The reference's pose_fit.py with cuda/fit_mesh.cu renders one candidate per GUI frame
// through OpenGL, reads a float cost summed by order-dependent atomics back to the host and keeps a random perturbation when
// the cost drops; here a generation is K candidates, five launches and no host read.  Built into librdf_labels.so; the rules
// (C, P, K, S) are in include/rdf_labels.h and restated in tests/pose_fit_numpy.py.
//
// k_pose_propose: six lanes per candidate.  Every lane derives the pose numbers it needs from the incumbent and the hash
// (rule P) -- nothing is exchanged -- and composes B = cam_from_plane T Rz Rx Ry; lane 0 writes the pose and the palm and
// zeroes the candidate's terms, lanes 1..5 walk one finger's chain each (rule K).  fp64 with a written-out operation order
// and a polynomial sine and cosine of its own, so that numpy restates it bit for bit; the library is built with
// -ffp-contract=off.  The config arrives by value in the kernel's arguments: nothing to upload, nothing to keep alive.
// k_pose_cost: rule C.  A candidate's depth and label images are each one contiguous run whatever the window is, so a lane
// takes eight pixels of each with one 16-byte load between the run's first and last 16-byte boundary (the boundary is
// found per candidate: K * ww * wh * 2 bytes need not be a multiple of 16); the up to seven pixels in front and behind
// are taken one per lane by the candidate's first workgroup.  The observed pixels under a group of eight are contiguous too
// unless the group crosses the window's right edge, but aligned to 2 bytes only: the compiler's loads of a 2-byte aligned
// copy, from a window that stays in cache while all K candidates read it.  Three 32-bit counters and a 64-bit sum of
// squares per lane, summed per wave by shuffles, per workgroup through LDS, then at most four 64-bit atomics.
// k_pose_select: one wave; rule S.
// The kinematics and the hash are __host__ __device__ so that a host program can run them against the restatement.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/rdf_labels.h"
#include "rdf_kernel_util.hpp"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxDim = 32768;
constexpr int kMaxChunk = 16;
constexpr int kTargetBlocks = 1024;     // four workgroups a compute unit
constexpr int kParts = 16;
constexpr int kLanesPerCandidate = 6;   // propose: the palm and five fingers
constexpr double kPi = 0x1.921fb54442d18p+1;

static_assert(sizeof(RdfPoseFitState) == 256, "RdfPoseFitState is 256 bytes");
static_assert(sizeof(RdfPoseFitConfig) == 1032, "RdfPoseFitConfig is 1032 bytes");

// ------------------------------------------------------------------ rules P and K ------------------------------------------
__host__ __device__ __forceinline__ double bits_to_double(u64 b)
{
    double d;
    __builtin_memcpy(&d, &b, 8);
    return d;
}

__host__ __device__ __forceinline__ void sincos_rule(double x, double *s, double *c)
{
    if (!(__builtin_fabs(x) <= 1048576.)) {
        *s = *c = bits_to_double(0x7ff8000000000000ull);
        return;
    }
    const double k = __builtin_rint(x * 0x1.45f306dc9c883p-1);
    const double r = (x - k * 0x1.921fb544p+0) - k * 0x1.0b4611a626331p-34;
    const double z = r * r;
    const double S = r + (r * z) * (-0x1.5555555555549p-3 + z * (0x1.111111110f8a6p-7 + z * (-0x1.a01a019c161d5p-13 + z * (0x1.71de357b1fe7dp-19 + z * (-0x1.ae5e68a2b9cebp-26 + z * 0x1.5d93a5acfd57cp-33)))));
    const double C = 1. + z * (-0.5 + z * (0x1.555555555554cp-5 + z * (-0x1.6c16c16c15177p-10 + z * (0x1.a01a019cb159p-16 + z * (-0x1.27e4f809c52adp-22 + z * (0x1.1ee9ebdb4b1c4p-29 + z * -0x1.8fae9be8838d4p-37))))));
    const int q = (int)k & 3;
    *s = q == 0 ? S : q == 1 ? C : q == 2 ? -S : -C;
    *c = q == 0 ? C : q == 1 ? -S : q == 2 ? -C : S;
}

struct Aff {
    double m[12];
};

__host__ __device__ __forceinline__ Aff mul(const Aff &a, const Aff &b)
{
    Aff c;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            double v = (a.m[4 * i] * b.m[j] + a.m[4 * i + 1] * b.m[4 + j]) + a.m[4 * i + 2] * b.m[8 + j];
            if (j == 3) v = v + a.m[4 * i + 3];
            c.m[4 * i + j] = v;
        }
    return c;
}

__host__ __device__ __forceinline__ Aff shift(double x, double y, double z)
{
    Aff a = {{1., 0., 0., x, 0., 1., 0., y, 0., 0., 1., z}};
    return a;
}

// axis 0, 1, 2 = x, y, z: the rotations of hand_model.py's _rot
__host__ __device__ __forceinline__ Aff rot(int axis, double angle)
{
    double s, c;
    sincos_rule(angle, &s, &c);
    Aff a = {{1., 0., 0., 0., 0., 1., 0., 0., 0., 0., 1., 0.}};
    const int i = axis == 0 ? 1 : axis == 1 ? 2 : 0, j = axis == 0 ? 2 : axis == 1 ? 0 : 1;
    a.m[4 * i + i] = c;
    a.m[4 * i + j] = -s;
    a.m[4 * j + i] = s;
    a.m[4 * j + j] = c;
    return a;
}

__host__ __device__ __forceinline__ bool in_group(uint32_t group, int j)
{
    if (group == 7u) return true;
    if (group == 0u) return j < 3;
    if (group == 1u) return j >= 3 && j < 6;
    const int first = 6 + 4 * ((int)group - 2);
    return j >= first && j < first + 4;
}

struct Proposal {           // of one candidate: what every pose number of it shares
    uint32_t h;
    bool perturbed;
    double scale;
};

__host__ __device__ __forceinline__ Proposal proposal(const RdfPoseFitConfig &cfg, uint32_t g, int k, bool fresh_first)
{
    Proposal p;
    p.h = mix32(mix32(cfg.seed + g * 0x9e3779b9u) ^ (uint32_t)k);
    p.perturbed = !(fresh_first && k == 0);
    uint32_t e = g / (uint32_t)cfg.anneal_every;
    e = e > 1022u ? 1022u : e;
    p.scale = bits_to_double((u64)(1023u - e) << 52);
    return p;
}

__host__ __device__ __forceinline__ double pose_number(const RdfPoseFitConfig &cfg, const double *__restrict__ inc,
                                                       const Proposal &p, int j)
{
    double v = inc[j];
    if (!p.perturbed || !in_group(p.h & 7u, j)) return v;
    const uint32_t a = mix32(p.h ^ ((2u * (uint32_t)j + 1u) * 0x85ebca6bu)), b = mix32(a ^ 0xc2b2ae35u);
    const double n = (double)((int)((a & 0xffffu) + (a >> 16) + (b & 0xffffu) + (b >> 16)) - 131070) / 65536.;
    v = v + (cfg.sigma[j] * p.scale) * n;
    v = v < cfg.lo[j] ? cfg.lo[j] : v;
    v = v > cfg.hi[j] ? cfg.hi[j] : v;
    return v;
}

__host__ __device__ __forceinline__ void store_tform(const Aff &a, float *__restrict__ out)
{
#pragma unroll
    for (int i = 0; i < 12; ++i) out[i] = (float)a.m[i];
}

// One of a candidate's six units: 0 writes the pose (and the palm), 1..5 a finger's three phalanges.
__host__ __device__ __forceinline__ void propose_unit(const RdfPoseFitConfig &cfg, const double *__restrict__ inc, uint32_t g,
                                                      bool fresh_first, int k, int unit, double *__restrict__ pose_out,
                                                      float *__restrict__ tforms_out)
{
    const Proposal p = proposal(cfg, g, k, fresh_first);
    Aff cam;
#pragma unroll
    for (int i = 0; i < 12; ++i) cam.m[i] = cfg.cam_from_plane[i];
    Aff hand = mul(shift(pose_number(cfg, inc, p, 0), pose_number(cfg, inc, p, 1), pose_number(cfg, inc, p, 2)),
                   rot(2, pose_number(cfg, inc, p, 3)));
    hand = mul(hand, rot(0, pose_number(cfg, inc, p, 4)));
    hand = mul(hand, rot(1, pose_number(cfg, inc, p, 5)));
    const Aff B = mul(cam, hand);
    if (unit == 0) {
        for (int j = 0; j < RDF_POSE_SIZE; ++j) pose_out[j] = pose_number(cfg, inc, p, j);
        store_tform(B, tforms_out);
        return;
    }
    const int f = unit - 1;
    const double *geo = cfg.geometry + 6 * f;
    Aff M = mul(shift(geo[0], geo[1], 0.), rot(2, geo[2] + pose_number(cfg, inc, p, 6 + 4 * f)));
    for (int q = 0; q < 3; ++q) {
        if (q) M = mul(M, shift(0., geo[3 + q - 1], 0.));
        M = mul(M, rot(0, -pose_number(cfg, inc, p, 7 + 4 * f + q)));
        Aff Mm = M;
        if (cfg.mirrored) {
            Mm.m[1] = -Mm.m[1];
            Mm.m[2] = -Mm.m[2];
            Mm.m[4] = -Mm.m[4];
            Mm.m[8] = -Mm.m[8];
            Mm.m[3] = -Mm.m[3];
        }
        store_tform(mul(B, Mm), tforms_out + (1 + 3 * f + q) * 12);
    }
}

__global__ void __launch_bounds__(64) k_pose_propose(RdfPoseFitConfig cfg, const RdfPoseFitState *__restrict__ state,
                                                     int fresh_first, double *__restrict__ poses,
                                                     float *__restrict__ part_tforms, u64 *__restrict__ terms)
{
    const int t = blockIdx.x * 64 + threadIdx.x;
    const int k = t / kLanesPerCandidate, unit = t - k * kLanesPerCandidate;
    if (k >= cfg.candidates) return;
    const uint32_t g = fresh_first ? 0u : state->generation;
    propose_unit(cfg, state->pose, g, fresh_first != 0, k, unit, poses + (size_t)k * RDF_POSE_SIZE,
                 part_tforms + (size_t)k * kParts * 12);
    if (unit == 0 && terms) {
#pragma unroll
        for (int i = 0; i < 4; ++i) terms[(size_t)k * 4 + i] = 0ull;
    }
}

// ------------------------------------------------------------------ rule C ------------------------------------------------
struct CostGeo {
    int W, Wl, Hl, r;           // the observed frame
    int x0, y0, ww;
    uint32_t n_px;              // ww * wh
    uint32_t chunk;             // sets of kThreads groups a workgroup takes
};

struct Sums {
    uint32_t missing, extra, label;
    u64 sq;
};

__device__ __forceinline__ void account(uint32_t d0, uint32_t l0, uint32_t d1, uint32_t l1, u64 mask, Sums &s)
{
    const bool hand = l0 < 64u && ((mask >> (l0 & 63u)) & 1ull) != 0ull;
    const bool seen = d0 != 0u, drawn = d1 != 0u;
    const bool both = seen && hand && drawn;
    s.missing += (uint32_t)(seen && hand && !drawn);
    s.extra += (uint32_t)(seen && !hand && drawn);
    s.label += (uint32_t)(both && l1 != l0);
    const uint32_t diff = d0 > d1 ? d0 - d1 : d1 - d0;          // <= 65535: the square fits 32 bits
    s.sq += both ? (u64)(diff * diff) : 0ull;
}

template <bool R1>
__device__ __forceinline__ uint32_t observed_label(const CostGeo &g, const uint16_t *__restrict__ labels, int x, int y)
{
    if (R1) return labels[(size_t)y * g.W + x];
    return labels[(size_t)min(y / g.r, g.Hl - 1) * g.Wl + min(x / g.r, g.Wl - 1)];
}

// Every index is inside its array: a window pixel idx < n_px gives (x, y) inside the window, the window is inside the frame
// (checked by the host), and a label position is clamped to [0, Wl) x [0, Hl).
template <bool R1>
__global__ void __launch_bounds__(kThreads) k_pose_cost(CostGeo g, const uint16_t *__restrict__ depth,
                                                        const uint16_t *__restrict__ labels,
                                                        const uint16_t *__restrict__ cand_depth,
                                                        const uint16_t *__restrict__ cand_labels, u64 mask,
                                                        u64 *__restrict__ terms)
{
    __shared__ u64 part[kWaves][4];
    const int tid = threadIdx.x;
    const uint32_t k = blockIdx.y, n_px = g.n_px, ww = (uint32_t)g.ww;
    const uint16_t *__restrict__ d1p = cand_depth + (size_t)k * n_px;
    const uint16_t *__restrict__ l1p = cand_labels + (size_t)k * n_px;
    uint32_t head = (uint32_t)(((16u - (unsigned)(reinterpret_cast<uintptr_t>(d1p) & 15u)) & 15u) / 2u);
    head = head > n_px ? n_px : head;
    const uint32_t n_groups = (n_px - head) / 8u, tail = n_px - head - 8u * n_groups;
    const bool labels_vec = (reinterpret_cast<uintptr_t>(l1p + head) & 15u) == 0u;       // uniform
    Sums s = {0u, 0u, 0u, 0ull};

    if (blockIdx.x == 0 && (uint32_t)tid < head + tail) {       // in front of and behind the full groups, one per lane
        const uint32_t idx = (uint32_t)tid < head ? (uint32_t)tid : head + 8u * n_groups + ((uint32_t)tid - head);
        const uint32_t j = idx / ww, i = idx - j * ww;
        const int x = g.x0 + (int)i, y = g.y0 + (int)j;
        account(depth[(size_t)y * g.W + x], observed_label<R1>(g, labels, x, y), d1p[idx], l1p[idx], mask, s);
    }

    const uint4 *__restrict__ d1v = reinterpret_cast<const uint4 *>(d1p + head);
    for (uint32_t trip = 0; trip < g.chunk; ++trip) {
        const uint32_t grp = (blockIdx.x * g.chunk + trip) * (uint32_t)kThreads + (uint32_t)tid;
        if (grp >= n_groups) break;         // rising with trip
        const uint4 dv = d1v[grp];
        uint4 lv;
        if (labels_vec)
            lv = reinterpret_cast<const uint4 *>(l1p + head)[grp];
        else
            __builtin_memcpy(&lv, l1p + head + 8 * (size_t)grp, 16);
        const uint32_t idx0 = head + 8u * grp;
        const uint32_t j0 = idx0 / ww, i0 = idx0 - j0 * ww;
        uint32_t d0[8], l0[8], d1[8], l1[8];
        unpack8(dv, d1);
        unpack8(lv, l1);
        if (i0 + 8u <= ww) {                // the eight observed pixels are one run of the frame's row
            const int x = g.x0 + (int)i0, y = g.y0 + (int)j0;
            uint4 ov;
            __builtin_memcpy(&ov, depth + (size_t)y * g.W + x, 16);
            unpack8(ov, d0);
            if (R1) {
                __builtin_memcpy(&ov, labels + (size_t)y * g.W + x, 16);
                unpack8(ov, l0);
            } else {
                const uint16_t *row = labels + (size_t)min(y / g.r, g.Hl - 1) * g.Wl;
#pragma unroll
                for (int e = 0; e < 8; ++e) l0[e] = row[min((x + e) / g.r, g.Wl - 1)];
            }
        } else {
            uint32_t i = i0, j = j0;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int x = g.x0 + (int)i, y = g.y0 + (int)j;
                d0[e] = depth[(size_t)y * g.W + x];
                l0[e] = observed_label<R1>(g, labels, x, y);
                if (++i == ww) {
                    i = 0u;
                    ++j;        // idx0 + e + 1 < n_px while another element follows: j stays inside the window
                }
            }
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) account(d0[e], l0[e], d1[e], l1[e], mask, s);
    }

    const uint32_t m = wave_sum(s.missing), x = wave_sum(s.extra), l = wave_sum(s.label);
    const u64 q = wave_sum64(s.sq);
    if ((tid & 63) == 0) {
        part[tid >> 6][0] = m;
        part[tid >> 6][1] = x;
        part[tid >> 6][2] = l;
        part[tid >> 6][3] = q;
    }
    __syncthreads();
    if (tid < 4) {
        u64 v = 0ull;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) v += part[w][tid];
        if (v) atomicAdd(terms + (size_t)k * 4 + tid, v);
    }
}

// ------------------------------------------------------------------ rule S ------------------------------------------------
__global__ void __launch_bounds__(64) k_pose_select(int K, const u64 *__restrict__ terms, const double *__restrict__ poses,
                                                    uint32_t w_boundary, uint32_t w_label, int fresh_first,
                                                    RdfPoseFitState *__restrict__ state, u64 *__restrict__ history_slot)
{
    const int lane = threadIdx.x;
    u64 best = ~0ull;
    int best_k = 0x7fffffff;            // a lane without candidates loses to any candidate, whatever its cost
    for (int k = lane; k < K; k += 64) {
        const u64 *t = terms + (size_t)k * 4;
        const u64 c = (u64)w_boundary * (t[0] + t[1]) + (u64)w_label * t[2] + t[3];
        if (c < best || best_k == 0x7fffffff) {     // k rises: of equal costs the first stays
            best = c;
            best_k = k;
        }
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const u64 oc = shfl_xor64(best, m);
        const int ok = __shfl_xor(best_k, m, 64);
        const bool mine_real = best_k != 0x7fffffff, other_real = ok != 0x7fffffff;
        if (other_real && (!mine_real || oc < best || (oc == best && ok < best_k))) {
            best = oc;
            best_k = ok;
        }
    }
    // (K >= 1: every lane now holds the same real candidate)
    const u64 old_cost = state->cost;
    const uint32_t g = state->generation, accepted = state->accepted;
    const bool replace = fresh_first != 0 || best < old_cost;
    __syncthreads();                    // one wave: every lane has read the state before any lane writes it
    if (replace) {
        if (lane < RDF_POSE_SIZE) state->pose[lane] = poses[(size_t)best_k * RDF_POSE_SIZE + lane];
        if (lane >= 32 && lane < 36) state->terms[lane - 32] = terms[(size_t)best_k * 4 + (lane - 32)];
        if (lane == 0) state->cost = best;
    }
    if (lane == 0) {
        state->generation = fresh_first ? 1u : g + 1u;
        state->accepted = fresh_first ? 1u : accepted + (replace ? 1u : 0u);
        if (history_slot) *history_slot = replace ? best : old_cost;
    }
}

// ------------------------------------------------------------------ host --------------------------------------------------
inline bool finite_d(double v) { return __builtin_fabs(v) <= 1.7e308; }
inline size_t up256(size_t n) { return (n + 255) & ~(size_t)255; }

struct Layout {
    size_t keys, cand_depth, cand_labels, tforms, poses, terms, total;
};

Layout layout(int K, int ww, int wh)
{
    Layout l;
    const size_t n = (size_t)K * (size_t)ww * (size_t)wh;
    l.keys = 0;
    l.cand_depth = up256(n * sizeof(u64));
    l.cand_labels = l.cand_depth + up256(n * 2);
    l.tforms = l.cand_labels + up256(n * 2);
    l.poses = l.tforms + up256((size_t)K * kParts * 12 * sizeof(float));
    l.terms = l.poses + up256((size_t)K * RDF_POSE_SIZE * sizeof(double));
    l.total = l.terms + up256((size_t)K * 4 * sizeof(u64));
    return l;
}

// what rule P and rule K ask of a config (not the window: that needs the frame)
int check_rules(const RdfPoseFitConfig &c)
{
    if (c.candidates < 1 || c.candidates > RDF_POSE_MAX_CANDIDATES || c.anneal_every < 1) return RDF_ERR_BAD_ARG;
    for (int j = 0; j < RDF_POSE_SIZE; ++j) {
        if (!finite_d(c.sigma[j]) || !finite_d(c.lo[j]) || !finite_d(c.hi[j])) return RDF_ERR_BAD_ARG;
        if (!(c.sigma[j] >= 0.) || !(c.lo[j] <= c.hi[j])) return RDF_ERR_BAD_ARG;
        if (j >= 3 && (c.lo[j] < -kPi || c.hi[j] > kPi)) return RDF_ERR_BAD_ARG;
    }
    for (int i = 0; i < 12; ++i)
        if (!finite_d(c.cam_from_plane[i])) return RDF_ERR_BAD_ARG;
    for (int i = 0; i < 30; ++i)
        if (!finite_d(c.geometry[i])) return RDF_ERR_BAD_ARG;
    return RDF_OK;
}

int check_window(int dim_x, int dim_y, int labels_reduce, int x0, int y0, int ww, int wh)
{
    if (dim_x < 0 || dim_y < 0 || labels_reduce < 1 || x0 < 0 || y0 < 0 || ww < 1 || wh < 1) return RDF_ERR_BAD_ARG;
    if ((long long)x0 + ww > dim_x || (long long)y0 + wh > dim_y) return RDF_ERR_BAD_ARG;
    if (dim_x / labels_reduce < 1 || dim_y / labels_reduce < 1) return RDF_ERR_BAD_ARG;
    return RDF_OK;
}

void launch_propose(const RdfPoseFitConfig &cfg, const RdfPoseFitState *state, int fresh_first, double *poses, float *tforms,
                    u64 *terms, hipStream_t stream)
{
    const unsigned blocks = (unsigned)((cfg.candidates * kLanesPerCandidate + 63) / 64);
    hipLaunchKernelGGL(k_pose_propose, dim3(blocks), dim3(64), 0, stream, cfg, state, fresh_first, poses, tforms, terms);
}

void launch_cost(int dim_x, int dim_y, const uint16_t *depth, const uint16_t *labels, int r, int x0, int y0, int ww, int wh,
                 int K, const uint16_t *cand_depth, const uint16_t *cand_labels, u64 mask, u64 *terms, hipStream_t stream)
{
    CostGeo g;
    g.W = dim_x, g.Wl = dim_x / r, g.Hl = dim_y / r, g.r = r;
    g.x0 = x0, g.y0 = y0, g.ww = ww;
    g.n_px = (uint32_t)ww * (uint32_t)wh;       // <= 2^30
    const uint32_t sets = (g.n_px / 8u + kThreads - 1) / kThreads;      // at least the sets of any candidate's groups
    uint32_t chunk = (uint32_t)(((u64)sets * (u64)K) / kTargetBlocks);
    chunk = chunk < 1u ? 1u : chunk > (uint32_t)kMaxChunk ? (uint32_t)kMaxChunk : chunk;
    g.chunk = chunk;
    const unsigned gx = sets ? (sets + chunk - 1) / chunk : 1u;
    if (r == 1)
        hipLaunchKernelGGL((k_pose_cost<true>), dim3(gx, (unsigned)K), dim3(kThreads), 0, stream, g, depth, labels, cand_depth,
                           cand_labels, mask, terms);
    else
        hipLaunchKernelGGL((k_pose_cost<false>), dim3(gx, (unsigned)K), dim3(kThreads), 0, stream, g, depth, labels, cand_depth,
                           cand_labels, mask, terms);
}

}  // namespace

extern "C" {

int rdf_pose_cost(int dim_x, int dim_y, const uint16_t *depth, const uint16_t *labels, int labels_reduce, int x0, int y0,
                  int ww, int wh, int candidates, const uint16_t *cand_depth, const uint16_t *cand_labels,
                  uint64_t target_mask, uint64_t *terms, void *stream)
{
    if (candidates < 1 || candidates > RDF_POSE_MAX_CANDIDATES) return RDF_ERR_BAD_ARG;
    const int rc = check_window(dim_x, dim_y, labels_reduce, x0, y0, ww, wh);
    if (rc) return rc;
    if (!depth || !labels || !cand_depth || !cand_labels || !terms) return RDF_ERR_NULL_PTR;
    if (dim_x > kMaxDim || dim_y > kMaxDim) return RDF_ERR_TOO_LARGE;
    if (misaligned(depth, 2) || misaligned(labels, 2) || misaligned(cand_depth, 2) || misaligned(cand_labels, 2) ||
        misaligned(terms, 8))
        return RDF_ERR_BAD_ARG;
    launch_cost(dim_x, dim_y, depth, labels, labels_reduce, x0, y0, ww, wh, candidates, cand_depth, cand_labels,
                (u64)target_mask, reinterpret_cast<u64 *>(terms), S(stream));
    return (int)hipGetLastError();
}

int rdf_pose_propose(const RdfPoseFitConfig *config_host, const RdfPoseFitState *state, int fresh_first, double *poses,
                     float *part_tforms, uint64_t *terms, void *stream)
{
    if (!config_host) return RDF_ERR_NULL_PTR;
    const int rc = check_rules(*config_host);
    if (rc) return rc;
    if (!state || !poses || !part_tforms) return RDF_ERR_NULL_PTR;
    if (misaligned(state, 8) || misaligned(poses, 8) || misaligned(part_tforms, 4) || misaligned(terms, 8)) return RDF_ERR_BAD_ARG;
    launch_propose(*config_host, state, fresh_first != 0, poses, part_tforms, reinterpret_cast<u64 *>(terms), S(stream));
    return (int)hipGetLastError();
}

int rdf_pose_select(int candidates, const uint64_t *terms, const double *poses, uint32_t w_boundary, uint32_t w_label,
                    int fresh_first, RdfPoseFitState *state, uint64_t *history_slot, void *stream)
{
    if (candidates < 1 || candidates > RDF_POSE_MAX_CANDIDATES) return RDF_ERR_BAD_ARG;
    if (!terms || !poses || !state) return RDF_ERR_NULL_PTR;
    if (misaligned(terms, 8) || misaligned(poses, 8) || misaligned(state, 8) || misaligned(history_slot, 8)) return RDF_ERR_BAD_ARG;
    hipLaunchKernelGGL(k_pose_select, dim3(1), dim3(64), 0, S(stream), candidates, reinterpret_cast<const u64 *>(terms), poses,
                       w_boundary, w_label, fresh_first != 0, state, reinterpret_cast<u64 *>(history_slot));
    return (int)hipGetLastError();
}

size_t rdf_pose_fit_workspace_bytes(int candidates, int ww, int wh)
{
    if (candidates < 1 || candidates > RDF_POSE_MAX_CANDIDATES || ww < 1 || wh < 1 || ww > kMaxDim || wh > kMaxDim) return 0;
    return layout(candidates, ww, wh).total;
}

int rdf_pose_fit(int generations, int fresh, const RdfPoseFitConfig *config_host, RdfPoseFitState *state, int dim_x,
                 int dim_y, const uint16_t *depth, const uint16_t *labels, int labels_reduce, int n_verts,
                 const float *verts, const int32_t *vert_part, int n_tris, const int32_t *tris, const uint16_t *tri_label,
                 void *workspace, uint64_t *history, void *stream)
{
    if (!config_host) return RDF_ERR_NULL_PTR;
    const RdfPoseFitConfig &c = *config_host;
    if (generations < 0 || n_verts < 0 || n_tris < 0) return RDF_ERR_BAD_ARG;
    int rc = check_rules(c);
    if (rc) return rc;
    rc = check_window(dim_x, dim_y, labels_reduce, c.x0, c.y0, c.ww, c.wh);
    if (rc) return rc;
    // what rdf_hand_scene_render will ask of its arguments, asked before anything is launched
    const float ppx = c.ppx - (float)c.x0, ppy = c.ppy - (float)c.y0;
    if (!(c.f > 0.f) || !finite_f(c.f) || !finite_f(ppx) || !finite_f(ppy) || !(c.zmin > 0.f) || !(c.zmax >= c.zmin) ||
        !finite_f(c.zmax))
        return RDF_ERR_BAD_ARG;
    if (generations == 0) return RDF_OK;
    if (!state || !depth || !labels || !workspace) return RDF_ERR_NULL_PTR;
    if (n_tris > 0 && (!verts || !vert_part || !tris || !tri_label)) return RDF_ERR_NULL_PTR;
    if (dim_x > kMaxDim || dim_y > kMaxDim) return RDF_ERR_TOO_LARGE;
    if (((long long)c.candidates * c.ww * c.wh + 255) / 256 > 0x7fffffffll) return RDF_ERR_TOO_LARGE;      // the renderer's limit
    if (misaligned(state, 8) || misaligned(depth, 2) || misaligned(labels, 2) || misaligned(workspace, 16) ||
        misaligned(history, 8) || misaligned(verts, 4) || misaligned(vert_part, 4) || misaligned(tris, 4) ||
        misaligned(tri_label, 2))
        return RDF_ERR_BAD_ARG;

    const int K = c.candidates;
    const Layout l = layout(K, c.ww, c.wh);
    char *ws = static_cast<char *>(workspace);
    uint16_t *cand_depth = reinterpret_cast<uint16_t *>(ws + l.cand_depth);
    uint16_t *cand_labels = reinterpret_cast<uint16_t *>(ws + l.cand_labels);
    float *tforms = reinterpret_cast<float *>(ws + l.tforms);
    double *poses = reinterpret_cast<double *>(ws + l.poses);
    u64 *terms = reinterpret_cast<u64 *>(ws + l.terms);
    for (int i = 0; i < generations; ++i) {
        const int fresh_first = fresh != 0 && i == 0;
        launch_propose(c, state, fresh_first, poses, tforms, terms, S(stream));
        rc = rdf_hand_scene_render(K, c.ww, c.wh, n_verts, verts, vert_part, n_tris, tris, tri_label, kParts, tforms, nullptr,
                                   c.f, ppx, ppy, c.zmin, c.zmax, 0, 0u, 0u, 0, ws + l.keys, cand_depth, cand_labels, stream);
        if (rc) return rc;
        launch_cost(dim_x, dim_y, depth, labels, labels_reduce, c.x0, c.y0, c.ww, c.wh, K, cand_depth, cand_labels,
                    (u64)c.target_mask, terms, S(stream));
        hipLaunchKernelGGL(k_pose_select, dim3(1), dim3(64), 0, S(stream), K, terms, poses, c.w_boundary, c.w_label, fresh_first,
                           state, history ? reinterpret_cast<u64 *>(history) + i : nullptr);
    }
    return (int)hipGetLastError();
}

}  // extern "C"
