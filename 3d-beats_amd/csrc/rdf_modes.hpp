// rdf_modes.hpp -- the one mode-finding kernel body behind k_mean_shift_fused (mean_shift_hip.hip, librdf_hip.so) and
// k_weighted_modes (soft_modes_hip.hip, librdf_labels.so): per-class 2-D mean shift over a label map, every pixel pulling
// equally or with an integer weight, and the fingertip heights of the modes.
//
// Reference: src/cuda/mean_shift.cu:3-48 (one pass over the label image per round, fp64 atomicAdd into a [classes][3] array)
// driven by the host loop of src/cuda/mean_shift.py:35-59, which per round zero-fills the sums, launches, copies sums and
// means to the host, divides, adds and copies the means back (12 transfers for 6 rounds); heights: src/3d_bz.py:503-522 on
// the host.
//
// Here all rounds of one class run in ONE workgroup and all classes (and frames) in one launch: classes never interact
// (mean_shift.cu:3-48 sums per class), so no round needs anything from another workgroup.  The workgroup lists its class's
// pixels once, in pixel order, in LDS and then iterates over the list: round 0 = centroid (:32-35), rounds >= 1 =
// kernel-weighted shift (:36-47), means += sums[:2] / sums[2] after each (mean_shift.py:54-57).  Every sum is taken in a
// fixed order (thread-strided partial sums, a DPP row scan, rows and waves in index order): no atomics, so the result is the
// same bits from run to run (the reference's fp64 atomics make its last bits run-dependent) and from any pointer alignment.
// An earlier version ran one launch per round over 64 workgroups with a cross-workgroup partial-sum hand-off at every
// kernel boundary: 7 launches, 74 us for the app's 424x240 label map (profiles/r02_pipeline_kernel_stats_before.csv).
//
// The two kernels are two policies of modes_body; what differs between them is an `if constexpr (P::kWeighted)` there.
#ifndef RDF_MODES_HPP
#define RDF_MODES_HPP

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "rdf_kernel_util.hpp"

namespace {

constexpr int kModesThreads = 1024;
constexpr int kModesWaves = kModesThreads / 64;
constexpr int kModesMaxClasses = 64;
constexpr uint32_t kTabCap = 3072;       // dim_x + dim_y the per-round weight tables cover (24 576 B)
constexpr int kSteps = 13;               // 16 waves x 13 steps x 512 pixels = 106 496 >= the app's 424 x 240 label map in one batch

// kListCap: pixels of one class kept in LDS; a class with more is not listed, its rounds rescan the maps.
struct Unweighted { static constexpr bool kWeighted = false; static constexpr uint32_t kListCap = 32768; };   // 131 072 B
// A weighted entry carries a 16-bit weight behind the list; pixels of weight 0 do not count: they take no slot and no part
// in any sum.  A null `weights` is weight 1 everywhere, on this policy's cap.
struct Weighted { static constexpr bool kWeighted = true; static constexpr uint32_t kListCap = 20480; };      // 122 880 B

// the dynamic LDS of a launch: with the 25 408 B of tables and sums below, 156 480 B / 148 288 B of the CU's 160 KB
template <class P>
constexpr int modes_lds_bytes() { return (int)(P::kListCap * (4u + (P::kWeighted ? 2u : 0u))); }

// One step of a row-wise (16 lanes) sum: v += the value `shr` lanes to the left in the same row (0.0 where there is none).
// DPP moves of the two halves: a VALU-speed lane exchange (ds_bpermute, which __shfl_down compiles to, is an LDS round trip).
template <int SHR>
__device__ __forceinline__ double row_add_shr(double v)
{
    const int lo = __double2loint(v), hi = __double2hiint(v);
    const int plo = __builtin_amdgcn_update_dpp(0, lo, 0x110 + SHR, 0xF, 0xF, true);   // row_shr:SHR, bound_ctrl: 0 outside
    const int phi = __builtin_amdgcn_update_dpp(0, hi, 0x110 + SHR, 0xF, 0xF, true);
    return v + __hiloint2double(phi, plo);
}

// Sum over the wave in a fixed order: a shift-add scan inside each row of 16 lanes (lane 15, 31, 47, 63 then hold their
// row's total), the four row totals added in order.  Every lane returns the same value.
__device__ __forceinline__ double wave_sum_f64(double v)
{
    v = row_add_shr<1>(v); v = row_add_shr<2>(v); v = row_add_shr<4>(v); v = row_add_shr<8>(v);
    double r[4];
#pragma unroll
    for (int q = 0; q < 4; ++q)
        r[q] = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), 16 * q + 15),
                                __builtin_amdgcn_readlane(__double2loint(v), 16 * q + 15));
    return ((r[0] + r[1]) + r[2]) + r[3];
}

// Sum of every thread's (a, b, c) in a fixed order: inside a wave as above, then the waves one after the other.
// Every thread returns with the totals in tot[0..2].  s_red is double-buffered by the caller's round parity, so one
// barrier per call is enough: a buffer is rewritten two calls later, after every thread has passed the barrier between.
__device__ __forceinline__ void block_sum3(double a, double b, double c, double (*s_red)[3], double *tot)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    a = wave_sum_f64(a); b = wave_sum_f64(b); c = wave_sum_f64(c);
    if (lane == 0) { s_red[wave][0] = a; s_red[wave][1] = b; s_red[wave][2] = c; }
    __syncthreads();
    double ta = 0.0, tb = 0.0, tc = 0.0;
    for (int w = 0; w < kModesWaves; ++w) { ta += s_red[w][0]; tb += s_red[w][1]; tc += s_red[w][2]; }   // broadcast reads
    tot[0] = ta; tot[1] = tb; tot[2] = tc;
}

struct HeightArgs {
    const int *class_ids;      // 1-based labels (device); n_ids of them
    int n_ids;
    const uint16_t *depth;     // the ORIGINAL depth frame (3d_bz.py:515)
    int dim_x, dim_y, labels_reduce;
    float fx, fy, ppx, ppy;
    const float *plane;        // 4x4 row-major (device)
    double *heights;           // [n_ids]
    int heights_stride;        // doubles between two frames' heights (unused for one frame)
};

// Height of a mode above the calibrated plane (3d_bz.py:503-522; rule S7 of include/rdf_labels.h):
//   px,py = int(mean) * labels_reduce; off-frame -> NaN ("reset"); z = depth[py][px];
//   pt = z * ((px-ppx)/fx, (py-ppy)/fy, 1)  (librealsense rs2_deproject_pixel_to_point, no distortion, fp32);
//   height = -(plane @ [pt,1]).z  with the fp32 plane matrix promoted to fp64 like numpy's float32 @ float64.
// The two halves below are also what k_vote_tips (vote_tips_hip.hip, rules T1 and T5) is made of: one bounds test and one
// deprojection in the package.
__device__ __forceinline__ bool mode_pixel(double mx, double my, const HeightArgs &h, long long *px, long long *py)
{
    if (!(mx == mx && my == my && fabs(mx) < 1e9 && fabs(my) < 1e9)) return false;
    *px = (long long)mx * h.labels_reduce;      // trunc toward 0
    *py = (long long)my * h.labels_reduce;
    return *px >= 0 && *py >= 0 && *px < h.dim_x && *py < h.dim_y;
}

// depth z at pixel (px, py) -> height above the plane
__device__ __forceinline__ double height_at_pixel(long long px, long long py, float z, const HeightArgs &h)
{
    const float x = ((float)px - h.ppx) / h.fx, y = ((float)py - h.ppy) / h.fy;
    const double pt[4] = {(double)(z * x), (double)(z * y), (double)z, 1.0};
    double pz = 0.0;
    for (int k = 0; k < 4; ++k) pz += (double)h.plane[2 * 4 + k] * pt[k];
    return -pz;
}

__device__ __forceinline__ double height_of_mode(double mx, double my, const HeightArgs &h)
{
    long long px, py;
    if (!mode_pixel(mx, my, h, &px, &py)) return nan("");
    return height_at_pixel(px, py, (float)h.depth[py * h.dim_x + px], h);
}

// Workgroup (c, f) of 1024 threads is class c + 1 of frame f; a single frame is a grid y of 1.  `weights` is read only by the
// weighted policy and may be null there; `variances` is not null (the entry points refuse it).
template <class P, bool HEIGHTS>
__device__ __forceinline__ void modes_body(const uint16_t *labels, const uint16_t *weights, int dim_x, int dim_y, int L,
                                           const float *variances, int num_rounds, double *means_out, const HeightArgs &hp)
{
    extern __shared__ uint32_t s_list[];     // kListCap x (x | y << 16); when weighted, then kListCap 16-bit weights
    uint16_t *s_wgt = reinterpret_cast<uint16_t *>(s_list + P::kListCap);
    __shared__ double s_tab[kTabCap];        // round's weights by column, then by row (see the rounds below)
    __shared__ double s_red[2][kModesWaves][3];
    __shared__ uint32_t s_wave_cnt[kModesWaves];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t want = blockIdx.x + 1u;
    const uint32_t n_px = (uint32_t)dim_x * (uint32_t)dim_y;
    const size_t frame = blockIdx.y;
    labels += frame * n_px;
    if constexpr (P::kWeighted) { if (weights) weights += frame * n_px; }
    means_out += frame * (size_t)L * 2;

    // ---- list this class's counted pixels (label == class and, when weighted, weight != 0).  A wave takes kSteps x 512
    // pixels per batch (512 consecutive ones per step, the sixteen waves interleaved), eight per lane and step (one 16-byte
    // load where the maps are aligned, one by one otherwise: the same eight pixels either way; a step's eight match bits are
    // one byte of a packed register); a lane's pixels go to consecutive list slots, the lanes of a wave, the waves and the
    // batches follow each other in order -- positions come from a wave scan of the per-lane counts and the waves' totals, so
    // the order does not depend on timing (the rounds' sums depend on the list order, and must be reproducible).  A class
    // that does not fit the list is not listed at all: its rounds rescan the maps. ----
    uintptr_t align = reinterpret_cast<uintptr_t>(labels);
    if constexpr (P::kWeighted) align |= reinterpret_cast<uintptr_t>(weights);      // both maps, or neither
    const bool vec_ok = (align & 15u) == 0u;
    uint32_t n_class = 0;
    for (uint32_t batch0 = 0; batch0 < n_px; batch0 += kModesWaves * kSteps * 512u) {
        // step k of wave w covers the 512 pixels from batch0 + (k * 16 + w) * 512: a class is a few blobs, and with the
        // waves interleaved every 512 pixels all sixteen share the work of listing it (a wave alone on its SIMD issues
        // an instruction every ~8 cycles: with 16 consecutive rows per wave, the one or two waves that held a fingertip
        // took 13 000 cycles to list 140 pixels while the others idled)
        const uint32_t wbase = batch0 + (uint32_t)wave * 512u;
        uint32_t mp[(kSteps + 3) / 4];      // byte k & 3 of word k >> 2: which of the lane's eight pixels of step k are counted
#pragma unroll
        for (int q = 0; q < (kSteps + 3) / 4; ++q) mp[q] = 0u;
        uint32_t cnt = 0u;
#pragma unroll
        for (int k = 0; k < kSteps; ++k) {
            const uint32_t p0 = wbase + ((uint32_t)k * (kModesWaves * 64u) + (uint32_t)lane) * 8u;
            uint32_t bits = 0u;
            if (p0 + 8u <= n_px && vec_ok) {
                uint32_t v[8];
                unpack8(*reinterpret_cast<const uint4 *>(labels + p0), v);
#pragma unroll
                for (int j = 0; j < 8; ++j) bits |= v[j] == want ? 1u << j : 0u;
                if constexpr (P::kWeighted) {
                    if (bits != 0u && weights) {      // (the weights are loaded only where a label matched)
                        unpack8(*reinterpret_cast<const uint4 *>(weights + p0), v);
#pragma unroll
                        for (int j = 0; j < 8; ++j) bits &= ~(v[j] == 0u ? 1u << j : 0u);
                    }
                }
            } else {
                for (uint32_t j = 0; j < 8u; ++j) {
                    bool counted = p0 + j < n_px && labels[p0 + j] == want;
                    if constexpr (P::kWeighted) counted = counted && (!weights || weights[p0 + j] != 0);
                    if (counted) bits |= 1u << j;
                }
            }
            mp[k >> 2] |= bits << (8 * (k & 3));
            cnt += (uint32_t)__builtin_popcount(bits);
        }
        // exclusive scan of the lanes' counts (fixed shuffle pattern) and the wave's total
        uint32_t incl = cnt;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t up = __shfl_up(incl, o);
            if (lane >= o) incl += up;
        }
        const uint32_t lane_off = incl - cnt, wave_total = __shfl(incl, 63);
        __syncthreads();             // the previous batch's s_wave_cnt has been read
        if (lane == 0) s_wave_cnt[wave] = wave_total;
        __syncthreads();
        uint32_t at = n_class + lane_off, batch_total = 0u;
        for (int w = 0; w < kModesWaves; ++w) {
            if (w < wave) at += s_wave_cnt[w];
            batch_total += s_wave_cnt[w];
        }
        if (cnt != 0u && at < P::kListCap) {      // (a lane whose first slot is beyond the list writes nothing: the class overflows)
            const auto put = [&](uint32_t slot, uint32_t x, uint32_t y, uint32_t p) {
                if (slot < P::kListCap) {
                    s_list[slot] = x | (y << 16);
                    if constexpr (P::kWeighted) s_wgt[slot] = weights ? weights[p] : (uint16_t)1;
                }
            };
#pragma unroll
            for (int k = 0; k < kSteps; ++k) {
                const uint32_t mk = (mp[k >> 2] >> (8 * (k & 3))) & 0xFFu;
                if (mk == 0u) continue;
                const uint32_t p0 = wbase + ((uint32_t)k * (kModesWaves * 64u) + (uint32_t)lane) * 8u;
                const uint32_t y0 = p0 / (uint32_t)dim_x, x0 = p0 - y0 * (uint32_t)dim_x;   // one division per eight pixels
                if (dim_x >= 8) {
#pragma unroll
                    for (uint32_t j = 0; j < 8u; ++j) {      // the eight pixels sit in at most two rows
                        if ((mk >> j) & 1u) {
                            const uint32_t xj = x0 + j, wrap = xj >= (uint32_t)dim_x ? 1u : 0u;
                            put(at + (uint32_t)__builtin_popcount(mk & ((1u << j) - 1u)), xj - (wrap ? (uint32_t)dim_x : 0u),
                                y0 + wrap, p0 + j);
                        }
                    }
                } else {
                    uint32_t rest = mk, slot = at;
                    while (rest) {
                        const uint32_t j = (uint32_t)__builtin_ctz(rest);
                        rest &= rest - 1u;
                        uint32_t x = x0 + j, y = y0;
                        while (x >= (uint32_t)dim_x) { x -= (uint32_t)dim_x; ++y; }      // (rows narrower than 8 wrap more than once)
                        put(slot++, x, y, p0 + j);
                    }
                }
                at += (uint32_t)__builtin_popcount(mk);
            }
        }
        n_class += batch_total;
    }
    __syncthreads();
    const bool listed = n_class <= P::kListCap;
    const uint32_t n_list = listed ? n_class : 0u, rescan_from = listed ? n_px : 0u;

    double mx = 0.0, my = 0.0;
    const float vf = variances[blockIdx.x];
    const double v_2 = (double)(vf * vf);          // float product, as mean_shift.cu:42 (rule S6)
    // The kernel weight factorises: exp(-((x-mx)^2 + (y-my)^2) / 2v^2) = exp(-(x-mx)^2 / 2v^2) * exp(-(y-my)^2 / 2v^2).
    // A round therefore needs dim_x + dim_y exponentials per class (one table entry per thread), not one per pixel, and a
    // pixel's weight is the product of two table entries (a few ulp from the exponential of the sum; the reference's own
    // sums differ more from run to run).  That took the app's 424x240 map from ~6 us to ~1 us per round.
    const bool tables = (uint32_t)dim_x + (uint32_t)dim_y <= kTabCap && v_2 > 0.0;
    for (int round = 0; round < num_rounds; ++round) {
        double sx = 0.0, sy = 0.0, sw = 0.0;
        if (round > 0 && tables) {
            // (no barrier before rewriting the tables: every thread has passed the barrier of the previous round's
            // block_sum3, which it reaches only after its last table read)
            for (uint32_t i = tid; i < (uint32_t)dim_x + (uint32_t)dim_y; i += kModesThreads) {
                const double c = i < (uint32_t)dim_x ? (double)(int)i - mx : (double)(int)(i - (uint32_t)dim_x) - my;
                s_tab[i] = exp(-(c * c) / (2 * v_2));
            }
            __syncthreads();
        }
        // one pixel (xi, yi) of integer weight wi (looked at only when weighted)
        auto term = [&](uint32_t xi, uint32_t yi, uint32_t wi) {
            const double x = (double)(int)xi, y = (double)(int)yi, om = (double)(int)wi;
            if (round == 0) {
                if constexpr (P::kWeighted) { sx += om * x; sy += om * y; sw += om; }      // S5: integers, exact in any order
                else { sx += x; sy += y; sw += 1.0; }
            } else {
                const double dx = x - mx, dy = y - my;
                double w;
                if (tables) {
                    w = s_tab[xi] * s_tab[(uint32_t)dim_x + yi];
                } else {
                    const double dist_sq = (dx * dx) + (dy * dy);
                    w = exp(-dist_sq / (2 * v_2));
                }
                if constexpr (P::kWeighted) w = om * w;
                sx += dx * w; sy += dy * w; sw += w;
            }
        };
        if (round > 0 && tables) {
            // four list entries per trip, their table reads in flight together; added in the same order as one by one
            for (uint32_t i = tid; i < n_list; i += 4u * kModesThreads) {
                uint32_t e[4], om[4];
                double wx[4], wy[4];
#pragma unroll
                for (uint32_t u = 0; u < 4u; ++u) {
                    const bool in = i + u * kModesThreads < n_list;
                    e[u] = in ? s_list[i + u * kModesThreads] : 0u;
                    if constexpr (P::kWeighted) om[u] = in ? (uint32_t)s_wgt[i + u * kModesThreads] : 0u;
                }
#pragma unroll
                for (uint32_t u = 0; u < 4u; ++u) { wx[u] = s_tab[e[u] & 0xFFFFu]; wy[u] = s_tab[(uint32_t)dim_x + (e[u] >> 16)]; }
#pragma unroll
                for (uint32_t u = 0; u < 4u; ++u) {
                    if (i + u * kModesThreads < n_list) {
                        const double dx = (double)(int)(e[u] & 0xFFFFu) - mx, dy = (double)(int)(e[u] >> 16) - my;
                        double w = wx[u] * wy[u];
                        if constexpr (P::kWeighted) w = (double)(int)om[u] * w;
                        sx += dx * w; sy += dy * w; sw += w;
                    }
                }
            }
        } else {
            for (uint32_t i = tid; i < n_list; i += kModesThreads) {
                const uint32_t e = s_list[i];
                term(e & 0xFFFFu, e >> 16, P::kWeighted ? (uint32_t)s_wgt[i] : 1u);
            }
        }
        for (uint32_t p = rescan_from + tid; p < n_px; p += kModesThreads) {
            if (labels[p] != want) continue;
            uint32_t om = 1u;
            if constexpr (P::kWeighted) om = weights ? (uint32_t)weights[p] : 1u;
            if (om != 0u) term(p % (uint32_t)dim_x, p / (uint32_t)dim_x, om);      // S4: weight 0 contributes nothing
        }
        double tot[3];
        block_sum3(sx, sy, sw, s_red[round & 1], tot);
        mx = mx + tot[0] / tot[2];                 // 0/0 = NaN for a class without counted pixels, as in the reference
        my = my + tot[1] / tot[2];
    }
    if (tid == 0) { means_out[blockIdx.x * 2] = mx; means_out[blockIdx.x * 2 + 1] = my; }
    if constexpr (HEIGHTS) {
        // the heights of this class's fingertips ride on its workgroup (one launch less per hand and frame); ids that name
        // no class are the first workgroup's
        if (tid < hp.n_ids) {
            HeightArgs h = hp;
            h.depth += frame * (size_t)hp.dim_x * (size_t)hp.dim_y;
            double *heights = hp.heights + frame * (size_t)hp.heights_stride;
            const int c = hp.class_ids[tid];
            if (c == (int)want) heights[tid] = height_of_mode(mx, my, h);
            else if (blockIdx.x == 0 && (c < 1 || c > L)) heights[tid] = nan("");
        }
    }
}

}  // namespace

#endif  // RDF_MODES_HPP
