// soft_modes_hip.hip -- soft modes: the fingertip mean shift weighted by the forest's confidence.  Where rdf_mean_shift lets
// every pixel of a class pull equally, rdf_labels_weighted_modes gives each pixel an integer weight, and
// rdf_labels_composite_weights makes that weight for a layered stack: the product of the confidences of the layers that
// rdf_composite's walk visits.  Built into librdf_labels.so.  The contract (rules S) is in include/rdf_labels.h and
// tests/soft_modes_numpy.py restates it.
//
// k_composite_weights: one lane per pixel, a wave leaves at once when none of its 64 pixels starts a path (layer 0 says 0 or
// 65535: most of a frame).  Integer arithmetic, no LDS, no atomics: the bytes do not depend on anything but the inputs.
//
// k_weighted_modes: the shape of k_mean_shift_fused (mean_shift_hip.hip), which was arrived at by measurement: one workgroup
// of 1024 threads per (class, frame); the class's pixels are listed once in LDS, positions from wave scans, and every round
// runs on the list with fixed-order sums (thread-strided partial sums, a DPP row scan, rows and waves in index order).  A list
// entry is x | y << 16 plus a 16-bit weight; pixels of weight 0 are skipped at listing time and take no slot.  A class with
// more than kListCap counted pixels is not listed: its rounds rescan the label and weight maps.  No atomics, no hand-off
// between workgroups: the result is the same bits from run to run and from any pointer alignment (a lane is given the same
// eight pixels whether it loads them as one 16-byte vector or one by one).

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <mutex>

#include "../../include/rdf_labels.h"
#include "rdf_kernel_util.hpp"

namespace {

constexpr uint32_t kNoLabel = 65535u;
constexpr int kFlatThreads = 256;
constexpr int kThreads = 1024;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxClasses = 64;
constexpr uint32_t kListCap = 20480;     // counted pixels of one class kept in LDS: 6 bytes each, 122 880 B
constexpr uint32_t kTabCap = 3072;       // dim_x + dim_y the per-round tables cover (24 576 B): 148 288 B of the CU's 160 KB
constexpr int kSteps = 13;               // 16 waves x 13 steps x 512 pixels = 106 496 >= a 424 x 240 label map in one batch

// ---- composite weights (rules S1-S3) ----
__global__ void __launch_bounds__(kFlatThreads) k_composite_weights(const uint16_t *const *__restrict__ labels,
                                                                    const uint16_t *const *__restrict__ conf, int n_layers,
                                                                    uint32_t n_px, uint32_t dim_x, uint32_t lpix,
                                                                    const int2 *__restrict__ cond, int n_cond, int flip_x,
                                                                    uint16_t *__restrict__ out)
{
    const uint32_t p = blockIdx.x * (uint32_t)kFlatThreads + threadIdx.x;
    const bool inside = p < n_px;
    uint32_t l = inside ? (uint32_t)labels[0][p] : 0u;
    if (__ballot(l != 0u && l != kNoLabel) == 0ull) return;          // (most of a frame starts no path)
    if (!inside) return;
    long long off = 0;
    uint32_t w = 65535u;
    for (int j = 0; j < n_layers; ++j) {
        if (j > 0) l = labels[j][p];
        if (l == 0u || l == kNoLabel) return;                        // S1: nothing is written
        const long long e = off + (long long)l - 1;
        if (e < 0 || e >= n_cond) return;
        w = (w * (uint32_t)conf[j][p] + 32767u) / 65535u;            // S2: 65535^2 + 32767 < 2^32
        const int2 tv = cond[e];
        if (tv.x == 0) {
            uint32_t q = p;
            if (flip_x) {                                            // S3: the mirror of rdf_layered_run_hand's composite
                const uint32_t img = p / lpix, rem = p - img * lpix;
                const uint32_t y = rem / dim_x, x = rem - y * dim_x;
                q = img * lpix + y * dim_x + (dim_x - 1u - x);
            }
            out[q] = (uint16_t)w;
            return;
        }
        off = tv.y;
    }
}

// ---- weighted modes (rules S4-S7) ----
// One step of a row-wise (16 lanes) sum: v += the value `shr` lanes to the left in the same row (0.0 where there is none).
template <int SHR>
__device__ __forceinline__ double row_add_shr(double v)
{
    const int lo = __double2loint(v), hi = __double2hiint(v);
    const int plo = __builtin_amdgcn_update_dpp(0, lo, 0x110 + SHR, 0xF, 0xF, true);   // row_shr:SHR, bound_ctrl: 0 outside
    const int phi = __builtin_amdgcn_update_dpp(0, hi, 0x110 + SHR, 0xF, 0xF, true);
    return v + __hiloint2double(phi, plo);
}

// Sum over the wave in a fixed order: a shift-add scan inside each row of 16 lanes, the four row totals added in order.
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

// Sum of every thread's (a, b, c): inside a wave as above, then the waves one after the other.  s_red is double-buffered by
// the caller's round parity, so one barrier per call is enough.
__device__ __forceinline__ void block_sum3(double a, double b, double c, double (*s_red)[3], double *tot)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    a = wave_sum_f64(a); b = wave_sum_f64(b); c = wave_sum_f64(c);
    if (lane == 0) { s_red[wave][0] = a; s_red[wave][1] = b; s_red[wave][2] = c; }
    __syncthreads();
    double ta = 0.0, tb = 0.0, tc = 0.0;
    for (int w = 0; w < kWaves; ++w) { ta += s_red[w][0]; tb += s_red[w][1]; tc += s_red[w][2]; }
    tot[0] = ta; tot[1] = tb; tot[2] = tc;
}

struct HeightArgs {
    const int *class_ids;
    int n_ids;
    const uint16_t *depth;
    int dim_x, dim_y, labels_reduce;
    float fx, fy, ppx, ppy;
    const float *plane;
    double *heights;
    int heights_stride;
};

// rule S7: rdf_fingertip_heights' expression, operation for operation
__device__ __forceinline__ double height_of_mode(double mx, double my, const HeightArgs &h)
{
    double out = nan("");
    if (mx == mx && my == my && fabs(mx) < 1e9 && fabs(my) < 1e9) {
        const long long px = (long long)mx * h.labels_reduce, py = (long long)my * h.labels_reduce;   // trunc toward 0
        if (px >= 0 && py >= 0 && px < h.dim_x && py < h.dim_y) {
            const float z = (float)h.depth[py * h.dim_x + px];
            const float x = ((float)px - h.ppx) / h.fx, y = ((float)py - h.ppy) / h.fy;
            const double pt[4] = {(double)(z * x), (double)(z * y), (double)z, 1.0};
            double pz = 0.0;
            for (int k = 0; k < 4; ++k) pz += (double)h.plane[2 * 4 + k] * pt[k];
            out = -pz;
        }
    }
    return out;
}

// which of the eight pixels from p0 on are counted pixels of class `want` (bit j: pixel p0 + j)
__device__ __forceinline__ uint32_t match8(const uint16_t *__restrict__ labels, const uint16_t *__restrict__ weights,
                                           uint32_t p0, uint32_t n_px, uint32_t want, bool vec_ok)
{
    uint32_t bits = 0u;
    if (p0 + 8u <= n_px && vec_ok) {
        uint32_t v[8];
        unpack8(*reinterpret_cast<const uint4 *>(labels + p0), v);
#pragma unroll
        for (int j = 0; j < 8; ++j) bits |= v[j] == want ? 1u << j : 0u;
        if (bits != 0u && weights) {
            unpack8(*reinterpret_cast<const uint4 *>(weights + p0), v);
#pragma unroll
            for (int j = 0; j < 8; ++j) bits &= ~(v[j] == 0u ? 1u << j : 0u);
        }
    } else {
        for (uint32_t j = 0; j < 8u; ++j)
            if (p0 + j < n_px && labels[p0 + j] == want && (!weights || weights[p0 + j] != 0)) bits |= 1u << j;
    }
    return bits;
}

template <bool HEIGHTS>
__global__ __launch_bounds__(kThreads) void k_weighted_modes(const uint16_t *labels, const uint16_t *weights, int dim_x,
                                                             int dim_y, int L, const float *variances, int num_rounds,
                                                             double *means_out, const HeightArgs hp)
{
    extern __shared__ uint32_t s_list[];                         // kListCap x (x | y << 16), then kListCap 16-bit weights
    uint16_t *s_wgt = reinterpret_cast<uint16_t *>(s_list + kListCap);
    __shared__ double s_tab[kTabCap];
    __shared__ double s_red[2][kWaves][3];
    __shared__ uint32_t s_wave_cnt[kWaves];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t want = blockIdx.x + 1u;
    const uint32_t n_px = (uint32_t)dim_x * (uint32_t)dim_y;
    const size_t frame = blockIdx.y;
    labels += frame * n_px;
    if (weights) weights += frame * n_px;
    means_out += frame * (size_t)L * 2;

    // ---- list the class's counted pixels (label == class, weight != 0): the lister of k_mean_shift_fused.  Step k of wave w
    // covers the 512 pixels from batch0 + (k * 16 + w) * 512, eight consecutive ones per lane; a lane's pixels go to consecutive
    // slots, and the lanes of a wave, the waves and the batches follow each other in index order. ----
    const bool vec_ok = ((reinterpret_cast<uintptr_t>(labels) | reinterpret_cast<uintptr_t>(weights)) & 15u) == 0u;
    uint32_t n_class = 0;
    for (uint32_t batch0 = 0; batch0 < n_px; batch0 += kWaves * kSteps * 512u) {
        const uint32_t wbase = batch0 + (uint32_t)wave * 512u;
        uint32_t mp[(kSteps + 3) / 4];      // byte k & 3 of word k >> 2: which of the lane's eight pixels of step k are counted
#pragma unroll
        for (int q = 0; q < (kSteps + 3) / 4; ++q) mp[q] = 0u;
        uint32_t cnt = 0u;
#pragma unroll
        for (int k = 0; k < kSteps; ++k) {
            const uint32_t p0 = wbase + ((uint32_t)k * (kWaves * 64u) + (uint32_t)lane) * 8u;
            const uint32_t bits = p0 < n_px ? match8(labels, weights, p0, n_px, want, vec_ok) : 0u;
            mp[k >> 2] |= bits << (8 * (k & 3));
            cnt += (uint32_t)__builtin_popcount(bits);
        }
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
        for (int w = 0; w < kWaves; ++w) {
            if (w < wave) at += s_wave_cnt[w];
            batch_total += s_wave_cnt[w];
        }
        if (cnt != 0u && at < kListCap) {      // (a lane whose first slot is beyond the list writes nothing: the class overflows)
#pragma unroll
            for (int k = 0; k < kSteps; ++k) {
                uint32_t rest = (mp[k >> 2] >> (8 * (k & 3))) & 0xFFu;
                if (rest == 0u) continue;
                const uint32_t p0 = wbase + ((uint32_t)k * (kWaves * 64u) + (uint32_t)lane) * 8u;
                const uint32_t y0 = p0 / (uint32_t)dim_x, x0 = p0 - y0 * (uint32_t)dim_x;   // one division per eight pixels
                while (rest) {
                    const uint32_t j = (uint32_t)__builtin_ctz(rest);
                    rest &= rest - 1u;
                    uint32_t x = x0 + j, y = y0;
                    while (x >= (uint32_t)dim_x) { x -= (uint32_t)dim_x; ++y; }      // (once at most for rows of eight and more)
                    if (at < kListCap) {
                        s_list[at] = x | (y << 16);
                        s_wgt[at] = weights ? weights[p0 + j] : (uint16_t)1;
                    }
                    ++at;
                }
            }
        }
        n_class += batch_total;
    }
    __syncthreads();
    const bool listed = n_class <= kListCap;
    const uint32_t n_list = listed ? n_class : 0u, rescan_from = listed ? n_px : 0u;

    double mx = 0.0, my = 0.0;
    const float vf = variances[blockIdx.x];
    const double v_2 = (double)(vf * vf);          // S6: the float product, as rdf_mean_shift
    // the kernel weight factorises into a column and a row factor: dim_x + dim_y exponentials per round, not one per pixel
    const bool tables = (uint32_t)dim_x + (uint32_t)dim_y <= kTabCap && v_2 > 0.0;
    for (int round = 0; round < num_rounds; ++round) {
        double sx = 0.0, sy = 0.0, sw = 0.0;
        if (round > 0 && tables) {
            // (no barrier before rewriting the tables: every thread has passed the barrier of the previous round's block_sum3)
            for (uint32_t i = tid; i < (uint32_t)dim_x + (uint32_t)dim_y; i += kThreads) {
                const double c = i < (uint32_t)dim_x ? (double)(int)i - mx : (double)(int)(i - (uint32_t)dim_x) - my;
                s_tab[i] = exp(-(c * c) / (2 * v_2));
            }
            __syncthreads();
        }
        auto term = [&](uint32_t xi, uint32_t yi, uint32_t wi) {
            const double x = (double)(int)xi, y = (double)(int)yi, om = (double)(int)wi;
            if (round == 0) {
                sx += om * x; sy += om * y; sw += om;              // S5: integers, exact in any order
            } else {
                const double dx = x - mx, dy = y - my;
                double g;
                if (tables) {
                    g = s_tab[xi] * s_tab[(uint32_t)dim_x + yi];
                } else {
                    const double dist_sq = (dx * dx) + (dy * dy);
                    g = exp(-dist_sq / (2 * v_2));
                }
                const double wg = om * g;
                sx += dx * wg; sy += dy * wg; sw += wg;
            }
        };
        if (round > 0 && tables) {
            // four list entries per trip, their table reads in flight together; added in the same order as one by one
            for (uint32_t i = tid; i < n_list; i += 4u * kThreads) {
                uint32_t e[4], om[4];
                double wx[4], wy[4];
#pragma unroll
                for (uint32_t u = 0; u < 4u; ++u) {
                    const bool in = i + u * kThreads < n_list;
                    e[u] = in ? s_list[i + u * kThreads] : 0u;
                    om[u] = in ? (uint32_t)s_wgt[i + u * kThreads] : 0u;
                }
#pragma unroll
                for (uint32_t u = 0; u < 4u; ++u) { wx[u] = s_tab[e[u] & 0xFFFFu]; wy[u] = s_tab[(uint32_t)dim_x + (e[u] >> 16)]; }
#pragma unroll
                for (uint32_t u = 0; u < 4u; ++u) {
                    if (i + u * kThreads < n_list) {
                        const double dx = (double)(int)(e[u] & 0xFFFFu) - mx, dy = (double)(int)(e[u] >> 16) - my;
                        const double wg = (double)(int)om[u] * (wx[u] * wy[u]);
                        sx += dx * wg; sy += dy * wg; sw += wg;
                    }
                }
            }
        } else {
            for (uint32_t i = tid; i < n_list; i += kThreads) {
                const uint32_t e = s_list[i];
                term(e & 0xFFFFu, e >> 16, s_wgt[i]);
            }
        }
        for (uint32_t p = rescan_from + tid; p < n_px; p += kThreads) {
            if (labels[p] != want) continue;
            const uint32_t om = weights ? (uint32_t)weights[p] : 1u;
            if (om != 0u) term(p % (uint32_t)dim_x, p / (uint32_t)dim_x, om);      // S4: weight 0 contributes nothing
        }
        double tot[3];
        block_sum3(sx, sy, sw, s_red[round & 1], tot);
        mx = mx + tot[0] / tot[2];                 // 0/0 = NaN for a class without counted pixels
        my = my + tot[1] / tot[2];
    }
    if (tid == 0) { means_out[blockIdx.x * 2] = mx; means_out[blockIdx.x * 2 + 1] = my; }
    if (HEIGHTS) {
        // a class's fingertips ride on its workgroup; ids that name no class are the first workgroup's
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

constexpr long long kMaxElems = 1ll << 31;

}  // namespace

extern "C" {

int rdf_labels_composite_weights(const uint16_t *const *layer_labels, const uint16_t *const *layer_conf, int n_layers, int n_img,
                                 int dim_x, int dim_y, const int32_t *cond, int n_cond, int flip_x, uint16_t *weights_out,
                                 void *stream)
{
    if (n_layers < 1 || n_img < 0 || dim_x < 0 || dim_y < 0 || n_cond < 0 || dim_x > 65535 || dim_y > 65535) return RDF_ERR_BAD_ARG;
    if (misaligned(layer_labels, 8) || misaligned(layer_conf, 8) || misaligned(cond, 4) || misaligned(weights_out, 2))
        return RDF_ERR_BAD_ARG;
    const long long n_px = (long long)n_img * dim_x * dim_y;
    if (n_px >= kMaxElems) return RDF_ERR_TOO_LARGE;
    if (n_px == 0) return RDF_OK;
    if (!layer_labels || !layer_conf || !weights_out || (n_cond > 0 && !cond)) return RDF_ERR_NULL_PTR;
    hipLaunchKernelGGL(k_composite_weights, dim3(blocks(n_px, kFlatThreads)), dim3(kFlatThreads), 0, S(stream), layer_labels,
                       layer_conf, n_layers, (uint32_t)n_px, (uint32_t)dim_x, (uint32_t)dim_x * (uint32_t)dim_y,
                       reinterpret_cast<const int2 *>(cond), n_cond, flip_x ? 1 : 0, weights_out);
    return (int)hipGetLastError();
}

uint32_t rdf_labels_weighted_modes_list_cap(void) { return kListCap; }

int rdf_labels_weighted_modes(const uint16_t *labels, const uint16_t *weights, int n_img, int dim_x, int dim_y, int num_classes,
                              const float *variances, int num_rounds, double *means_out, const int *class_ids, int n_ids,
                              const uint16_t *depth, int depth_dim_x, int depth_dim_y, int labels_reduce, float fx, float fy,
                              float ppx, float ppy, const float *plane, double *heights_out, int heights_stride, void *stream)
{
    if (n_img < 0 || dim_x < 0 || dim_y < 0 || dim_x > 65535 || dim_y > 65535 || num_classes < 1 || num_classes > kMaxClasses ||
        num_rounds < 0 || n_ids < 0 || n_ids > kThreads)
        return RDF_ERR_BAD_ARG;
    if (n_ids > 0 && (depth_dim_x < 0 || depth_dim_y < 0 || labels_reduce < 1 || heights_stride < n_ids)) return RDF_ERR_BAD_ARG;
    if (misaligned(labels, 2) || misaligned(weights, 2) || misaligned(variances, 4) || misaligned(means_out, 8))
        return RDF_ERR_BAD_ARG;
    if (n_ids > 0 && (misaligned(class_ids, 4) || misaligned(depth, 2) || misaligned(plane, 4) || misaligned(heights_out, 8)))
        return RDF_ERR_BAD_ARG;
    const long long n_px = (long long)n_img * dim_x * dim_y;
    if (n_px >= kMaxElems || n_img > 65535) return RDF_ERR_TOO_LARGE;          // (the frame is the grid's y)
    if (n_ids > 0 && (long long)n_img * depth_dim_x * depth_dim_y >= kMaxElems) return RDF_ERR_TOO_LARGE;
    if (n_px == 0) return RDF_OK;
    if (!labels || !variances || !means_out) return RDF_ERR_NULL_PTR;
    if (n_ids > 0 && (!class_ids || !depth || !plane || !heights_out)) return RDF_ERR_NULL_PTR;

    const bool heights = n_ids > 0;
    const int lds_bytes = (int)(kListCap * (sizeof(uint32_t) + sizeof(uint16_t)));
    const void *kp = heights ? reinterpret_cast<const void *>(k_weighted_modes<true>)
                             : reinterpret_cast<const void *>(k_weighted_modes<false>);
    {   // more than 64 KB of dynamic LDS has to be allowed once per device and kernel
        static std::mutex mu;
        static unsigned long long allowed[2] = {0ull, 0ull};
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess) return (int)hipErrorNoDevice;
        std::lock_guard<std::mutex> lock(mu);
        unsigned long long &bits = allowed[heights ? 1 : 0];
        if (dev >= 64 || !((bits >> dev) & 1ull)) {
            const hipError_t e = hipFuncSetAttribute(kp, hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes);
            if (e != hipSuccess) return (int)e;
            if (dev < 64) bits |= 1ull << dev;
        }
    }
    const dim3 grid((unsigned)num_classes, (unsigned)n_img), block(kThreads);
    if (heights) {
        const HeightArgs h = {class_ids, n_ids, depth, depth_dim_x, depth_dim_y, labels_reduce, fx, fy, ppx, ppy, plane,
                              heights_out, heights_stride};
        hipLaunchKernelGGL(k_weighted_modes<true>, grid, block, lds_bytes, S(stream), labels, weights, dim_x, dim_y, num_classes,
                           variances, num_rounds, means_out, h);
    } else {
        hipLaunchKernelGGL(k_weighted_modes<false>, grid, block, lds_bytes, S(stream), labels, weights, dim_x, dim_y, num_classes,
                           variances, num_rounds, means_out, HeightArgs{});
    }
    return (int)hipGetLastError();
}

}  // extern "C"
