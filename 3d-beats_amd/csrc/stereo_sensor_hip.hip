// stereo_sensor_hip.hip -- the stereo depth sensor behind the hand renderer: a clean left and a clean right render become
// the depth frame an active stereo camera would report (projected dot pattern, census transform, block matching with a
// uniqueness and a left-right check, equiangular sub-pixel fit), many frames per call.  Built into librdf_labels.so; the
// rules (I, N, M, W, Z) are in include/rdf_labels.h under rdf_stereo_sense and restated in tests/stereo_numpy.py.  All
// arithmetic is integer, so the images do not depend on the order in which anything is visited.
//
// k_stereo_ir        one lane per pixel and camera: rule I.
// k_stereo_census    a workgroup owns 64 x 4 pixels of one image and reads them, with the 9 x 7 window's halo, from an LDS
//                    tile: rule N for both cameras in one launch.
// k_stereo_match<R>  rules M and W, once per direction.  A workgroup of four waves owns kTileX columns x kTileY rows; the
//                    OTHER image's census of those rows (+ 2 above and below), widened by D - 1 columns towards where the
//                    disparity points, is its LDS tile.  A wave owns kRows rows and is on its own after the tile is loaded:
//                    a lane owns one column (64 lanes: kTileX output columns and two either side for the box), keeps its OWN
//                    image's census of the wave's kRows + 4 rows in registers, and per d takes one popcount per row, slides
//                    the vertical 5-sum down the rows in registers and takes the horizontal 5-sum from its four neighbour
//                    lanes.  The winner's bookkeeping (C*, d*, second, cm, cp) stays in registers across the d loop.
// k_stereo_resolve   one lane per pixel: the left-right check, the reason code, rule Z.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/rdf_labels.h"
#include "rdf_kernel_util.hpp"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxDim = 32768;                          // per axis, as the renderer: a frame's pixels stay below 2^31
constexpr int kMaxDisparity = 256;
constexpr unsigned kMaxGrid = 1u << 20;                 // one-lane-per-element kernels stride beyond this many workgroups
constexpr unsigned kMaxGridZ = 65535u;
constexpr int kHamOutside = 62;                         // rule M
constexpr u64 kNoCensus = 1ull << 63;                   // an LDS tile entry outside the image (a census has 62 bits)
constexpr int kNone = 0xffff;                           // "no such cost" (a cost is 1550 at most)

constexpr int kCensusW = 64, kCensusH = 4;              // census: pixels per workgroup
constexpr int kCensusTileW = kCensusW + 8, kCensusTileH = kCensusH + 6;

constexpr int kRows = 8;                                // matcher: rows per wave (even: two rows share a shuffle)
constexpr int kWaves = kThreads / 64;
constexpr int kTileX = 60, kTileY = kRows * kWaves;     // output pixels per workgroup
constexpr int kTileRows = kTileY + 4;                   // rows of the LDS tile

// bit layout of a left winner in the workspace: d* | (sub + 8) << 8 | not unique << 15
constexpr int kSubShift = 8, kNotUniqueShift = 15;

__device__ __forceinline__ uint32_t texel(uint32_t row, uint32_t u, uint32_t threshold)
{
    const uint32_t h = mix32(row ^ u);
    return h < threshold ? 64u + (h & 127u) : 0u;
}

// ir uint8 [n_frames][2][H][W]; n_total = n_frames * 2 * H * W
__global__ void __launch_bounds__(kThreads) k_stereo_ir(long long n_total, int W, int H, const uint16_t *__restrict__ depth_l,
                                                        const uint16_t *__restrict__ depth_r, RdfStereoConfig cfg, uint32_t seed,
                                                        uint8_t *__restrict__ ir)
{
    const long long n_px = (long long)W * H;
    for (long long at = (long long)blockIdx.x * kThreads + threadIdx.x; at < n_total; at += (long long)gridDim.x * kThreads) {
        const long long img = at / n_px;
        const uint32_t p = (uint32_t)(at - img * n_px);
        const long long n = img >> 1;
        const int c = (int)(img & 1);
        const int y = (int)(p / (uint32_t)W), x = (int)(p - (uint32_t)y * (uint32_t)W);
        const uint32_t Z = (c ? depth_r : depth_l)[n * n_px + p];
        int v = cfg.ambient;
        if (Z > 0u && Z < 65535u) {
            const uint32_t num = (uint32_t)(c ? cfg.fb16 - cfg.fbp16 : cfg.fbp16) + (Z >> 1);       // < 2^31
            const long long s = (long long)(num / Z);
            const long long sq = 16ll * x + (c ? s : -s);
            const uint32_t u = (uint32_t)(int32_t)(sq >> 4);
            const uint32_t fr = (uint32_t)(sq & 15);
            const uint32_t row = mix32(cfg.pattern_seed + (uint32_t)y * 0x9e3779b9u);
            v += (int)(((16u - fr) * texel(row, u, cfg.dot_threshold) + fr * texel(row, u + 1u, cfg.dot_threshold)) >> 4);
        }
        if (cfg.ir_noise_amp > 0) {
            const uint32_t h = mix32(mix32(seed + (uint32_t)n * 0x9e3779b9u + (uint32_t)c * 0x632be5abu) ^ p);
            v += (int)(h % (uint32_t)(2 * cfg.ir_noise_amp + 1)) - cfg.ir_noise_amp;
        }
        ir[at] = (uint8_t)min(max(v, 0), 255);
    }
}

// census u64 [n_img][H][W] of ir uint8 [n_img][H][W], n_img = 2 * n_frames
__global__ void __launch_bounds__(kThreads) k_stereo_census(long long n_img, int W, int H, int margin,
                                                            const uint8_t *__restrict__ ir, u64 *__restrict__ census)
{
    __shared__ uint8_t tile[kCensusTileH][kCensusTileW];
    const int tx = threadIdx.x % kCensusW, ty = threadIdx.x / kCensusW;
    const int x0 = blockIdx.x * kCensusW, y0 = blockIdx.y * kCensusH;
    const long long n_px = (long long)W * H;
    for (long long img = blockIdx.z; img < n_img; img += gridDim.z) {
        const uint8_t *src = ir + img * n_px;
        __syncthreads();                                // the previous image's tile has been read
        for (int k = threadIdx.x; k < kCensusTileH * kCensusTileW; k += kThreads) {
            const int r = k / kCensusTileW, q = k - r * kCensusTileW;
            const int yy = y0 - 3 + r, xx = x0 - 4 + q;
            tile[r][q] = (xx >= 0 && xx < W && yy >= 0 && yy < H) ? src[(long long)yy * W + xx] : (uint8_t)0;
        }
        __syncthreads();
        const int x = x0 + tx, y = y0 + ty;
        if (x < W && y < H) {
            const int bar = (int)tile[ty + 3][tx + 4] + margin;
            u64 bits = 0;
            int k = 0;
#pragma unroll
            for (int dy = -3; dy <= 3; ++dy)
#pragma unroll
                for (int dx = -4; dx <= 4; ++dx)
                    if (dx != 0 || dy != 0) {
                        bits |= (u64)((int)tile[ty + 3 + dy][tx + 4 + dx] > bar) << k;
                        ++k;
                    }
            census[img * n_px + (long long)y * W + x] = bits;
        }
    }
}

// census u64 [n_frames][2][H][W].  RIGHT false: win_l uint16 [n_frames][H][W] (layout above); true: win_r uint8, dR.
// Tile column q holds the other image's column other0 + q; the lane of column `col` reads other column col - d (left pass)
// or col + d (right pass): tile column lane + D - 1 - d, or lane + d, both within [0, 64 + D - 1).
template <bool RIGHT>
__global__ void __launch_bounds__(kThreads, 2) k_stereo_match(int n_frames, int W, int H, int D, int uniqueness,
                                                           const u64 *__restrict__ census, uint16_t *__restrict__ win_l,
                                                           uint8_t *__restrict__ win_r)
{
    extern __shared__ u64 other[];                      // [kTileRows][tile_w]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int tile_w = 64 + D - 1;
    const int x0 = blockIdx.x * kTileX, y0 = blockIdx.y * kTileY;
    const int col = x0 - 2 + lane;
    const int other0 = RIGHT ? x0 - 2 : x0 - 2 - (D - 1);
    const int wy0 = y0 + wave * kRows;                  // the wave's first output row
    const long long n_px = (long long)W * H;
    for (int n = blockIdx.z; n < n_frames; n += gridDim.z) {
        const u64 *own = census + ((long long)n * 2 + (RIGHT ? 1 : 0)) * n_px;
        const u64 *oth = census + ((long long)n * 2 + (RIGHT ? 0 : 1)) * n_px;
        __syncthreads();                                // the previous frame's tile has been read
        for (int k = threadIdx.x; k < kTileRows * tile_w; k += kThreads) {
            const int r = k / tile_w, q = k - r * tile_w;
            const int yy = y0 - 2 + r, xx = other0 + q;
            other[k] = (xx >= 0 && xx < W && yy >= 0 && yy < H) ? oth[(long long)yy * W + xx] : kNoCensus;
        }
        __syncthreads();
        if (wy0 >= H) continue;                         // the whole wave, and every lane comes back to the barrier above

        u64 mine[kRows + 4];
        unsigned inside = 0;
#pragma unroll
        for (int r = 0; r < kRows + 4; ++r) {
            const int yy = wy0 - 2 + r;
            const bool in = col >= 0 && col < W && yy >= 0 && yy < H;
            mine[r] = in ? own[(long long)yy * W + col] : 0ull;
            inside |= (in ? 1u : 0u) << r;
        }
        int best[kRows], best_d[kRows], second[kRows], cm[kRows], cp[kRows], lagged[kRows], prev[kRows];
#pragma unroll
        for (int j = 0; j < kRows; ++j) {
            best[j] = second[j] = cm[j] = cp[j] = lagged[j] = prev[j] = kNone;
            best_d[j] = 0;
        }
        const u64 *column = other + (wave * kRows) * tile_w + (RIGHT ? lane : lane + D - 1);
#pragma unroll 1
        for (int d = 0; d < D; ++d) {
            const u64 *t = RIGHT ? column + d : column - d;
            int ham[kRows + 4];
#pragma unroll
            for (int r = 0; r < kRows + 4; ++r) {
                const u64 b = t[r * tile_w];
                ham[r] = (((inside >> r) & 1u) != 0u && (b >> 63) == 0ull) ? __popcll(mine[r] ^ b) : kHamOutside;
            }
            // the vertical 5-sums, sliding down the rows; then the horizontal 5-sum of two rows at a time: a cost is 1550 at
            // most, so two ride in one register through the neighbour lanes' shuffles without a carry between them.  Lanes 0,
            // 1, 62 and 63 get a wrapped neighbour and own no output
            int cost[kRows];
            cost[0] = ham[0] + ham[1] + ham[2] + ham[3] + ham[4];
#pragma unroll
            for (int j = 1; j < kRows; ++j) cost[j] = cost[j - 1] + ham[j + 4] - ham[j - 1];
#pragma unroll
            for (int j = 0; j < kRows; j += 2) {
                const int pair = cost[j] | (cost[j + 1] << 16);
                const int sum = pair + __shfl(pair, lane - 2) + __shfl(pair, lane - 1) + __shfl(pair, lane + 1) + __shfl(pair, lane + 2);
                cost[j] = sum & 0xffff;
                cost[j + 1] = sum >> 16;
            }
#pragma unroll
            for (int j = 0; j < kRows; ++j) {
                const int c = cost[j];
                if (RIGHT) {
                    if (c < best[j]) best[j] = c, best_d[j] = d;
                } else {
                    // lagged = the least cost over d' <= d - 2, prev = the cost of d - 1.  Selects, no branches: every lane
                    // of the wave does the same work whatever its pixel decides
                    const bool better = c < best[j], next = d == best_d[j] + 1;
                    second[j] = better ? lagged[j] : next ? second[j] : min(second[j], c);
                    cm[j] = better ? prev[j] : cm[j];
                    cp[j] = better ? kNone : next ? c : cp[j];
                    best_d[j] = better ? d : best_d[j];
                    best[j] = min(best[j], c);
                    lagged[j] = min(lagged[j], prev[j]);
                    prev[j] = c;
                }
            }
        }
        const bool owns = lane >= 2 && lane < 2 + kTileX && col < W;
#pragma unroll
        for (int j = 0; j < kRows; ++j) {
            const int y = wy0 + j;
            if (!owns || y >= H) continue;
            const long long at = (long long)n * n_px + (long long)y * W + col;
            if (RIGHT) {
                win_r[at] = (uint8_t)best_d[j];
            } else {
                int sub = 0;
                if (best_d[j] >= 1 && best_d[j] <= D - 2) {
                    const int den = max(cm[j] - best[j], cp[j] - best[j]);
                    if (den > 0 && best[j] > 0) {                                       // an exact match stays whole
                        const int num = 16 * (cm[j] - cp[j]) + den;                     // floor(num / (2 den))
                        const int q = num >= 0 ? num / (2 * den) : -((-num + 2 * den - 1) / (2 * den));
                        sub = min(max(q, -8), 8);
                    }
                }
                const bool unique = second[j] == kNone || best[j] * 100 < second[j] * (100 - uniqueness);
                win_l[at] = (uint16_t)(best_d[j] | ((sub + 8) << kSubShift) | ((unique ? 0 : 1) << kNotUniqueShift));
            }
        }
    }
}

__global__ void __launch_bounds__(kThreads) k_stereo_resolve(long long n_total, int W, int H, RdfStereoConfig cfg,
                                                             uint16_t empty_depth, const uint16_t *__restrict__ win_l,
                                                             const uint8_t *__restrict__ win_r,
                                                             const uint16_t *__restrict__ labels_l,
                                                             uint16_t *__restrict__ depth_out, uint16_t *__restrict__ labels_out,
                                                             uint16_t *__restrict__ dq_out, uint8_t *__restrict__ reason_out)
{
    for (long long at = (long long)blockIdx.x * kThreads + threadIdx.x; at < n_total; at += (long long)gridDim.x * kThreads) {
        const int x = (int)(at % W);
        const int w = win_l[at];
        const int d = w & 255, sub = ((w >> kSubShift) & 31) - 8;
        const int dq = 16 * d + sub;
        const bool lr = x - d >= 0 && abs((int)win_r[at - d] - d) <= cfg.lr_max;
        const int reason = (w >> kNotUniqueShift) | (lr ? 0 : 2) | (dq >= cfg.dq_min ? 0 : 4);
        uint16_t depth = empty_depth, label = 0;
        if (reason == 0) {
            depth = (uint16_t)min(max((cfg.fb16 + dq / 2) / dq, 1), 65534);
            label = labels_l[at];
        }
        depth_out[at] = depth;
        labels_out[at] = label;
        if (dq_out) dq_out[at] = (uint16_t)dq;
        if (reason_out) reason_out[at] = (uint8_t)reason;
    }
}

inline unsigned blocks_for(long long n) { return (unsigned)min((n + kThreads - 1) / kThreads, (long long)kMaxGrid); }

// what both entry points check alike; > 0: the batch's pixels, 0: no pixels, < 0: rejected
long long check_shape(int n_frames, int dim_x, int dim_y, const RdfStereoConfig &c)
{
    if (n_frames < 1 || dim_x < 0 || dim_y < 0) return RDF_ERR_BAD_ARG;
    if (dim_x > kMaxDim || dim_y > kMaxDim) return RDF_ERR_TOO_LARGE;
    if (c.fbp16 < 0 || c.fb16 < c.fbp16 || c.fb16 >= 0x7fffffff - 0x7fff || c.max_disparity < 1 ||
        c.max_disparity > kMaxDisparity || c.ambient < 0 || c.ambient > 255 || c.ir_noise_amp < 0 || c.ir_noise_amp > 255 ||
        c.census_margin < 0 || c.census_margin > 255 || c.uniqueness < 0 || c.uniqueness > 100 || c.lr_max < 0 ||
        c.lr_max > 255 || c.dq_min < 1 || c.dq_min > 65535)
        return RDF_ERR_BAD_ARG;
    const long long n_total = (long long)n_frames * dim_x * dim_y;
    if (n_total >= (1ll << 39)) return RDF_ERR_TOO_LARGE;
    return n_total;
}

void launch_ir(long long n_total, int dim_x, int dim_y, const uint16_t *depth_l, const uint16_t *depth_r,
               const RdfStereoConfig &cfg, uint32_t seed, uint8_t *ir, void *stream)
{
    hipLaunchKernelGGL(k_stereo_ir, dim3(blocks_for(2 * n_total)), dim3(kThreads), 0, S(stream), 2 * n_total, dim_x, dim_y,
                       depth_l, depth_r, cfg, seed, ir);
}

inline int match_lds_bytes(int D) { return kTileRows * (64 + D - 1) * (int)sizeof(u64); }       // 91 872 at D = 256

// before anything is launched: a tile beyond 64 KiB has to be allowed per kernel.  The attribute is an upper bound and one per
// kernel for the whole process, so it is always set to the widest range's tile (D = 256): two sensors with two ranges on two
// threads then cannot lower it under each other's launch.
template <bool RIGHT>
int allow_match_lds(int D)
{
    if (match_lds_bytes(D) <= 64 * 1024) return RDF_OK;
    return (int)hipFuncSetAttribute(reinterpret_cast<const void *>(k_stereo_match<RIGHT>),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, match_lds_bytes(256));
}

template <bool RIGHT>
void launch_match(int n_frames, int dim_x, int dim_y, const RdfStereoConfig &cfg, const u64 *census, uint16_t *win_l,
                  uint8_t *win_r, void *stream)
{
    const int lds = match_lds_bytes(cfg.max_disparity);
    const dim3 grid((unsigned)((dim_x + kTileX - 1) / kTileX), (unsigned)((dim_y + kTileY - 1) / kTileY),
                    (unsigned)n_frames < kMaxGridZ ? (unsigned)n_frames : kMaxGridZ);
    hipLaunchKernelGGL(k_stereo_match<RIGHT>, grid, dim3(kThreads), (size_t)lds, S(stream), n_frames, dim_x, dim_y,
                       cfg.max_disparity, cfg.uniqueness, census, win_l, win_r);
}

}  // namespace

extern "C" {

size_t rdf_stereo_workspace_bytes(int n_frames, int dim_x, int dim_y, int max_disparity)
{
    if (n_frames < 1 || dim_x < 0 || dim_y < 0 || dim_x > kMaxDim || dim_y > kMaxDim || max_disparity < 1 ||
        max_disparity > kMaxDisparity)
        return 0;
    return (size_t)n_frames * (size_t)dim_x * (size_t)dim_y * 21;
}

int rdf_stereo_ir(int n_frames, int dim_x, int dim_y, const uint16_t *depth_l, const uint16_t *depth_r, RdfStereoConfig config,
                  uint32_t seed, uint8_t *ir_out, void *stream)
{
    const long long n_total = check_shape(n_frames, dim_x, dim_y, config);
    if (n_total <= 0) return (int)n_total;
    if (!depth_l || !depth_r || !ir_out) return RDF_ERR_NULL_PTR;
    if (misaligned(depth_l, 2) || misaligned(depth_r, 2)) return RDF_ERR_BAD_ARG;
    launch_ir(n_total, dim_x, dim_y, depth_l, depth_r, config, seed, ir_out, stream);
    return (int)hipGetLastError();
}

int rdf_stereo_sense(int n_frames, int dim_x, int dim_y, const uint16_t *depth_l, const uint16_t *labels_l,
                     const uint16_t *depth_r, RdfStereoConfig config, uint32_t seed, uint16_t empty_depth, void *workspace,
                     uint16_t *depth_out, uint16_t *labels_out, uint8_t *ir_out, uint16_t *dq_out, uint8_t *reason_out,
                     void *stream)
{
    const long long n_total = check_shape(n_frames, dim_x, dim_y, config);
    if (n_total <= 0) return (int)n_total;
    if (!depth_l || !labels_l || !depth_r || !workspace || !depth_out || !labels_out) return RDF_ERR_NULL_PTR;
    if (misaligned(depth_l, 2) || misaligned(labels_l, 2) || misaligned(depth_r, 2) || misaligned(workspace, 8) ||
        misaligned(depth_out, 2) || misaligned(labels_out, 2) || misaligned(dq_out, 2) || depth_out == labels_out)
        return RDF_ERR_BAD_ARG;
    // the workspace: census u64 [N][2][H][W], left winners u16 [N][H][W], IR u8 [N][2][H][W], right winners u8 [N][H][W]
    uint8_t *ws = static_cast<uint8_t *>(workspace);
    u64 *census = reinterpret_cast<u64 *>(ws);
    uint16_t *win_l = reinterpret_cast<uint16_t *>(ws + 16 * n_total);
    uint8_t *ir = ir_out ? ir_out : ws + 18 * n_total;
    uint8_t *win_r = ws + 20 * n_total;

    int rc = allow_match_lds<false>(config.max_disparity);
    if (rc == RDF_OK) rc = allow_match_lds<true>(config.max_disparity);
    if (rc != RDF_OK) return rc;
    launch_ir(n_total, dim_x, dim_y, depth_l, depth_r, config, seed, ir, stream);
    const long long n_img = 2ll * n_frames;
    const dim3 census_grid((unsigned)((dim_x + kCensusW - 1) / kCensusW), (unsigned)((dim_y + kCensusH - 1) / kCensusH),
                           n_img < (long long)kMaxGridZ ? (unsigned)n_img : kMaxGridZ);
    hipLaunchKernelGGL(k_stereo_census, census_grid, dim3(kThreads), 0, S(stream), n_img, dim_x, dim_y, config.census_margin,
                       ir, census);
    launch_match<false>(n_frames, dim_x, dim_y, config, census, win_l, win_r, stream);
    launch_match<true>(n_frames, dim_x, dim_y, config, census, win_l, win_r, stream);
    hipLaunchKernelGGL(k_stereo_resolve, dim3(blocks_for(n_total)), dim3(kThreads), 0, S(stream), n_total, dim_x, dim_y, config,
                       empty_depth, win_l, win_r, labels_l, depth_out, labels_out, dq_out, reason_out);
    return (int)hipGetLastError();
}

}  // extern "C"
