// depth_filter_hip.hip -- the depth post-filter between a stereo camera's raw frames and rdf_frame_front: an edge-preserving
// spatial mean (rule S), a temporal filter with persistence (rule T) and a row-wise hole fill (rule F), integer throughout.
// Built into librdf_frontend.so.  The rules are in include/rdf_frontend.h; tests/depth_filter_numpy.py restates them.
//
// ONE launch per call, whatever the number of frames.  A workgroup of 256 threads owns one whole row and walks the call's
// frames in order; a thread owns one chunk of 8 consecutive pixels of it (a row is at most 256 chunks).  The T state of its 8
// pixels lives in registers from the first frame to the last and is read and written once per call.  Per frame:
//   1. the row and its R halo rows above and below go to LDS as whole chunks (pixels beyond the row's end, the halo rows
//      beyond the frame and 8 columns of padding on either side are 0 = "no reading", which is also what rule S makes of a
//      pixel outside the frame, so the window needs no bounds);                                            -- barrier
//      the NEXT frame's chunks are loaded into registers here, so that they travel while this frame is computed;
//   2. S from LDS (three reads per window row: 2 + 8 + 2 pixels; a tap is four instructions: |n - c|, the compare, a select
//      and ONE add, the sum and the count sharing a register), T in registers, T's output to a second LDS row with, per
//      chunk, the columns of its first and its last reading;                                               -- barrier
//   3. F: inside a chunk by a sweep over its 8 pixels; the nearest reading beyond the chunk is found by walking the chunk
//      records of the row outwards until one has a reading or max_gap is passed (at most max_gap / 8 + 1 records, each two
//      bytes of LDS; the walk is only made by a chunk that begins or ends with a hole).  Then the stores.
// Global accesses are 16 bytes per lane (8 for the flags) when dim_x is a multiple of 8 and every pointer is 16-byte
// aligned, element by element otherwise.  A row's halo is read by its neighbours' workgroups too: 1 + 2 R reads of every
// input pixel, all but the first from the L2.  No atomics, vector stores only.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/rdf_frontend.h"
#include "rdf_kernel_util.hpp"

namespace {

constexpr int kThreads = 256;
constexpr int kChunk = 8;                                   // pixels: 16 bytes of depth
constexpr int kPad = 8;                                     // zero columns left and right of a staged row (>= the radius, and
                                                            // a multiple of 8 so that chunks stay 16-byte aligned in LDS)
static_assert(RDF_DEPTH_FILTER_MAX_WIDTH == kThreads * kChunk, "a row is at most one chunk per thread");

constexpr int kNoFirst = 0x7fff;                            // a chunk record's "first reading" when it has none
constexpr int kNoLast = -1;
constexpr uint32_t kFar = 0xfff00000u;                      // a hole among rule S's neighbours: further than any delta from any reading
constexpr uint32_t kOne = 1u << 24;                         // rule S's count, above its sum (<= 25 * 65535 < 2^24) in one register

struct Chunk8 {
    uint32_t w[4];                                          // 8 uint16, little endian
};

__device__ __forceinline__ uint32_t px(const Chunk8 &c, int i) { return (c.w[i >> 1] >> ((i & 1) * 16)) & 0xffffu; }

// 8 pixels of a row from global memory; beyond the row's end: 0
__device__ __forceinline__ Chunk8 load_chunk(const uint16_t *row, int x0, int W, bool vec)
{
    Chunk8 c;
    if (vec) {
        const uint4 v = *reinterpret_cast<const uint4 *>(row + x0);
        c.w[0] = v.x; c.w[1] = v.y; c.w[2] = v.z; c.w[3] = v.w;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t lo = x0 + 2 * k < W ? row[x0 + 2 * k] : 0u;
            const uint32_t hi = x0 + 2 * k + 1 < W ? row[x0 + 2 * k + 1] : 0u;
            c.w[k] = lo | (hi << 16);
        }
    }
    return c;
}

template <int R>
__global__ void __launch_bounds__(kThreads)
k_depth_filter(int n, int W, int H, const uint16_t *__restrict__ depth, RdfDepthFilterConfig cfg, uint32_t *__restrict__ state,
               uint16_t *__restrict__ depth_out, uint8_t *__restrict__ flags_out, int vec)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    constexpr int kStaged = 1 + 2 * R;                      // rows in LDS
    const int cpr = (W + kChunk - 1) / kChunk;              // chunks per row
    const int wp = cpr * kChunk;                            // a row, rounded up to whole chunks
    const int stride = wp + 2 * kPad;                       // of a staged row, in pixels
    uint16_t *stage = reinterpret_cast<uint16_t *>(lds);                        // [kStaged][stride]: the raw row and its halo
    uint16_t *timg = stage + kStaged * stride;                                  // [wp]: T's output
    int16_t *rec_first = reinterpret_cast<int16_t *>(timg + wp);                // [cpr]
    int16_t *rec_last = rec_first + cpr;                                        // [cpr]

    const int tid = threadIdx.x;
    const int y = blockIdx.x;                               // this workgroup's row
    const bool mine = tid < cpr;                            // this thread has a chunk
    const int x0 = tid * kChunk;
    const size_t frame_px = (size_t)W * H;
    const size_t at = (size_t)y * W + x0;                   // the chunk within a frame
    const bool temporal = cfg.temporal != 0;

    // the padding columns are written once: nothing else ever touches them
    for (int i = tid; i < kStaged * 2 * kPad; i += kThreads) {
        const int r = i / (2 * kPad), k = i % (2 * kPad);
        stage[r * stride + (k < kPad ? k : wp + k)] = 0;
    }

    // this thread's chunk of staged row j of a frame: row y - R + j; 0 beyond the frame
    auto fetch = [&](const uint16_t *frame, int j) -> Chunk8 {
        const int yy = y - R + j;
        if (yy < 0 || yy >= H) return Chunk8{{0u, 0u, 0u, 0u}};
        return load_chunk(frame + (size_t)yy * W, x0, W, vec != 0);
    };

    // the T state of this thread's pixels: (v << 8) | hist
    uint32_t st[kChunk];
#pragma unroll
    for (int i = 0; i < kChunk; ++i) st[i] = 0u;
    if (temporal && mine) {
        const uint32_t *p = state + at;
        if (vec) {
            const uint4 a = *reinterpret_cast<const uint4 *>(p), b = *reinterpret_cast<const uint4 *>(p + 4);
            st[0] = a.x; st[1] = a.y; st[2] = a.z; st[3] = a.w;
            st[4] = b.x; st[5] = b.y; st[6] = b.z; st[7] = b.w;
        } else {
#pragma unroll
            for (int i = 0; i < kChunk; ++i)
                if (x0 + i < W) st[i] = p[i];
        }
    }

    Chunk8 next[kStaged];
    if (mine) {
#pragma unroll
        for (int j = 0; j < kStaged; ++j) next[j] = fetch(depth, j);
    }

    const uint32_t span_mask = (1u << cfg.persist_span) - 1u;
    const uint32_t alpha = (uint32_t)cfg.temporal_alpha, delta_s = (uint32_t)cfg.spatial_delta;
    const int delta_t16 = 16 * cfg.temporal_delta, need = cfg.persist_need;
    const int max_gap = cfg.max_gap, mode = max_gap > 0 ? cfg.fill_mode : 0;

    for (int f = 0; f < n; ++f) {
        // ---- 1. this frame's rows to LDS, the next frame's into registers
        if (mine) {
#pragma unroll
            for (int j = 0; j < kStaged; ++j)
                *reinterpret_cast<uint4 *>(stage + j * stride + kPad + x0) = make_uint4(next[j].w[0], next[j].w[1], next[j].w[2], next[j].w[3]);
        }
        __syncthreads();
        if (mine && f + 1 < n) {
            const uint16_t *frame = depth + (size_t)(f + 1) * frame_px;
#pragma unroll
            for (int j = 0; j < kStaged; ++j) next[j] = fetch(frame, j);
        }

        // ---- 2. S and T
        uint32_t tv[kChunk];                                // T's output
        uint32_t fl[2] = {0u, 0u};                          // the flags, four pixels to a word
        if (mine) {
            const uint16_t *centre = stage + R * stride + kPad + x0;
            uint32_t sv[kChunk];
            {
                const uint4 m = *reinterpret_cast<const uint4 *>(centre);
                const Chunk8 cc = {{m.x, m.y, m.z, m.w}};
#pragma unroll
                for (int i = 0; i < kChunk; ++i) sv[i] = px(cc, i);
            }
            if (R > 0) {
                uint32_t acc[kChunk];                       // count << 24 | sum
#pragma unroll
                for (int i = 0; i < kChunk; ++i) acc[i] = 0u;
#pragma unroll
                for (int dy = -R; dy <= R; ++dy) {
                    const uint16_t *p = centre + dy * stride;
                    const uint32_t lo = *reinterpret_cast<const uint32_t *>(p - 2);
                    const uint4 m = *reinterpret_cast<const uint4 *>(p);
                    const uint32_t hi = *reinterpret_cast<const uint32_t *>(p + kChunk);
                    uint32_t v[kChunk + 4];                 // columns x0 - 2 .. x0 + 9
                    v[0] = lo & 0xffffu; v[1] = lo >> 16;
                    v[2] = m.x & 0xffffu; v[3] = m.x >> 16; v[4] = m.y & 0xffffu; v[5] = m.y >> 16;
                    v[6] = m.z & 0xffffu; v[7] = m.z >> 16; v[8] = m.w & 0xffffu; v[9] = m.w >> 16;
                    v[10] = hi & 0xffffu; v[11] = hi >> 16;
                    uint32_t far[kChunk + 4], one[kChunk + 4];
#pragma unroll
                    for (int k = 2 - R; k < kChunk + 2 + R; ++k) {
                        far[k] = v[k] != 0u ? v[k] : kFar;
                        one[k] = v[k] + kOne;
                    }
#pragma unroll
                    for (int i = 0; i < kChunk; ++i) {
#pragma unroll
                        for (int dx = -R; dx <= R; ++dx)
                            acc[i] += __usad(far[i + 2 + dx], sv[i], 0u) <= delta_s ? one[i + 2 + dx] : 0u;
                    }
                }
#pragma unroll
                for (int i = 0; i < kChunk; ++i) {
                    const uint32_t sum = acc[i] & (kOne - 1u), cnt = acc[i] >> 24;
                    if (sv[i] != 0u) sv[i] = (2u * sum + cnt) / (2u * cnt);                // cnt >= 1: the centre
                }
            }
            if (temporal) {
#pragma unroll
                for (int i = 0; i < kChunk; ++i) {
                    const uint32_t s = st[i];
                    const uint32_t v = s >> 8, hist = s & 255u;
                    const uint32_t c16 = sv[i] * 16u;
                    const bool reading = sv[i] != 0u;
                    const int d = (int)c16 - (int)v;
                    const bool blend = reading && v != 0u && (d < 0 ? -d : d) <= delta_t16;
                    const uint32_t nv = blend ? (alpha * c16 + (256u - alpha) * v + 128u) >> 8 : c16;
                    const bool persist = !reading && v != 0u && __popc(hist & span_mask) >= need;
                    const uint32_t out = reading ? (nv + 8u) >> 4 : (persist ? (v + 8u) >> 4 : 0u);
                    const uint32_t hist2 = ((hist << 1) | (reading ? 1u : 0u)) & 255u;
                    uint32_t v2 = reading ? nv : v;
                    if (!reading && hist2 == 0u) v2 = 0u;
                    st[i] = (v2 << 8) | hist2;
                    tv[i] = out;
                    fl[i >> 2] |= ((blend ? 1u : 0u) | (persist ? 2u : 0u)) << ((i & 3) * 8);
                }
            } else {
#pragma unroll
                for (int i = 0; i < kChunk; ++i) tv[i] = sv[i];
            }
            if (mode != 0) {
                int first = kNoFirst, last = kNoLast;
#pragma unroll
                for (int i = kChunk - 1; i >= 0; --i)
                    if (tv[i] != 0u) first = x0 + i;
#pragma unroll
                for (int i = 0; i < kChunk; ++i)
                    if (tv[i] != 0u) last = x0 + i;
                *reinterpret_cast<uint4 *>(timg + x0) =
                    make_uint4(tv[0] | (tv[1] << 16), tv[2] | (tv[3] << 16), tv[4] | (tv[5] << 16), tv[6] | (tv[7] << 16));
                rec_first[tid] = (int16_t)first;
                rec_last[tid] = (int16_t)last;
            }
        }
        __syncthreads();        // T's row is complete; and every read of `stage` is behind us, so step 1 may overwrite it

        // ---- 3. F, and the stores
        if (mine) {
            uint32_t o[kChunk];
#pragma unroll
            for (int i = 0; i < kChunk; ++i) o[i] = tv[i];
            if (mode != 0) {
                uint32_t L[kChunk];
                // the last reading left of the chunk, if the chunk begins with a hole
                int col = kNoLast;
                uint32_t val = 0u;
                if (o[0] == 0u) {
                    for (int k = tid - 1; k >= 0 && x0 - (k * kChunk + kChunk - 1) <= max_gap; --k) {
                        const int l = rec_last[k];
                        if (l != kNoLast) {
                            col = l;
                            val = timg[l];
                            break;
                        }
                    }
                }
#pragma unroll
                for (int i = 0; i < kChunk; ++i) {
                    if (o[i] != 0u) {
                        col = x0 + i;
                        val = o[i];
                    }
                    L[i] = (col != kNoLast && x0 + i - col <= max_gap) ? val : 0u;
                }
                uint32_t Rv[kChunk];
#pragma unroll
                for (int i = 0; i < kChunk; ++i) Rv[i] = 0u;
                if (mode == 2) {
                    col = kNoFirst;
                    val = 0u;
                    if (o[kChunk - 1] == 0u) {
                        for (int k = tid + 1; k < cpr && k * kChunk - (x0 + kChunk - 1) <= max_gap; ++k) {
                            const int r = rec_first[k];
                            if (r != kNoFirst) {
                                col = r;
                                val = timg[r];
                                break;
                            }
                        }
                    }
#pragma unroll
                    for (int i = kChunk - 1; i >= 0; --i) {
                        if (o[i] != 0u) {
                            col = x0 + i;
                            val = o[i];
                        }
                        Rv[i] = (col != kNoFirst && col - (x0 + i) <= max_gap) ? val : 0u;
                    }
                }
#pragma unroll
                for (int i = 0; i < kChunk; ++i) {
                    if (o[i] == 0u) {
                        const uint32_t v = L[i] > Rv[i] ? L[i] : Rv[i];
                        o[i] = v;
                        if (v != 0u) fl[i >> 2] |= 4u << ((i & 3) * 8);
                    }
                }
            }
            uint16_t *out_frame = depth_out + (size_t)f * frame_px;
            uint8_t *flag_frame = flags_out ? flags_out + (size_t)f * frame_px : nullptr;
            if (vec) {
                *reinterpret_cast<uint4 *>(out_frame + at) =
                    make_uint4(o[0] | (o[1] << 16), o[2] | (o[3] << 16), o[4] | (o[5] << 16), o[6] | (o[7] << 16));
                if (flag_frame) *reinterpret_cast<uint2 *>(flag_frame + at) = make_uint2(fl[0], fl[1]);
            } else {
#pragma unroll
                for (int i = 0; i < kChunk; ++i) {
                    if (x0 + i < W) {
                        out_frame[at + i] = (uint16_t)o[i];
                        if (flag_frame) flag_frame[at + i] = (uint8_t)(fl[i >> 2] >> ((i & 3) * 8));
                    }
                }
            }
        }
    }

    if (temporal && mine) {
        uint32_t *p = state + at;
        if (vec) {
            *reinterpret_cast<uint4 *>(p) = make_uint4(st[0], st[1], st[2], st[3]);
            *reinterpret_cast<uint4 *>(p + 4) = make_uint4(st[4], st[5], st[6], st[7]);
        } else {
#pragma unroll
            for (int i = 0; i < kChunk; ++i)
                if (x0 + i < W) p[i] = st[i];
        }
    }
}

inline size_t lds_bytes(int W, int R)
{
    const size_t cpr = ((size_t)W + kChunk - 1) / kChunk, wp = cpr * kChunk;
    return (size_t)(1 + 2 * R) * (wp + 2 * kPad) * 2 + wp * 2 + cpr * 2 * 2;
}

inline bool in_range(int v, int lo, int hi) { return v >= lo && v <= hi; }

}  // namespace

extern "C" {

size_t rdf_depth_filter_state_bytes(int dim_x, int dim_y)
{
    return dim_x < 0 || dim_y < 0 ? 0 : (size_t)4 * (size_t)dim_x * (size_t)dim_y;
}

int rdf_depth_filter(int n, int dim_x, int dim_y, const uint16_t *depth, const RdfDepthFilterConfig *config, uint32_t *state,
                     uint16_t *depth_out, uint8_t *flags_out, void *stream)
{
    if (n < 0 || dim_x < 0 || dim_y < 0) return RDF_ERR_BAD_ARG;
    if (!config) return RDF_ERR_NULL_PTR;
    const RdfDepthFilterConfig cfg = *config;
    if (!in_range(cfg.spatial_radius, 0, 2) || !in_range(cfg.spatial_delta, 0, 65535) || !in_range(cfg.temporal, 0, 1) ||
        !in_range(cfg.temporal_alpha, 0, 256) || !in_range(cfg.temporal_delta, 0, 65535) || !in_range(cfg.persist_need, 0, 9) ||
        !in_range(cfg.persist_span, 1, 8) || !in_range(cfg.fill_mode, 0, 2) || !in_range(cfg.max_gap, 0, 65535))
        return RDF_ERR_BAD_ARG;
    if (n == 0 || dim_x == 0 || dim_y == 0) return RDF_OK;
    if (dim_x > RDF_DEPTH_FILTER_MAX_WIDTH) return RDF_ERR_BAD_ARG;
    const unsigned long long pixels = (unsigned long long)n * (unsigned long long)dim_x * (unsigned long long)dim_y;
    if (pixels >= (1ull << 31)) return RDF_ERR_TOO_LARGE;
    if (!depth || !depth_out || (cfg.temporal && !state)) return RDF_ERR_NULL_PTR;
    if (misaligned(depth, 2) || misaligned(depth_out, 2) || misaligned(state, 4)) return RDF_ERR_BAD_ARG;
    const uintptr_t a = reinterpret_cast<uintptr_t>(depth), b = reinterpret_cast<uintptr_t>(depth_out), bytes = (uintptr_t)pixels * 2;
    if (a < b + bytes && b < a + bytes) return RDF_ERR_BAD_ARG;
    const int vec = dim_x % kChunk == 0 && !misaligned(depth, 16) && !misaligned(depth_out, 16) && !misaligned(state, 16) &&
                    !misaligned(flags_out, 8);
    const dim3 grid((unsigned)dim_y), block(kThreads);
    hipStream_t s = S(stream);
    uint32_t *st = cfg.temporal ? state : nullptr;
    switch (cfg.spatial_radius) {
    case 0: hipLaunchKernelGGL(k_depth_filter<0>, grid, block, lds_bytes(dim_x, 0), s, n, dim_x, dim_y, depth, cfg, st, depth_out, flags_out, vec); break;
    case 1: hipLaunchKernelGGL(k_depth_filter<1>, grid, block, lds_bytes(dim_x, 1), s, n, dim_x, dim_y, depth, cfg, st, depth_out, flags_out, vec); break;
    default: hipLaunchKernelGGL(k_depth_filter<2>, grid, block, lds_bytes(dim_x, 2), s, n, dim_x, dim_y, depth, cfg, st, depth_out, flags_out, vec); break;
    }
    return (int)hipGetLastError();
}

}  // extern "C"
