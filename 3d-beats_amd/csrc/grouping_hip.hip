// grouping_hip.hip -- the app's hand grouping on the device: depth frame -> image at mip level L that says
// which pixels belong to hand 1 and which to hand 2.  Replaces the host round trip of src/3d_bz.py:213-263 (shrink_image,
// synchronise, copy to the host, CppGrouping().make_groups, upload, write_pixel_groups_to_stencil_image, grow_groups) with
// one stream-ordered, capturable call.  The contract (bit-exact to that chain) is spelled out above rdf_hand_groups in
// include/rdf_hip.h; in short: 4-connected components of the nonzero pixels of depth[y*f][x*f], size filter, centroid,
// side by centroid x, largest component per side (ties: smallest raster index), stencil, one grow step.
//
// Components are a union-find over raster indices whose links always point from the larger root to the smaller
// (atomicMin), so every root ends as its component's minimum raster index -- the pixel the reference's raster-order BFS
// meets first, which is what its `size > best` tie-break keeps.  Every sum is an integer atomic and the per-side choice is
// a 64-bit atomicMax over (size << 32 | ~root): results do not depend on the order in which lanes or workgroups run.
//
// Resident path (Hm * Wm <= kResMaxPixels): ONE workgroup of 1024 threads per frame, everything in LDS, one launch.
//   dynamic LDS = parent int32 [P] + per-component stats {count, sum x, sum y} int32 [ceil(P/2)] (a 4-connected grid has
//   at most ceil(P/2) components) = 10 bytes per pixel; the stats area is reused for the uint8 stencil that grow reads.
//   kResMaxPixels = 16000 -> 160 000 B + 152 B static, inside the CU's 160 KiB; the app's 106x60 (63 600 B) and 160x90
//   (144 000 B) frames take it.
// Global path (larger frames, or path = 2): five launches on the caller's stream, scratch in the caller's workspace,
//   no workgroup ever waits for another (phases are ordered by launch boundaries only):
//   1. 16x16 tiles: fused shrink, tile-local union-find in LDS, write each pixel's tile root as a global index; zero stats
//   2. tile borders: union across tile edges in global memory (lock-free atomicMin linking, no waiting)
//   3. compression + per-root stats (global integer atomics, one per wave where the wave's pixels share a root)
//   4. selection: each root that survives the size filter bids atomicMax on its side's key
//   5. stencil + grow + components + g_info, straight from the compressed parents (no stencil buffer)
//   (+ coords: one workgroup per frame scans the groups in raster order)

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/rdf_hip.h"
#include "rdf_kernel_util.hpp"

namespace {

constexpr int kResThreads = 1024;
constexpr int kResWaves = kResThreads / 64;
constexpr int kResMaxPixels = 16000;
constexpr int kTile = 16;
constexpr int kGlThreads = 256;
constexpr int kMaxLevel = 15;

struct Stats {
    int cnt, sx, sy;
};

__host__ __device__ constexpr size_t resident_lds_bytes(int P)
{
    return (size_t)P * 4 + (size_t)((P + 1) / 2) * sizeof(Stats);
}

// grouping.cpp:139 -- `size * 1.f / (dim_x * dim_y) <= pct_thresh` drops the component
__device__ __forceinline__ bool keep_component(int size, int P, float pct) { return !((float)size / (float)P <= pct); }

// grouping.cpp:141-152 -- fp32 centroid x; side 0 (group 1) when c_x < dim_x / 2.f
__device__ __forceinline__ int side_of(int sx, int size, int Wm) { return (float)sx / (float)size < (float)Wm / 2.f ? 0 : 1; }

__device__ __forceinline__ unsigned long long side_key(int size, int root)
{
    return ((unsigned long long)(uint32_t)size << 32) | (uint32_t)~(uint32_t)root;
}
__device__ __forceinline__ int key_root(unsigned long long k) { return k ? (int)~(uint32_t)k : -1; }

// ---- union-find in LDS (one workgroup) ----
__device__ __forceinline__ int lds_find(volatile int *p, int i)
{
    int q = p[i];
    while (q != i) { i = q; q = p[i]; }
    return i;
}

__device__ void lds_union(int *p, int a, int b)
{
    for (;;) {
        a = lds_find(p, a);
        b = lds_find(p, b);
        if (a == b) return;
        if (a > b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(&p[b], a);   // links b under a only while b is still a root
        if (old == b) return;
        b = old;                               // b was linked meanwhile: retry from its new parent
    }
}

// ---- union-find in global memory (many workgroups, one launch; lock-free, nobody waits) ----
__device__ __forceinline__ int gl_load(int *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ __forceinline__ int gl_find(int *p, int i)
{
    int q = gl_load(p + i);
    while (q != i) { i = q; q = gl_load(p + i); }   // parents only ever decrease: terminates
    return i;
}

__device__ void gl_union(int *p, int a, int b)
{
    for (;;) {
        a = gl_find(p, a);
        b = gl_find(p, b);
        if (a == b) return;
        if (a > b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(&p[b], a);
        if (old == b) return;
        b = old;
    }
}

__device__ __forceinline__ int wave_sum(int v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// Adds (1, x, y) of every active lane into st[slot]: one atomic triple per wave when the wave's active lanes share the
// slot (a wave is 64 consecutive pixels of a row: usually one hand or none), per-lane atomics otherwise.  All 64 lanes
// of the wave must call it together.
__device__ __forceinline__ void add_stats(int *cnt, int *sx, int *sy, size_t stride, bool act, int slot, int x, int y)
{
    const unsigned long long m = __ballot(act);
    if (!m) return;
    const int first = __ffsll((long long)m) - 1;
    const int s0 = __shfl(slot, first, 64);
    if (__ballot(act && slot != s0) == 0ull) {
        const int c = wave_sum(act ? 1 : 0), tx = wave_sum(act ? x : 0), ty = wave_sum(act ? y : 0);
        if ((int)(threadIdx.x & 63) == first) {
            atomicAdd(cnt + (size_t)s0 * stride, c);
            atomicAdd(sx + (size_t)s0 * stride, tx);
            atomicAdd(sy + (size_t)s0 * stride, ty);
        }
    } else if (act) {
        atomicAdd(cnt + (size_t)slot * stride, 1);
        atomicAdd(sx + (size_t)slot * stride, x);
        atomicAdd(sy + (size_t)slot * stride, y);
    }
}

// coords_out rows (y, x, group): group 1 first, then group 2, each in raster order (the reference emits BFS order; its only
// consumer scatters the list into an image).  One workgroup walks the frame 1024 pixels at a time: ballot prefix counts
// inside a wave, wave totals through LDS.  n1 = size of group 1.  Rows past n1 + n2 are not written.
template <class G>
__device__ void emit_coords(int P, int Wm, int n1, G group_of, int32_t *coords, int (*s_wtot)[2])
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long below = (1ull << lane) - 1ull;
    int run1 = 0, run2 = n1;
    for (int base = 0; base < P; base += kResThreads) {
        const int i = base + (int)threadIdx.x;
        const int g = i < P ? group_of(i) : 0;
        const unsigned long long m1 = __ballot(g == 1), m2 = __ballot(g == 2);
        if (lane == 0) { s_wtot[wave][0] = __popcll(m1); s_wtot[wave][1] = __popcll(m2); }
        __syncthreads();
        int o1 = 0, o2 = 0, t1 = 0, t2 = 0;
        for (int w = 0; w < kResWaves; ++w) {
            const int a = s_wtot[w][0], b = s_wtot[w][1];
            if (w < wave) { o1 += a; o2 += b; }
            t1 += a; t2 += b;
        }
        if (g) {
            const int row = g == 1 ? run1 + o1 + __popcll(m1 & below) : run2 + o2 + __popcll(m2 & below);
            const int y = i / Wm;
            coords[(size_t)row * 3 + 0] = y;
            coords[(size_t)row * 3 + 1] = i - y * Wm;
            coords[(size_t)row * 3 + 2] = g;
        }
        run1 += t1; run2 += t2;
        __syncthreads();                    // s_wtot is rewritten by the next step
    }
}

// grow_groups (points_ops.cu:407-438): own value if nonzero, else the first nonzero of left, right, up, down
template <class G>
__device__ __forceinline__ uint16_t grown(int i, int x, int y, int Wm, int Hm, G s)
{
    uint32_t g = s(i);
    if (!g && x > 0) g = s(i - 1);
    if (!g && x + 1 < Wm) g = s(i + 1);
    if (!g && y > 0) g = s(i - Wm);
    if (!g && y + 1 < Hm) g = s(i + Wm);
    return (uint16_t)g;
}

__device__ __forceinline__ void write_ginfo(float *gi, int side, int cnt, int sx, int sy)
{
    gi[side * 3 + 0] = (float)cnt;
    gi[side * 3 + 1] = cnt ? (float)sx / (float)cnt : 0.0f;   // empty side: 0 (the reference leaves it uninitialised)
    gi[side * 3 + 2] = cnt ? (float)sy / (float)cnt : 0.0f;
}

// ================================ resident path: one workgroup per frame ================================
__global__ __launch_bounds__(kResThreads) void k_groups_resident(const uint16_t *depth, int W, int H, int L, int Wm, int Hm,
                                                                 float pct, uint16_t *groups, float *ginfo, int32_t *comps,
                                                                 int32_t *coords)
{
    extern __shared__ int s_parent[];
    __shared__ int s_nroots;
    __shared__ unsigned long long s_best[2];
    __shared__ int s_wtot[kResWaves][2];
    const int P = Wm * Hm, tid = threadIdx.x, f = blockIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    Stats *st = reinterpret_cast<Stats *>(s_parent + P);
    uint8_t *sten = reinterpret_cast<uint8_t *>(s_parent + P);   // replaces st once the selection is done
    volatile int *vp = s_parent;
    const uint16_t *dep = depth + (size_t)f * H * W;

    // 1. shrink fused into the load (points_ops.cu:376-403): mm[y][x] = depth[y*f][x*f]; foreground = mm != 0
    for (int i = tid; i < P; i += kResThreads) {
        const int y = i / Wm, x = i - y * Wm;
        s_parent[i] = dep[(size_t)(y << L) * W + (x << L)] ? i : -1;
    }
    for (int i = tid; i < (P + 1) / 2; i += kResThreads) st[i] = Stats{0, 0, 0};
    if (tid == 0) { s_nroots = 0; s_best[0] = 0ull; s_best[1] = 0ull; }
    __syncthreads();

    // 2. 4-connected unions with the left and upper neighbours (grouping.cpp:82-135's DIRS, as a union-find)
    for (int i = tid; i < P; i += kResThreads) {
        if (vp[i] < 0) continue;            // (foreground-ness never changes: a pixel's parent stays >= 0)
        const int y = i / Wm, x = i - y * Wm;
        if (x > 0 && vp[i - 1] >= 0) lds_union(s_parent, i, i - 1);
        if (y > 0 && vp[i - Wm] >= 0) lds_union(s_parent, i, i - Wm);
    }
    __syncthreads();

    // 3. compression: every pixel points at its root, the component's minimum raster index
    for (int i = tid; i < P; i += kResThreads)
        if (vp[i] >= 0) vp[i] = lds_find(vp, i);
    __syncthreads();

    // 4. each root takes a stats slot; its parent entry becomes -2 - slot (background stays -1)
    for (int i = tid; i < P; i += kResThreads)
        if (vp[i] == i) vp[i] = -2 - atomicAdd(&s_nroots, 1);
    __syncthreads();

    // 5. per-component size and coordinate sums (grouping.cpp:141-150), integer LDS atomics
    for (int base = wave * 64; base < P; base += kResThreads) {
        const int i = base + lane;
        const int p = i < P ? vp[i] : -1;
        const bool act = p != -1;
        const int slot = !act ? 0 : p < 0 ? -2 - p : -2 - vp[p];
        const int y = i / Wm;
        add_stats(&st[0].cnt, &st[0].sx, &st[0].sy, 3, act, slot, i - y * Wm, y);
    }
    __syncthreads();

    // 6. size filter, side, largest per side (grouping.cpp:139-165)
    for (int i = tid; i < P; i += kResThreads) {
        const int p = vp[i];
        if (p > -2) continue;
        const Stats c = st[-2 - p];
        if (!keep_component(c.cnt, P, pct)) continue;
        atomicMax(&s_best[side_of(c.sx, c.cnt, Wm)], side_key(c.cnt, i));
    }
    __syncthreads();
    const int r0 = key_root(s_best[0]), r1 = key_root(s_best[1]);
    if (ginfo && tid < 2) {
        const int r = tid ? r1 : r0;
        const Stats c = r >= 0 ? st[-2 - vp[r]] : Stats{0, 0, 0};
        write_ginfo(ginfo + (size_t)f * 6, tid, c.cnt, c.sx, c.sy);
    }
    const int n1 = (int)(s_best[0] >> 32);
    __syncthreads();                        // the stats area becomes the stencil

    // 7. stencil (write_pixel_groups_to_stencil_image): 1 / 2 / 0 by winner membership; components
    for (int i = tid; i < P; i += kResThreads) {
        const int p = vp[i];
        const int root = p >= 0 ? p : p == -1 ? -1 : i;
        sten[i] = root < 0 ? 0 : root == r0 ? 1 : root == r1 ? 2 : 0;
        if (comps) comps[(size_t)f * P + i] = root;
    }
    __syncthreads();

    // 8. grow from the stencil in LDS
    uint16_t *gout = groups + (size_t)f * P;
    const auto s_of = [&](int j) { return (uint32_t)sten[j]; };
    for (int i = tid; i < P; i += kResThreads) {
        const int y = i / Wm, x = i - y * Wm;
        gout[i] = grown(i, x, y, Wm, Hm, s_of);
    }
    if (coords) emit_coords(P, Wm, n1, s_of, coords + (size_t)f * P * 3, s_wtot);
}

// ================================ global path ================================
struct Ws {
    unsigned long long *best;   // [n][2]
    int *parent, *cnt, *sx, *sy;   // [n][P] each
};

__host__ __device__ inline Ws carve(void *ws, int n, size_t P)
{
    char *b = reinterpret_cast<char *>(ws);
    Ws w;
    w.best = reinterpret_cast<unsigned long long *>(b);
    int *q = reinterpret_cast<int *>(b + (size_t)n * 16);
    w.parent = q;
    w.cnt = q + (size_t)n * P;
    w.sx = q + 2 * (size_t)n * P;
    w.sy = q + 3 * (size_t)n * P;
    return w;
}

__global__ __launch_bounds__(kGlThreads) void k_gl_tiles(const uint16_t *depth, int W, int H, int L, int Wm, int Hm, Ws w)
{
    __shared__ int s_p[kTile * kTile];
    const int f = blockIdx.z, tid = threadIdx.x;
    const int lx = tid % kTile, ly = tid / kTile;
    const int gx = blockIdx.x * kTile + lx, gy = blockIdx.y * kTile + ly;
    const bool in = gx < Wm && gy < Hm;
    const size_t P = (size_t)Wm * Hm;
    const bool fg = in && depth[(size_t)f * H * W + (size_t)(gy << L) * W + (gx << L)] != 0;
    s_p[tid] = fg ? tid : -1;
    if (blockIdx.x == 0 && blockIdx.y == 0 && tid < 2) w.best[(size_t)f * 2 + tid] = 0ull;
    __syncthreads();
    if (fg && lx > 0 && s_p[tid - 1] >= 0) lds_union(s_p, tid, tid - 1);
    __syncthreads();                        // (horizontal then vertical: fewer retries on the same roots)
    if (fg && ly > 0 && s_p[tid - kTile] >= 0) lds_union(s_p, tid, tid - kTile);
    __syncthreads();
    if (!in) return;
    const size_t gi = (size_t)f * P + (size_t)gy * Wm + gx;
    int root = -1;
    if (fg) {
        const int r = lds_find(s_p, tid);   // local raster order = global raster order inside a tile
        root = (blockIdx.y * kTile + r / kTile) * Wm + blockIdx.x * kTile + r % kTile;
    }
    w.parent[gi] = root;
    w.cnt[gi] = 0; w.sx[gi] = 0; w.sy[gi] = 0;
}

__global__ __launch_bounds__(kGlThreads) void k_gl_borders(int Wm, int Hm, Ws w)
{
    const int i = blockIdx.x * kGlThreads + threadIdx.x;
    const int P = Wm * Hm;
    if (i >= P) return;
    const int y = i / Wm, x = i - y * Wm;
    const bool left = x > 0 && x % kTile == 0, up = y > 0 && y % kTile == 0;
    if (!left && !up) return;
    int *p = w.parent + (size_t)blockIdx.y * P;
    if (p[i] < 0) return;
    if (left && p[i - 1] >= 0) gl_union(p, i, i - 1);
    if (up && p[i - Wm] >= 0) gl_union(p, i, i - Wm);
}

__global__ __launch_bounds__(kGlThreads) void k_gl_stats(int Wm, int Hm, Ws w)
{
    const int i = blockIdx.x * kGlThreads + threadIdx.x;
    const int P = Wm * Hm;
    const size_t o = (size_t)blockIdx.y * P;
    int *p = w.parent + o;
    const bool act = i < P && p[i] >= 0;
    int root = 0;
    if (act) {
        root = gl_find(p, i);
        p[i] = root;
    }
    const int y = act ? i / Wm : 0;
    add_stats(w.cnt + o, w.sx + o, w.sy + o, 1, act, root, i - y * Wm, y);
}

__global__ __launch_bounds__(kGlThreads) void k_gl_select(int Wm, int Hm, float pct, Ws w)
{
    const int i = blockIdx.x * kGlThreads + threadIdx.x;
    const int P = Wm * Hm;
    if (i >= P) return;
    const size_t o = (size_t)blockIdx.y * P;
    if (w.parent[o + i] != i) return;
    const int c = w.cnt[o + i], sx = w.sx[o + i];
    if (!keep_component(c, P, pct)) return;
    atomicMax(&w.best[(size_t)blockIdx.y * 2 + side_of(sx, c, Wm)], side_key(c, i));
}

__global__ __launch_bounds__(kGlThreads) void k_gl_output(int Wm, int Hm, Ws w, uint16_t *groups, float *ginfo,
                                                          int32_t *comps)
{
    const int i = blockIdx.x * kGlThreads + threadIdx.x;
    const int P = Wm * Hm, f = blockIdx.y;
    const size_t o = (size_t)f * P;
    const int r0 = key_root(w.best[(size_t)f * 2]), r1 = key_root(w.best[(size_t)f * 2 + 1]);
    if (ginfo && i < 2) {
        const int r = i ? r1 : r0;
        write_ginfo(ginfo + (size_t)f * 6, i, r >= 0 ? w.cnt[o + r] : 0, r >= 0 ? w.sx[o + r] : 0, r >= 0 ? w.sy[o + r] : 0);
    }
    if (i >= P) return;
    const int *p = w.parent + o;
    const auto s_of = [&](int j) { const int r = p[j]; return (uint32_t)(r < 0 ? 0 : r == r0 ? 1 : r == r1 ? 2 : 0); };
    const int y = i / Wm, x = i - y * Wm;
    groups[o + i] = grown(i, x, y, Wm, Hm, s_of);
    if (comps) comps[o + i] = p[i];
}

__global__ __launch_bounds__(kResThreads) void k_gl_coords(int Wm, int Hm, Ws w, int32_t *coords)
{
    __shared__ int s_wtot[kResWaves][2];
    const int P = Wm * Hm, f = blockIdx.x;
    const int *p = w.parent + (size_t)f * P;
    const unsigned long long b0 = w.best[(size_t)f * 2], b1 = w.best[(size_t)f * 2 + 1];
    const int r0 = key_root(b0), r1 = key_root(b1);
    const auto s_of = [&](int j) { const int r = p[j]; return (uint32_t)(r < 0 ? 0 : r == r0 ? 1 : r == r1 ? 2 : 0); };
    emit_coords(P, Wm, (int)(b0 >> 32), s_of, coords + (size_t)f * P * 3, s_wtot);
}

} // namespace

extern "C" {

size_t rdf_hand_groups_workspace_bytes(int n, int dim_x, int dim_y, int mipmap_level)
{
    if (n <= 0 || dim_x < 0 || dim_y < 0 || mipmap_level < 0 || mipmap_level > kMaxLevel) return 0;
    const size_t P = (size_t)(dim_x >> mipmap_level) * (size_t)(dim_y >> mipmap_level);
    return (size_t)n * 16 + (size_t)n * P * 16;
}

int rdf_hand_groups(const uint16_t *depth, int n, int dim_x, int dim_y, int mipmap_level, float pct_thresh,
                    uint16_t *groups_out, float *g_info_out, int32_t *components_out, int32_t *coords_out, void *workspace,
                    int path, void *stream)
{
    if (n < 0 || dim_x < 0 || dim_y < 0 || mipmap_level < 0 || mipmap_level > kMaxLevel || path < 0 || path > 2)
        return RDF_ERR_BAD_ARG;
    if (n == 0) return RDF_OK;
    const int Wm = dim_x >> mipmap_level, Hm = dim_y >> mipmap_level;
    const long long P = (long long)Wm * Hm;
    if (P * (long long)(Wm > Hm ? Wm : Hm) >= (1ll << 31)) return RDF_ERR_TOO_LARGE;   // exact int32 coordinate sums
    if (!depth || !groups_out) return RDF_ERR_NULL_PTR;
    const bool fits = P <= kResMaxPixels;
    if (path == 1 && !fits) return RDF_ERR_BAD_ARG;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (path == 1 || (path == 0 && fits)) {
        static LdsAllowance allowed;
        const int rc = allowed.allow(reinterpret_cast<const void *>(k_groups_resident), (int)resident_lds_bytes(kResMaxPixels),
                                     RDF_ERR_NO_DEVICE);
        if (rc != RDF_OK) return rc;
        hipLaunchKernelGGL(k_groups_resident, dim3((unsigned)n), dim3(kResThreads), resident_lds_bytes((int)P), s, depth,
                           dim_x, dim_y, mipmap_level, Wm, Hm, pct_thresh, groups_out, g_info_out, components_out, coords_out);
        return (int)hipGetLastError();
    }
    if (!workspace) return RDF_ERR_NULL_PTR;
    if ((reinterpret_cast<uintptr_t>(workspace) & 7u) != 0) return RDF_ERR_BAD_ARG;
    const Ws w = carve(workspace, n, (size_t)P);
    const dim3 lin((unsigned)((P + kGlThreads - 1) / kGlThreads > 0 ? (P + kGlThreads - 1) / kGlThreads : 1), (unsigned)n);
    hipLaunchKernelGGL(k_gl_tiles, dim3((unsigned)((Wm + kTile - 1) / kTile > 0 ? (Wm + kTile - 1) / kTile : 1),
                                        (unsigned)((Hm + kTile - 1) / kTile > 0 ? (Hm + kTile - 1) / kTile : 1), (unsigned)n),
                       dim3(kGlThreads), 0, s, depth, dim_x, dim_y, mipmap_level, Wm, Hm, w);
    hipLaunchKernelGGL(k_gl_borders, lin, dim3(kGlThreads), 0, s, Wm, Hm, w);
    hipLaunchKernelGGL(k_gl_stats, lin, dim3(kGlThreads), 0, s, Wm, Hm, w);
    hipLaunchKernelGGL(k_gl_select, lin, dim3(kGlThreads), 0, s, Wm, Hm, pct_thresh, w);
    hipLaunchKernelGGL(k_gl_output, lin, dim3(kGlThreads), 0, s, Wm, Hm, w, groups_out, g_info_out, components_out);
    if (coords_out) hipLaunchKernelGGL(k_gl_coords, dim3((unsigned)n), dim3(kResThreads), 0, s, Wm, Hm, w, coords_out);
    return (int)hipGetLastError();
}

} // extern "C"
