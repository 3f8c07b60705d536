// rdf_kernel_util.hpp -- the small helpers that sources of the three libraries have in common: the 32-bit mix behind every
// hash rule of include/rdf_labels.h, the wave-wide sums and the 64-bit shuffle, the lanes of a wave that share a key, the
// unpacking of eight 16-bit pixels, and the host one-liners of the entry points and their allowance of large dynamic LDS.
// A helper that only one file uses stays in that file; so do constants that mean different things in different files
// (kThreads, kMaxGrid*).
#ifndef RDF_KERNEL_UTIL_HPP
#define RDF_KERNEL_UTIL_HPP

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <mutex>

namespace {

typedef unsigned long long u64;

// Rule H of rdf_hand_scene_render, rule I of rdf_stereo_sense, rules P and K of rdf_pose_fit: one function.  __host__ too:
// pose_fit_hip.hip's kinematics run on the host against the restatement.
__host__ __device__ __forceinline__ uint32_t mix32(uint32_t x)
{
    x ^= x >> 16;
    x *= 0x7feb352du;
    x ^= x >> 15;
    x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}

// the sum over the wave's 64 lanes, in every lane
__device__ __forceinline__ uint32_t wave_sum(uint32_t v)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += (uint32_t)__shfl_xor((int)v, m, 64);
    return v;
}

__device__ __forceinline__ u64 shfl_xor64(u64 v, int m)
{
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, m, 64), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), m, 64);
    return ((u64)hi << 32) | lo;
}

__device__ __forceinline__ u64 wave_sum64(u64 v)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += shfl_xor64(v, m);
    return v;
}

// The lanes of the wave that hold the first pending lane's key.  `pending` is wave-uniform and not zero; `has` says whether
// this lane holds a key at all.  A wave that serves its keys group by group clears `lanes` from `pending` after each.
struct KeyGroup { int src, key; u64 lanes; };   // the first pending lane, its key (both wave-uniform), the lanes that hold it
__device__ __forceinline__ KeyGroup wave_key_group(u64 pending, int key, bool has)
{
    const int src = __ffsll((long long)pending) - 1;
    const int k0 = __builtin_amdgcn_readfirstlane(__shfl(key, src, 64));
    return {src, k0, __ballot(has && key == k0)};
}

// eight uint16 pixels of one 16-byte load
__device__ __forceinline__ void unpack8(const uint4 v, uint32_t out[8])
{
    out[0] = v.x & 0xffffu; out[1] = v.x >> 16;
    out[2] = v.y & 0xffffu; out[3] = v.y >> 16;
    out[4] = v.z & 0xffffu; out[5] = v.z >> 16;
    out[6] = v.w & 0xffffu; out[7] = v.w >> 16;
}

// ---- host ----
inline hipStream_t S(void *s) { return reinterpret_cast<hipStream_t>(s); }
inline unsigned blocks(long long n, int per) { return (unsigned)((n + per - 1) / per); }
inline bool misaligned(const void *p, unsigned a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; }    // a: a power of two
inline bool finite_f(float v) { return __builtin_fabsf(v) <= 3.0e38f; }                                          // false for NaN

// A launch with more than 64 KB of dynamic LDS has to be allowed once per device and kernel: one static instance per kernel.
struct LdsAllowance {
    std::mutex mu;
    u64 allowed = 0;      // bit d: done on device d (a device from 64 on is allowed again at every call)
    // 0, `no_device_code` without a current device, or the hipError_t of a failed attribute call
    int allow(const void *kernel, int bytes, int no_device_code)
    {
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess) return no_device_code;
        std::lock_guard<std::mutex> lock(mu);
        if (dev >= 64 || !((allowed >> dev) & 1ull)) {
            const hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
            if (e != hipSuccess) return (int)e;
            if (dev < 64) allowed |= 1ull << dev;
        }
        return 0;
    }
};

}  // namespace

#endif  // RDF_KERNEL_UTIL_HPP
