// hand_state_hip.hip -- fingertip heights to note events on the device: the reference's FingertipState / HandState
// (src/hand_state.py:4-75) as a state block and one kernel that runs behind the heights, so that a frame ends in note events
// without a host read.  Built into librdf_frontend.so.  The rule, the layout of the state block and the one documented
// difference from the reference (the order of the on-run's sum) are in include/rdf_frontend.h.
//
// The step is one workgroup of one wave, one lane per fingertip.  A fingertip gives at most one event per frame, so a frame's
// events are placed by a ballot and a prefix count of the lanes below: fingertip order, no atomics.  Everything a lane needs
// from frame to frame (its last two heights, the on-run's bookkeeping) lives in registers for the n_frames of a launch and
// is stored back once, which is why n_frames = F and F launches leave the same bytes.  All arithmetic is float64 in the
// order written (-ffp-contract=off).

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/rdf_frontend.h"
#include "rdf_kernel_util.hpp"

namespace {

constexpr int kWave = 64;
constexpr int kInitThreads = 256;
constexpr int kHeaderBytes = 32;
constexpr int kDoubleFields = 5, kIntFields = 6;
static_assert(RDF_HAND_STATE_MAX_TIPS == kWave, "one lane per fingertip");

struct Fields {
    double *z_thresh_offset;
    uint32_t *produced;
    double *z_thresh, *min_velocity, *max_velocity, *on_last, *on_mid, *positions;
    int32_t *midi_note, *note_on, *velocity_sensitive, *on_count, *steps, *pos_next;
};

__host__ __device__ inline size_t state_bytes(int T, int P)
{
    return (size_t)kHeaderBytes + (size_t)T * (8u * (size_t)(kDoubleFields + P) + 4u * kIntFields);
}

__host__ __device__ inline bool dims_ok(int T, int P)
{
    return T >= 1 && T <= RDF_HAND_STATE_MAX_TIPS && P >= RDF_HAND_STATE_MIN_POSITIONS && P <= RDF_HAND_STATE_MAX_POSITIONS;
}

__device__ __forceinline__ Fields fields(uint8_t *s, int T, int P)
{
    Fields f;
    f.z_thresh_offset = reinterpret_cast<double *>(s + 8);
    f.produced = reinterpret_cast<uint32_t *>(s + 16);
    double *d = reinterpret_cast<double *>(s + kHeaderBytes);
    f.z_thresh = d;
    f.min_velocity = d + T;
    f.max_velocity = d + 2 * T;
    f.on_last = d + 3 * T;
    f.on_mid = d + 4 * T;
    f.positions = d + 5 * T;
    int32_t *i = reinterpret_cast<int32_t *>(d + (size_t)(kDoubleFields + P) * T);
    f.midi_note = i;
    f.note_on = i + T;
    f.velocity_sensitive = i + 2 * T;
    f.on_count = i + 3 * T;
    f.steps = i + 4 * T;
    f.pos_next = i + 5 * T;
    return f;
}

struct TipValues {
    double z_thresh[kWave];
    int32_t midi_note[kWave];
};

struct SetValues {
    double v[kWave];
};

__global__ void __launch_bounds__(kInitThreads) k_hand_state_init(uint8_t *state, int T, int P, TipValues tv)
{
    uint32_t *w = reinterpret_cast<uint32_t *>(state);
    const size_t words = state_bytes(T, P) / 4;
    for (size_t i = threadIdx.x; i < words; i += kInitThreads) w[i] = 0u;
    __syncthreads();
    const Fields f = fields(state, T, P);
    if (threadIdx.x == 0) {
        reinterpret_cast<int32_t *>(state)[0] = T;
        reinterpret_cast<int32_t *>(state)[1] = P;
    }
    for (int t = threadIdx.x; t < T; t += kInitThreads) {
        f.z_thresh[t] = tv.z_thresh[t];
        f.min_velocity[t] = 15.;
        f.max_velocity[t] = 150.;
        f.midi_note[t] = tv.midi_note[t];
        f.velocity_sensitive[t] = 1;
    }
}

__global__ void __launch_bounds__(kWave) k_hand_state_set(uint8_t *state, int field, int tip_first, int n, SetValues sv)
{
    const int T = reinterpret_cast<const int32_t *>(state)[0], P = reinterpret_cast<const int32_t *>(state)[1];
    if (!dims_ok(T, P)) return;
    const Fields f = fields(state, T, P);
    const int lane = threadIdx.x;
    if (field == RDF_HAND_STATE_Z_THRESH_OFFSET) {
        if (lane == 0) *f.z_thresh_offset = sv.v[0];
        return;
    }
    if (lane >= n || tip_first + n > T) return;
    const int t = tip_first + lane;
    const double v = sv.v[lane];
    switch (field) {
    case RDF_HAND_STATE_Z_THRESH: f.z_thresh[t] = v; break;
    case RDF_HAND_STATE_MIN_VELOCITY: f.min_velocity[t] = v; break;
    case RDF_HAND_STATE_MAX_VELOCITY: f.max_velocity[t] = v; break;
    case RDF_HAND_STATE_VELOCITY_SENSITIVE: f.velocity_sensitive[t] = v != 0. ? 1 : 0; break;
    default: break;
    }
}

__global__ void __launch_bounds__(kWave) k_hand_state_step(uint8_t *state, const double *__restrict__ heights, int n_frames,
                                                           int tip_first, int n, int32_t *events, uint32_t *head,
                                                           uint32_t capacity)
{
    const int T = reinterpret_cast<const int32_t *>(state)[0], P = reinterpret_cast<const int32_t *>(state)[1];
    if (!dims_ok(T, P) || tip_first < 0 || n < 1 || tip_first + n > T) return;      // (uniform: the whole wave leaves)
    const Fields f = fields(state, T, P);
    const int lane = threadIdx.x;
    const bool active = lane < n;
    const int t = tip_first + (active ? lane : 0);      // (idle lanes read fingertip tip_first and store nothing)
    const double offset = *f.z_thresh_offset;
    uint32_t produced = *f.produced;

    double z_thresh = f.z_thresh[t], on_last = f.on_last[t], on_mid = f.on_mid[t];
    const double min_v = f.min_velocity[t], max_v = f.max_velocity[t];
    const int note = f.midi_note[t];
    const bool sensitive = f.velocity_sensitive[t] != 0;
    bool note_on = f.note_on[t] != 0;
    int on_count = f.on_count[t], steps = f.steps[t], pos_next = f.pos_next[t];
    if ((unsigned)pos_next >= (unsigned)P) pos_next = 0;  // (a block that init never wrote: stay inside it)
    double *pos = f.positions + t;                      // positions[k][t] = pos[k * T]
    double p1 = pos[(size_t)((pos_next + P - 1) % P) * T];     // the newest height,
    double p2 = pos[(size_t)((pos_next + P - 2) % P) * T];     // and the one before it

    for (int fr = 0; fr < n_frames; ++fr) {
        bool emit = false;
        int velocity = -1;
        if (active) {
            const double z = heights[(size_t)fr * n + lane];
            bool off = false;
            if (z != z) {                               // NaN: reset_positions()
                for (int k = 0; k < P; ++k) pos[(size_t)k * T] = 0.;
                p1 = 0.;
                p2 = 0.;
                off = true;
            } else {
                pos[(size_t)pos_next * T] = z;
                pos_next = pos_next + 1 == P ? 0 : pos_next + 1;
                const double v1 = p2 - p1, v2 = p1 - z;
                p2 = p1;
                p1 = z;
                if (z < z_thresh + offset) {
                    if (v1 > min_v && v2 > min_v && !note_on) {
                        double v = ((v1 + v2) / 2.) / (max_v - min_v);
                        v = 0.4 + v * (1. - 0.4);
                        if (v > 1.) v = 1.;
                        if (!sensitive) v = 1.;
                        note_on = true;
                        emit = true;
                        velocity = (int)(v * 127.);
                        on_count = 0;
                        on_last = 0.;
                        on_mid = 0.;
                    }
                } else {
                    off = true;
                }
            }
            if (off && note_on) {
                note_on = false;
                emit = true;
                velocity = -1;
                if (on_count >= 4) {
                    const double on_z = on_mid / ((double)on_count - 2.);
                    if (on_z > 70.) z_thresh = (1.0 - 0.1) * z_thresh + 0.1 * on_z;
                }
                on_count = 0;
                on_last = 0.;
                on_mid = 0.;
            }
            if (note_on) {
                if (on_count >= 2) on_mid += on_last;
                on_last = z;
                on_count += 1;
            }
        }
        const unsigned long long who = __ballot(emit);
        if (emit) {
            const uint32_t seq = produced + (uint32_t)__popcll(who & ((1ull << lane) - 1ull));
            int32_t *e = events + (size_t)(seq % capacity) * 4;
            e[0] = steps;
            e[1] = t;
            e[2] = note;
            e[3] = velocity;
        }
        produced += (uint32_t)__popcll(who);
        if (active) steps += 1;
    }

    if (active) {
        f.z_thresh[t] = z_thresh;
        f.on_last[t] = on_last;
        f.on_mid[t] = on_mid;
        f.note_on[t] = note_on ? 1 : 0;
        f.on_count[t] = on_count;
        f.steps[t] = steps;
        f.pos_next[t] = pos_next;
    }
    // the events first, for whoever reads them (the host, through mapped memory): then the count that announces them
    __threadfence_system();
    if (lane == 0) {
        *f.produced = produced;
        *reinterpret_cast<volatile uint32_t *>(head) = produced;
    }
}

}  // namespace

extern "C" {

size_t rdf_hand_state_bytes(int n_tips, int num_positions)
{
    return dims_ok(n_tips, num_positions) ? state_bytes(n_tips, num_positions) : 0;
}

int rdf_hand_state_init(void *state, int n_tips, int num_positions, const double *z_thresh, const int32_t *midi_notes,
                        void *stream)
{
    if (!dims_ok(n_tips, num_positions)) return RDF_ERR_BAD_ARG;
    if (!state || !z_thresh || !midi_notes) return RDF_ERR_NULL_PTR;
    if (misaligned(state, 8)) return RDF_ERR_BAD_ARG;
    TipValues tv = {};
    for (int t = 0; t < n_tips; ++t) {
        tv.z_thresh[t] = z_thresh[t];
        tv.midi_note[t] = midi_notes[t];
    }
    hipLaunchKernelGGL(k_hand_state_init, dim3(1), dim3(kInitThreads), 0, S(stream), static_cast<uint8_t *>(state), n_tips,
                       num_positions, tv);
    return (int)hipGetLastError();
}

int rdf_hand_state_set(void *state, int field, int tip_first, int n, const double *values, void *stream)
{
    if (field < RDF_HAND_STATE_Z_THRESH || field > RDF_HAND_STATE_Z_THRESH_OFFSET) return RDF_ERR_BAD_ARG;
    if (tip_first < 0 || n < 1 || tip_first + n > RDF_HAND_STATE_MAX_TIPS) return RDF_ERR_BAD_ARG;
    if (field == RDF_HAND_STATE_Z_THRESH_OFFSET && (tip_first != 0 || n != 1)) return RDF_ERR_BAD_ARG;
    if (!state || !values) return RDF_ERR_NULL_PTR;
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (stream && hipStreamIsCapturing(S(stream), &cap) == hipSuccess && cap == hipStreamCaptureStatusActive)
        return RDF_ERR_CAPTURE;
    SetValues sv = {};
    for (int i = 0; i < n; ++i) sv.v[i] = values[i];
    hipLaunchKernelGGL(k_hand_state_set, dim3(1), dim3(kWave), 0, S(stream), static_cast<uint8_t *>(state), field, tip_first,
                       n, sv);
    return (int)hipGetLastError();
}

int rdf_hand_state_step(void *state, const double *heights, int n_frames, int tip_first, int n, int32_t *events,
                        uint32_t *head, uint32_t capacity, void *stream)
{
    if (n_frames < 1 || tip_first < 0 || n < 1 || tip_first + n > RDF_HAND_STATE_MAX_TIPS || capacity < 1)
        return RDF_ERR_BAD_ARG;
    if (!state || !heights || !events || !head) return RDF_ERR_NULL_PTR;
    if ((long long)capacity * 4 >= (1ll << 31)) return RDF_ERR_TOO_LARGE;
    hipLaunchKernelGGL(k_hand_state_step, dim3(1), dim3(kWave), 0, S(stream), static_cast<uint8_t *>(state), heights, n_frames,
                       tip_first, n, events, head, capacity);
    return (int)hipGetLastError();
}

}  // extern "C"
