/*
 * rdf_frontend.h -- C ABI of librdf_frontend.so: the depth front end of 3d-beats on MI355X (gfx950).  From the camera's raw
 * depth frame to the table-free depth frame that the hand grouping takes, and the RANSAC plane fit that calibrates it:
 * the reference's CalibratedPlane (src/calibrated_plane.py, src/cuda/calibrated_plane.cu) and the per-frame chain
 * deproject_points -> transform_points -> filter_points_by_plane -> remove_missing_3d_points_from_depth_image ->
 * gaussian_depth_filter of src/3d_bz.py:163-212 (src/cuda/points_ops.cu:5-36, 63-73, 131-146, 327-373).
 * Also in this library: the note state machine behind the fingertip heights (rdf_hand_state_*), and the depth post-filter that
 * stands in front of rdf_frame_front when the frames come from a stereo camera (rdf_depth_filter).
 *
 * It is a library of its own, next to librdf_hip.so, with its own ABI number and build id.  Conventions are those of
 * rdf_hip.h: every pointer is caller-owned DEVICE memory unless stated; nothing is allocated, freed or synchronised
 * inside a call (all calls can be captured into a graph); launches are asynchronous on `stream` (a hipStream_t, NULL =
 * the default stream); the return value is 0, a negative RDF_ERR_* for rejected arguments, or a positive hipError_t, and
 * rdf_frontend_error_string() names either kind.
 *
 * Arithmetic: fp32, round to nearest, no contraction, in the order written below.  Matrices are float [4][4] ROW-major,
 * p' = M p.  The reference hands numpy's row-major bytes to a glm::mat4 (column-major) and multiplies by its transpose, so
 * its M is the same matrix.  Where the order comes from glm 0.9.9 it is spelled out:
 *   mat4 * vec4   p'_i = (M_i0 * x + M_i1 * y) + (M_i2 * z + M_i3 * w)          (Mul0 + Mul1, Mul2 + Mul3, Add0 + Add1)
 *   dot(v, v)     (v.x * v.x + v.y * v.y) + v.z * v.z
 *   normalize(v)  v * (1.f / sqrtf(dot(v, v)))                                     (inversesqrt = 1 / sqrt)
 *   cross(a, b)   (a.y * b.z - b.y * a.z,  a.z * b.x - b.z * a.x,  a.x * b.y - b.x * a.y)
 * Points are float4 {x, y, z, w}; a point is valid when w == 1.
 */
#ifndef RDF_FRONTEND_H
#define RDF_FRONTEND_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 1: first version.  2: rdf_hand_state_* (the note state machine behind the fingertip heights), RDF_ERR_CAPTURE.
 * rdf_depth_filter and rdf_depth_filter_state_bytes are a pure addition to 2. */
#define RDF_FRONTEND_ABI_VERSION 2

#define RDF_OK 0
#define RDF_ERR_BAD_ARG (-1)
#define RDF_ERR_NULL_PTR (-2)
#define RDF_ERR_TOO_LARGE (-3)
#define RDF_ERR_CAPTURE (-6)     /* `stream` is being captured into a hipGraph and the call may not be recorded */

#define RDF_FRONTEND_MAX_FILTER 41   /* largest Gaussian window (points_ops.py: MAX_FILTER_SIZE) */

/*
 * Plane candidates, one per random draw row (calibrated_plane.cu:51-90).  rand float [G][32], pts float4 [dim_y][dim_x].
 * For candidate i, draw j = 0, 1, ... 31: r = floor(((float)rand[i][j] * (float)dim_x) * (float)dim_y) (two fp32
 * roundings); pts[r] is taken when pts[r].z > 0, until three points P0, P1, P2 are taken.  Then
 *   v0 = normalize((P1 - P0).xyz), v1 = normalize((P2 - P0).xyz), z = normalize(cross(v0, v1)), x = v0,
 *   y = normalize(cross(z, x)),
 *   candidates[i] = | x.x  y.x  z.x  -P0.x |
 *                   | x.y  y.y  z.y  -P0.y |
 *                   | x.z  y.z  z.z  -P0.z |
 *                   | 0    0    0     1    |
 * so z' = M[2,:] . p takes the z components of the three axes, not the normal, exactly as the reference does.
 * A duplicate or collinear draw gives NaN axes, and such a candidate counts 0 inliers, as in the reference.
 * Deviations from the reference:
 *   - a draw with r < 0 or r >= dim_x * dim_y is a miss.  curand's uniform is (0, 1]: 1.0 gives r = dim_x * dim_y, and
 *     the reference then reads past the end of pts;
 *   - a candidate that takes fewer than 3 points is invalid: all 16 entries NaN and counts[i] = -1.  The reference builds
 *     it from uninitialised registers.
 * counts int32 [G] (may be NULL): set to 0 for a valid candidate, -1 for an invalid one, ready for rdf_plane_inliers.
 * start_mat float [16] (may be NULL): written over candidate 0 (valid, count 0), as calibrated_plane.py:62-64 does
 * before counting, so that a new plane must beat it (it wins ties: the lowest index does).
 */
int rdf_make_plane_candidates(int num_candidates, int dim_x, int dim_y, const float *rand, const float *pts,
                              const float *start_mat, float *candidates, int32_t *counts, void *stream);

/*
 * Inlier counts (find_plane_ransac, calibrated_plane.cu:3-27): for every point with w == 1 and every candidate,
 * z' = (M20 * x + M21 * y) + (M22 * z + M23 * w); the point is an inlier when z' < T && z' > -T (|z'| < T, false for NaN).
 * counts[i] += the number of inliers of candidate i.  Counts are integers: the result does not depend on any order.
 * A candidate with no inlier is not touched (an invalid one keeps its -1).  n_pts = dim_x * dim_y in the app.
 */
int rdf_plane_inliers(int num_candidates, float threshold, int n_pts, const float *pts, const float *candidates,
                      int32_t *counts, void *stream);

/* The device record rdf_plane_select writes (112 bytes). */
typedef struct RdfPlaneResult {
    float plane[16];       /* the recentred plane, row-major; a copy of plane_inout after the call */
    int32_t best_index;    /* highest count, lowest index on ties (np.argmax) */
    int32_t best_count;
    double c[4];           /* float64(M) @ [0, 0, t, 1] of the winner */
    int32_t status;        /* RDF_PLANE_OK or RDF_PLANE_NONE */
    int32_t reserved;
} RdfPlaneResult;

#define RDF_PLANE_OK 0
#define RDF_PLANE_NONE 1       /* best count <= 0, or |c[2]| >= 0.001 (the reference's assert): plane_inout untouched */

/*
 * The winner and its recentring (calibrated_plane.py:70-87), one workgroup.  best = np.argmax(counts).  With M the winner,
 * t = (-M23) / M22 in fp32, c = float64(M) @ [0, 0, t, 1] (M_i2 * t + M_i3, exact product, one double rounding), and
 * when |c[2]| < 0.001 and the best count > 0: plane = T(-(float)c[0], -(float)c[1], 0) @ M with the translation in
 * column 3, i.e. M with one fp32 add on each of M[0][3] and M[1][3] (M[0][3] + -(float)c[0]) and rows 2 and 3 unchanged.
 * plane_inout float [16] is written only then; result (may be NULL) always.
 */
int rdf_plane_select(int num_candidates, const float *candidates, const int32_t *counts, float *plane_inout,
                     RdfPlaneResult *result, void *stream);

/*
 * The three in sequence: CalibratedPlane.make without its host read.  workspace: rdf_calibrate_plane_workspace_bytes(G)
 * bytes, 16-byte aligned: candidates float [G][16] at offset 0, then counts int32 [G] (both readable after the call).
 */
size_t rdf_calibrate_plane_workspace_bytes(int num_candidates);
int rdf_calibrate_plane(int num_candidates, float threshold, int dim_x, int dim_y, const float *rand, const float *pts,
                        const float *start_mat, void *workspace, float *plane_inout, RdfPlaneResult *result, void *stream);

/*
 * The per-frame chain of 3d_bz.py:163-212 in one launch.  depth uint16 [n][dim_y][dim_x]; the n frames share M =
 * plane float [16] (device memory, so a plane that rdf_calibrate_plane left on the device feeds it directly).
 * Per pixel with depth d:
 *   d == 0                                   -> 0
 *   p = ((d * (x - ppx)) / f, (d * (y - ppy)) / f, d, 1), with x - ppx and d as float       (points_ops.cu:5-36)
 *   p' = M p (the order above, all four rows)                                              (points_ops.cu:63-73)
 *   w' == 1 && z' > -T                       -> 0                                          (calibrated_plane.cu:31-46)
 *   else w' == 0                             -> 0                                          (points_ops.cu:131-146)
 *   else                                     -> d
 * Then, when gauss is not NULL, the Gaussian filter of that cleaned image (points_ops.cu:327-373): weights float [k][k],
 * k odd, 1 <= k <= 41; for dy then dx, taps outside the frame skipped, w0 += w where the tap is 0, else wn += w and
 * sum += (float)d * w (a multiply, then an add); out = w0 > wn ? 0 : (uint16)(uint32)floor(sum / wn), where the uint32
 * conversion saturates (NaN -> 0, as __float2uint_rd) and the cast keeps the low 16 bits.
 * depth_out uint16 [n][dim_y][dim_x]; may equal depth only when gauss is NULL.
 * pts_out float4 [n][dim_y][dim_x] (may be NULL): p' where d > 0 and the point was not filtered (so also where w' == 0),
 * {0, 0, 0, 0} elsewhere -- what the reference's chain leaves in its points buffer.  The reference leaves a
 * pixel with d == 0 as its points buffer held it from earlier frames (never cleared) and transforms those stale points again
 * every frame; no depth value depends on them.
 */
int rdf_frame_front(const uint16_t *depth, int n, int dim_x, int dim_y, float ppx, float ppy, float f, const float *plane,
                    float threshold, const float *gauss, int k, uint16_t *depth_out, float *pts_out, void *stream);

/*
 * Stand-alone kernels with the reference's semantics, for the drop-in (each a thin launch over the device functions of
 * rdf_frame_front).
 *   deproject_points: pts[i][y][x] = p for d > 0; pixels with d == 0 untouched (as the reference).
 *   transform_points: pts[i] = M pts[i] where pts[i].w == 1; M = plane float [16] in HOST memory (passed by value there).
 *   filter_points_by_plane: pts[i] = 0 where w == 1 and z > -T.
 *   remove_missing_3d_points_from_depth_image: depth[i] = 0 where pts[i].w == 0.
 *   gaussian_depth_filter: one frame; weights in device memory as above; d_out must not be d_in.
 */
int rdf_deproject_points(int n, int dim_x, int dim_y, float ppx, float ppy, float f, const uint16_t *depth, float *pts,
                         void *stream);
int rdf_transform_points(int n_pts, float *pts, const float *plane_host, void *stream);
int rdf_filter_points_by_plane(int n_pts, float threshold, float *pts, void *stream);
int rdf_remove_missing_3d_points_from_depth_image(int n_pts, const float *pts, uint16_t *depth, void *stream);
int rdf_gaussian_depth_filter(int dim_x, int dim_y, int k, const float *gauss, const uint16_t *d_in, uint16_t *d_out,
                              void *stream);

/*
 * ---- Fingertip heights to note events: the reference's FingertipState / HandState (src/hand_state.py:4-75), driven as
 * src/3d_bz.py:496-522 drives them, as a state block in device memory and one kernel behind the heights. ----
 *
 * The state block is a struct of arrays; T = n_tips (1 .. 64), P = num_positions (11 .. 4096).  A host reads all of it
 * with ONE copy of rdf_hand_state_bytes(T, P) bytes.  Offsets in bytes:
 *      0  int32   n_tips
 *      4  int32   num_positions
 *      8  double  z_thresh_offset         the global offset added to every fingertip's threshold
 *     16  uint32  produced                events ever produced (what a step stores into *head)
 *     20  uint32  reserved[3]             0
 *     32  double  z_thresh[T]
 *         double  min_velocity[T]         15 after init
 *         double  max_velocity[T]         150 after init
 *         double  on_last[T]              the "on" run: its last element,
 *         double  on_mid[T]                 and the sum of its elements 1 .. on_count-2, added in arrival order
 *         double  positions[P][T]         a ring per fingertip: slot pos_next[t] holds the oldest height and is written next
 *         int32   midi_note[T]
 *         int32   note_on[T]              0 / 1
 *         int32   velocity_sensitive[T]   0 / 1, 1 after init
 *         int32   on_count[T]             length of the "on" run
 *         int32   steps[T]                frames this fingertip has consumed
 *         int32   pos_next[T]
 * rdf_hand_state_bytes = 32 + T * (8 * (5 + P) + 4 * 6); 0 for T or P outside the ranges above.
 *
 * One step of fingertip t with height z (IEEE float64, no contraction; thr = z_thresh[t] + z_thresh_offset; p[-1] is the
 * height just pushed, p[-2] and p[-3] the two before it):
 *   z is NaN (the pipeline's "reset", 3d_bz.py:512-513): every position := 0, then OFF.
 *   otherwise: positions[pos_next] := z, pos_next := (pos_next + 1) % P; then
 *     z < thr:  v1 = p[-3] - p[-2], v2 = p[-2] - p[-1]; when v1 > min_velocity && v2 > min_velocity:
 *               v = ((v1 + v2) / 2) / (max_velocity - min_velocity); v = 0.4 + v * (1 - 0.4); v > 1 -> 1; not velocity
 *               sensitive -> 1; ON(v).  Otherwise nothing: a note stays on while the finger stays below the threshold.
 *     else:     OFF.
 *     then, when note_on: on_count >= 2 -> on_mid += on_last; on_last = z; on_count += 1.
 *   ON(v) while off:  note_on = 1; event {steps, t, midi_note, (int)(v * 127)} (truncation); the on-run is cleared
 *                     (on_count = 0, on_last = 0, on_mid = 0).
 *   OFF while on:     note_on = 0; event {steps, t, midi_note, -1}; when on_count >= 4: on_z = on_mid / (on_count - 2.),
 *                     and when on_z > 70: z_thresh = (1.0 - 0.1) * z_thresh + 0.1 * on_z; the on-run is cleared.
 *   steps += 1.
 * The one difference from the reference: it sums the on-run with np.sum(on_positions[1:-1]), which adds pairwise with eight
 * accumulators from eight elements on; on_mid adds in arrival order.  z_thresh can differ from the reference's in the last
 * bits (a relative 3e-16 over 3000-frame tap sequences); events and positions do not.  (The reference's positions list holds
 * num_positions entries from the start, so its `len(positions) > 10` is always true for P >= 11.)
 *
 * Events are int32 [4] = {step, tip, note, velocity or -1 for note off}, stored at events[(seq % capacity) * 4] where seq
 * counts every event since init.  Within a frame they are in fingertip order (a ballot and a prefix count over the one
 * wave; no atomics), frames are in order, launches in stream order.  *head (uint32) receives `produced` once per launch,
 * after a system-scope fence that follows the event stores.  events and head are device memory or pinned host memory
 * mapped into the device's address space; a host that reads them waits for the stream first.  When more than `capacity`
 * events arrive between two reads the oldest are overwritten; a reader sees that from head.
 */
#define RDF_HAND_STATE_MAX_TIPS 64
#define RDF_HAND_STATE_MIN_POSITIONS 11
#define RDF_HAND_STATE_MAX_POSITIONS 4096

#define RDF_HAND_STATE_Z_THRESH 0
#define RDF_HAND_STATE_MIN_VELOCITY 1
#define RDF_HAND_STATE_MAX_VELOCITY 2
#define RDF_HAND_STATE_VELOCITY_SENSITIVE 3     /* values[i] != 0 */
#define RDF_HAND_STATE_Z_THRESH_OFFSET 4        /* global: tip_first = 0, n = 1 */

size_t rdf_hand_state_bytes(int n_tips, int num_positions);

/* Writes the whole block: the header, z_thresh and midi_notes from the HOST arrays [n_tips] (copied during the call),
 * z_thresh_offset = 0, the defaults above, everything else 0.  state: 8-byte aligned device memory. */
int rdf_hand_state_init(void *state, int n_tips, int num_positions, const double *z_thresh, const int32_t *midi_notes,
                        void *stream);

/* field[tip_first .. tip_first + n - 1] = values[0 .. n - 1], values a HOST array copied during the call; ordered on
 * `stream` with the steps around it.  RDF_ERR_CAPTURE while `stream` is being captured: a recorded setter would replay
 * the value of the day of the capture. */
int rdf_hand_state_set(void *state, int field, int tip_first, int n, const double *values, void *stream);

/* n_frames >= 1 steps of fingertips tip_first .. tip_first + n - 1 (the others are untouched), heights float64
 * [n_frames][n] in device or mapped pinned host memory, read when the kernel runs.  One workgroup of one wave, one lane
 * per fingertip.  n_frames = F leaves exactly the bytes and events of F calls with n_frames = 1.  A range that does not
 * fit the block's n_tips does nothing.  capacity >= 1.  Can be captured into a graph. */
int rdf_hand_state_step(void *state, const double *heights, int n_frames, int tip_first, int n, int32_t *events,
                        uint32_t *head, uint32_t capacity, void *stream);

/*
 * ---- Depth post-filter: what stands between a stereo camera's raw frames and rdf_frame_front.  Three stages in the order
 * S -> T -> F, each of which can be switched off; integer arithmetic throughout (the reference has no counterpart: these
 * rules are this project's own).  Depth is uint16, 0 = no reading (a "hole"), as rdf_frame_front takes it. ----
 *
 * Rule S, spatial (spatial_radius r in 0 .. 2, 0 = off; spatial_delta in 0 .. 65535 depth units).  A hole stays a hole.  For
 * a reading c: of the (2r+1)^2 window round it, the readings n != 0 that lie inside the frame and have |n - c| <=
 * spatial_delta (the centre is always one of them); s is their sum and k their number; out = (2 s + k) / (2 k), integer
 * division: their mean, rounded half up.
 *
 * Rule T, temporal (temporal in 0 .. 1, 0 = off; temporal_alpha in 0 .. 256, the new reading's weight in 256ths;
 * temporal_delta in 0 .. 65535 depth units; persist_need in 0 .. 9, persist_span in 1 .. 8).  One uint32 of state per pixel:
 * bits 31..8 are v, the filtered value in sixteenths of a depth unit, 0 = none; bits 7..0 are hist, bit j = "the frame j + 1
 * frames ago had a reading".  With c the output of S and c16 = 16 c:
 *   on a reading (c != 0):  nv = (alpha * c16 + (256 - alpha) * v + 128) >> 8  when v != 0 and |c16 - v| <= 16 temporal_delta
 *                           ("blended"), nv = c16 otherwise; out = (nv + 8) >> 4; v' = nv.
 *   on a hole (c == 0):     out = (v + 8) >> 4 when v != 0 and popcount(hist & (2^span - 1)) >= need ("persisted"), else 0;
 *                           v' = v.
 *   then hist' = ((hist << 1) | (c != 0)) & 255, and on a hole with hist' == 0: v' = 0 -- a value is forgotten after eight
 *   frames without a reading.
 * alpha = 256 with need = 9 is the identity.  With T off the state is neither read nor written.
 *
 * Rule F, hole filling, row by row on T's output t (fill_mode 0 = off, 1 = "left", 2 = "farthest"; max_gap in 0 .. 65535
 * columns).  A reading is unchanged.  For a hole at x: L = t[x - k] for the smallest k in 1 .. max_gap with x - k >= 0 and
 * t[x - k] != 0, or 0 when there is none; R the same with x + k <= dim_x - 1.  Mode 1 gives L, mode 2 max(L, R).  Only
 * readings of t are sources, never filled values, and filled values do not enter T's state.
 *
 * flags (uint8 per pixel and frame): bit 0 = T blended, bit 1 = T persisted, bit 2 = F wrote a value other than 0 into a hole.
 *
 * The n frames of a call are consecutive in time: frame i + 1 sees the state frame i left, and the state after the call is
 * what the next call starts from, so the result of a sequence does not depend on how it is cut into calls.
 */
typedef struct RdfDepthFilterConfig {
    int32_t spatial_radius;
    int32_t spatial_delta;
    int32_t temporal;
    int32_t temporal_alpha;
    int32_t temporal_delta;
    int32_t persist_need;
    int32_t persist_span;
    int32_t fill_mode;
    int32_t max_gap;
} RdfDepthFilterConfig;

#define RDF_DEPTH_FILTER_MAX_WIDTH 2048    /* a workgroup holds whole rows */

/* 4 * dim_x * dim_y: one uint32 per pixel, 4-byte aligned.  All zero = no history (the caller resets by zeroing it);
 * 0 for a negative size. */
size_t rdf_depth_filter_state_bytes(int dim_x, int dim_y);

/*
 * depth, depth_out uint16 [n][dim_y][dim_x]; state uint32 [dim_y][dim_x], read at the start of the call and written at its
 * end (may be NULL with T off); flags_out uint8 [n][dim_y][dim_x] or NULL.  config is HOST memory, read during the call and
 * passed to the kernel by value.  ONE launch whatever n is; no synchronous HIP call, nothing read back.
 * RDF_ERR_BAD_ARG: a negative n, dim_x or dim_y; a config field outside its range; dim_x > RDF_DEPTH_FILTER_MAX_WIDTH; a
 * depth or depth_out that is not 2-byte aligned, a state that is not 4-byte aligned; depth_out overlapping depth (a pixel's
 * window reaches into its neighbours' rows).  RDF_ERR_NULL_PTR: config, depth or depth_out NULL, state NULL with T on.
 * RDF_ERR_TOO_LARGE: n * dim_x * dim_y >= 2^31.  n = 0, dim_x = 0 or dim_y = 0 does nothing and returns 0 (after the
 * config's ranges have been checked).
 */
int rdf_depth_filter(int n, int dim_x, int dim_y, const uint16_t *depth, const RdfDepthFilterConfig *config, uint32_t *state,
                     uint16_t *depth_out, uint8_t *flags_out, void *stream);

int rdf_frontend_abi_version(void);
const char *rdf_frontend_build_id(void);
const char *rdf_frontend_error_string(int code);

#ifdef __cplusplus
}
#endif

#endif /* RDF_FRONTEND_H */
