/*
 * rdf_labels.h -- C ABI of librdf_labels.so: colour-glove recordings to training labels on MI355X (gfx950).  The kernels
 * behind the reference's src/live_data_convert.py: split_pixels_by_nearest_color, apply_point_mapping and
 * depths_from_points (src/cuda/points_ops.cu:207-255, 167-205, 39-63), the whole of its make_color_mapping
 * (live_data_convert.py:156-204) as device work, and the per-frame labelling of its tick() (:413-458) as one pass.
 * And the converter's augmentation: the centre of a frame's points (rdf_points_center) and the re-render of the moved
 * scene (rdf_rerender), a software rasteriser in place of the reference's OpenGL draw; those two are fp32 / fp64 with a
 * stated operation order, described with their declarations below.
 * And the score of what was trained on those labels: predicted label maps against true ones as a confusion matrix
 * (rdf_score_labels), integer like the colour kernels.
 * And where those labels come from when there is no recording: frames of an articulated, labelled triangle mesh over a table
 * plane (rdf_hand_scene_render), the re-render's rasteriser with many frames per call.
 * And the way back from a labelled depth frame to the hand's pose (rdf_pose_fit): candidates proposed, drawn, priced and
 * selected on the device, the reference's pose_fit.py and cuda/fit_mesh.cu.
 * And what a stereo depth camera makes of those frames (rdf_stereo_sense): a left and a right render through a projected dot
 * pattern, a census transform and a block matcher, integer like the colour kernels.
 * And the leaf refit (rdf_labels_refit_count, rdf_labels_refit_apply): a trained forest's leaf distributions re-estimated
 * from labelled frames, in integer counts.
 * And the pruning of such a forest on those counts (rdf_labels_prune_plan, rdf_labels_prune_apply): subtrees that label held-out
 * frames no better than one leaf are folded into one.
 * And what the forest knows beyond its argmax (rdf_labels_forest_posterior, rdf_labels_confidence_counts): per-pixel class
 * sums, a confidence, a reject option and a reliability histogram.
 *
 * It is a library of its own, next to librdf_hip.so and librdf_frontend.so, with its own ABI number and build id.
 * Conventions are those of rdf_hip.h: every pointer is caller-owned DEVICE memory; nothing is allocated, freed or
 * synchronised inside a call (all calls can be captured into a graph); launches are asynchronous on `stream` (a
 * hipStream_t, NULL = the default stream); the return value is 0, a negative RDF_ERR_* for rejected arguments (nothing is
 * launched then), or a positive hipError_t, and rdf_labels_error_string() names either kind.
 *
 * Images: colour uint8 [dim_y][dim_x][3] (r, g, b), 4-byte aligned (pixels are read four at a time as three dwords);
 * colours / mappings uint8 [K][3].  1 <= K <= RDF_LABELS_MAX_COLORS, 1 <= tries <= RDF_LABELS_MAX_TRIES.
 *
 * Arithmetic of the colour kernels is integer throughout, so every result is independent of the order in which pixels are visited:
 *   skipped pixel    r + g + b == 0.
 *   nearest colour   d(i) = (r - c_i.r)^2 + (g - c_i.g)^2 + (b - c_i.b)^2 (each term <= 65 025, d <= 195 075); colour 0
 *                    first, then a strictly smaller d wins: ties go to the lowest index.  The reference computes d in fp32,
 *                    where these integers and their sums are exact.
 *   sums             per colour: pixels, sum r, sum g, sum b, sum d of the pixels nearest to it.  The reference keeps
 *                    sum d as a double; it is an integer far below 2^53, so the double is exact whatever the order.
 *   update           new colour channel = sum / pixels, truncated (numpy: (sums / count).astype(uint8); the fp64 quotient
 *                    of two integers never rounds up across an integer).  AN EMPTY GROUP BECOMES (0, 0, 0): 0 / 0 is NaN,
 *                    which numpy's cast on x86-64 turns into 0.
 */
#ifndef RDF_LABELS_H
#define RDF_LABELS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/*
 * 1: first version.  The number changes when something declared here is removed or re-typed; a pure addition (as
 * rdf_points_center, rdf_rerender, rdf_hand_scene_render and the pose fit -- rdf_pose_cost, rdf_pose_propose, rdf_pose_select,
 * rdf_pose_fit_workspace_bytes and rdf_pose_fit --, the stereo sensor's three, the leaf refit's three, the forest posterior's two and the pruning's three were) keeps it, since every caller of the older entry points still links and runs.
 * Two builds with the same number are told apart by rdf_labels_build_id().
 */
#define RDF_LABELS_ABI_VERSION 1

#ifndef RDF_OK
#define RDF_OK 0
#define RDF_ERR_BAD_ARG (-1)
#define RDF_ERR_NULL_PTR (-2)
#define RDF_ERR_TOO_LARGE (-3)
#endif

#define RDF_LABELS_MAX_COLORS 16   /* K; the reference uses 3..8 */
#define RDF_LABELS_MAX_TRIES 8     /* COLOR_EM_NUM_TRIES of the reference */

/*
 * One step, with the reference's contract (points_ops.cu:207-255): ADDS onto counts uint64 [K][5] = {pixels, sum r,
 * sum g, sum b, sum d}, where word 4 holds a double (the reference's atomicAdd((double*)p + 4, ...)).  The caller zeroes
 * counts.  Sums are made per wave, then per workgroup in LDS; a workgroup adds each non-zero sum to counts once.
 */
int rdf_split_pixels_by_nearest_color(int dim_x, int dim_y, int num_colors, const uint8_t *colors, const uint8_t *image,
                                      uint64_t *counts, void *stream);

/* Every non-skipped pixel of image becomes its nearest colour, in place (points_ops.cu:167-205). */
int rdf_apply_point_mapping(int dim_x, int dim_y, int num_colors, const uint8_t *colors, uint8_t *image, void *stream);

/*
 * depth uint16 [n_img][dim_y][dim_x], pts float4 [n_img][dim_y][dim_x]: where pts.w > 0, depth = (uint16)pts.z, else
 * depth is untouched (points_ops.cu:59-62).  The conversion is the reference's float -> unsigned short: truncated towards
 * zero and clamped to [0, 65535], NaN -> 0.
 */
int rdf_depths_from_points(int n_img, int dim_x, int dim_y, uint16_t *depth, const float *pts, void *stream);

/* The device record rdf_make_color_mapping writes (80 bytes). */
typedef struct RdfColorMappingResult {
    int32_t best_try;                       /* the first try with the smallest cost */
    int32_t tries;
    double best_cost;
    double cost[RDF_LABELS_MAX_TRIES];      /* of every try; entries >= tries are 0 */
} RdfColorMappingResult;

/*
 * make_color_mapping (live_data_convert.py:156-204) without a host round trip.  image: n_px pixels.  init uint8
 * [tries][K][3]: the starting colours of each try (the reference draws them as np.random.uniform(0, 255, (K, 3))
 * .astype(uint8), once per try).  Each of `iterations` >= 1 passes reads the image ONCE for all tries: per try, the
 * sums above against the try's current colours, then the update.  The cost of a try is the sum d of its LAST pass, that
 * is, measured against the colours before the last update, while its colours are those after it (:189-197).  The best try
 * is the first with the strictly smallest cost (:195).
 * best uint8 [K][3]: the best try's colours.  result (may be NULL): the record above.
 * workspace: rdf_color_mapping_workspace_bytes(tries, K) bytes, 8-byte aligned; after the call it starts with the final
 * colours of every try, uint8 [tries][K][3].  2 * iterations + 1 launches, none of which waits for another workgroup.
 */
size_t rdf_color_mapping_workspace_bytes(int tries, int num_colors);
int rdf_make_color_mapping(int n_px, const uint8_t *image, int tries, int iterations, int num_colors, const uint8_t *init,
                           void *workspace, uint8_t *best, RdfColorMappingResult *result, void *stream);

/*
 * One frame of live_data_convert.py:413-458 in one pass; every input is read once and every output written once.
 *   mask_labels uint16 [dim_y][dim_x] (may be NULL): where mask_labels != mask_label the colour becomes (0, 0, 0) first.
 *   image (in/out): then every non-skipped pixel becomes its nearest mapping colour (as rdf_apply_point_mapping).
 *   labels uint16 [dim_y][dim_x]: i + 1 for the HIGHEST i with mapping[i] equal to the pixel's colour after that, 0 when
 *     there is none.  (The reference overwrites in index order, so of duplicate mapping colours the last wins although
 *     the snap chose the first; and a mapping entry (0, 0, 0) -- an empty group -- labels every black pixel.)
 *   labels_rgba uint8 [dim_y][dim_x][4] (may be NULL): the colour, alpha 255 where any channel is non-zero, else 0.
 *   depth uint16 [dim_y][dim_x] (in/out, may be NULL): 0 -> 65535.
 */
int rdf_label_frame(int dim_x, int dim_y, int num_colors, const uint8_t *mapping, uint8_t *image,
                    const uint16_t *mask_labels, int mask_label, uint16_t *depth, uint16_t *labels, uint8_t *labels_rgba,
                    void *stream);

/*
 * The mask step alone (live_data_convert.py:421): image becomes (0, 0, 0) where mask_labels != mask_label.  The first frame
 * needs it before rdf_make_color_mapping, which the reference runs on the masked image.
 */
int rdf_mask_color_image(int dim_x, int dim_y, uint8_t *image, const uint16_t *mask_labels, int mask_label, void *stream);

/*
 * The four component sums of pts float32 [n_pts][4] (16-byte aligned) as sums double[4] in device memory; the caller
 * divides by sums[3] (live_data_convert.py:363-364, where every point is read back to the host to be summed).
 * fp64 in a fixed two-level order, without float atomics, so the result is the same from run to run: B = min(ceil(n_pts /
 * 256), 1024) workgroups of 256 lanes; lane t of workgroup b adds points b * 256 + t, + B * 256, ... in that order, the
 * workgroup's 256 sums are halved (t += t + 128, t += t + 64, ..., t += t + 1) into its partial; one workgroup then sums
 * the partials the same way (lane t takes partials t, t + 256, ...).  n_pts == 0 gives zeros.
 * workspace: rdf_points_center_workspace_bytes(n_pts) bytes, 8-byte aligned, contents irrelevant before and after.
 */
size_t rdf_points_center_workspace_bytes(int n_pts);
int rdf_points_center(int n_pts, const float *pts, void *workspace, double *sums, void *stream);

/*
 * The re-render of live_data_convert.py:207-282 (rerender_image: make_triangles, std_camera.vert / .frag through OpenGL) as
 * a software rasteriser: the frame's points become a triangle mesh, the mesh is moved by obj_tform and drawn back into a
 * new depth image and a new colour image.  A GL driver's rasteriser cannot be matched bit for bit and is not; the rules
 * below are this library's own, tests/rerender_numpy.py restates them, and the kernels match that bit for bit.
 *
 *   pts float32 [dim_y][dim_x][4] (16-byte aligned), camera space; color uint8 [dim_y][dim_x][3]; obj_tform: 16 floats in
 *   HOST memory, row-major, read during the call (as rdf_transform_points takes its matrix), last row exactly (0, 0, 0, 1);
 *   f > 0, ppx, ppy: the depth camera; 0 < zmin <= zmax: the near and far plane (the converter passes 50 and 50000).
 *   depth_out uint16 [dim_y][dim_x], color_out uint8 [dim_y][dim_x][3] (not the input colour): every pixel is written;
 *   a pixel nothing covers gets depth 0 and colour (0, 0, 0), as after glClear.  dim_x, dim_y <= 32768 (else
 *   RDF_ERR_TOO_LARGE); a matrix that is not affine, f <= 0 or an empty or non-finite depth range is RDF_ERR_BAD_ARG.
 *
 * 1. Mesh (points_ops.cu:77-115).  Quad (x, y), x < dim_x - 1 and y < dim_y - 1, exists iff its four corner points have
 *    w > 0.  It gives triangle 0 = (p00, p01, p10) and triangle 1 = (p01, p10, p11), p01 = point (y, x + 1), p10 = point
 *    (y + 1, x).  Triangle id = 2 * (y * (dim_x - 1) + x) + k: fixed, where the reference draws them in the order of an
 *    atomic counter.  No index buffer is written.
 * 2. Vertex (std_camera.vert).  p' = M (x, y, z, 1) in fp32, each of the three rows as ((m0 * x + m1 * y) + m2 * z) + m3,
 *    every operation rounded (no fused multiply-add).  A triangle with a vertex whose z' is not > 0 is dropped (GL would
 *    clip a triangle that crosses the near plane; this does not).
 * 3. Projection (util.rs_projection, reduced to what reaches the viewport).  sx = (f * x') / z' + ppx, sy = (f * y') / z' +
 *    ppy, snapped to 1/256 pixel: X = (integer) floor(sx * 256 + 0.5), Y likewise.  A triangle with a vertex whose |X| or
 *    |Y| exceeds 2^20 (or is NaN) is dropped.  Pixel (i, j) is sampled at (256 i + 128, 256 j + 128).  So a vertex
 *    deprojected from pixel x (which deproject_points places at sx = x) sits on that pixel's top-left corner, half a pixel
 *    from its centre, exactly as in the reference: THE IDENTITY TRANSFORM RESAMPLES THE FRAME BY HALF A PIXEL AND LOSES ITS
 *    LAST ROW AND COLUMN.
 * 4. Coverage.  Integer arithmetic (int64).  E(A, B, P) = (B.X - A.X) * (P.Y - A.Y) - (B.Y - A.Y) * (P.X - A.X); area =
 *    E(V0, V1, V2), a triangle of area 0 is dropped, sgn = the area's sign: both windings are drawn (GL's default, no
 *    culling).  e0 = sgn * E(V1, V2, P), e1 = sgn * E(V2, V0, P), e2 = sgn * E(V0, V1, P).  P is covered iff every e_k > 0,
 *    or e_k == 0 on a top or left edge: with D = sgn * (B - A) the edge's direction, D.Y < 0 (left) or D.Y == 0 and D.X > 0
 *    (top).  A pixel centre on an edge shared by two triangles belongs to exactly one of them.
 * 5. Attributes, perspective-correct as GL interpolates v_depth and v_color: w_k = e_k as fp32 (round to nearest even),
 *    q_k = w_k / z'_k, s = (q0 + q1) + q2, z = ((w0 + w1) + w2) / s, channel c = ((q0 * c0 + q1 * c1) + q2 * c2) / s stored
 *    as min(255, floor(c + 0.5)).  A fragment whose z is not within [zmin, zmax] is discarded.  Depth is stored as z
 *    truncated to uint16 (std_camera.frag:20), 65535 at most.
 * 6. Depth test.  A pixel keeps the fragment with the smallest 64-bit key (bits(z) << 32) | triangle id: the nearest one
 *    (z > 0, so the bit pattern orders as the value), ties to the lowest id.  An integer minimum does not depend on the
 *    order in which fragments arrive.
 *
 * workspace: rdf_rerender_workspace_bytes(dim_x, dim_y) bytes (one key per pixel), 8-byte aligned.  EVERY BYTE MUST BE
 * 0xFF BEFORE THE FIRST CALL (the empty key); each call leaves it so, so one fill serves every later frame of that size.
 * Two launches: one lane per quad sets up its two triangles, walks their bounding boxes clipped to the frame and takes the
 * 64-bit atomic minimum per covered pixel; then one lane per pixel recomputes the winner's attributes from its id, writes
 * depth and colour and resets the key.  The first launch costs time in proportion to the summed bounding boxes: a
 * transform that blows one triangle up to the whole frame makes every lane of that workgroup walk the frame.
 */
size_t rdf_rerender_workspace_bytes(int dim_x, int dim_y);
int rdf_rerender(int dim_x, int dim_y, const float *pts, const uint8_t *color, const float *obj_tform_host, float f,
                 float ppx, float ppy, float zmin, float zmax, void *workspace, uint16_t *depth_out, uint8_t *color_out,
                 void *stream);

/*
 * Score predicted label maps against truth label maps: the confusion matrix and the two sums of the reference's `pct.
 * matching pixels` (train_model.py:104-107, 131-135, test_on_saved_model.py: np.sum(got == truth) / np.sum(truth > 0)) in
 * one pass, with nothing but the counts to read back.  tests/score_numpy.py restates it.
 *   pred   uint16 [n_img][dim_y / r][dim_x / r], r = labels_reduce >= 1 (integer division, as the forest's label maps);
 *   truth  uint16 [n_img][dim_y][dim_x], sampled at (x * r, y * r) for label pixel (x, y).
 *   Both need 2-byte alignment only (callers pass image slices).
 * With C = num_classes (1..RDF_SCORE_MAX_CLASSES), clamp(v) = min(v, C): index C stands for "none or unknown", which takes
 * the 65535 pre-fill and every id the model does not have.  For every label pixel, with p and t the raw 16-bit values:
 *   counts[clamp(t) * (C + 1) + clamp(p)] += 1          the confusion matrix, truth by prediction;
 *   counts[(C + 1)^2 + 0] += (p == t)                   the reference's numerator, raw values: a (0, 0) pixel counts;
 *   counts[(C + 1)^2 + 1] += (t > 0)                    the reference's denominator.
 * counts uint64 [(C + 1)^2 + 2] (rdf_score_counts_bytes(C) bytes, 0 for a rejected C), 8-byte aligned: the call ADDS, the
 * caller zeroes (as rdf_split_pixels_by_nearest_color).  The matrix cells of one call sum to n_img * (dim_y / r) * (dim_x / r):
 * no pixel is dropped.  per_image (may be NULL) uint32 [n_img][2] = {equal, labelled} of each image, ADDS likewise.
 * Rejected arguments leave counts untouched: C outside 1..64, r < 1, a negative dimension or a misaligned pointer is
 * RDF_ERR_BAD_ARG; zero label pixels is a successful no-op; else a NULL pred, truth or counts is RDF_ERR_NULL_PTR and
 * n_img * dim_y * dim_x >= 2^31 RDF_ERR_TOO_LARGE (callers split the batch by images).
 * One launch.  Counts are summed in registers and in 32-bit LDS histograms (a workgroup sees < 2^31 pixels) and each
 * workgroup adds its non-zero cells to counts once, with 64-bit integer atomics: the result does not depend on the order of
 * arrival and is the same from run to run.
 */
#define RDF_SCORE_MAX_CLASSES 64
size_t rdf_score_counts_bytes(int num_classes);
int rdf_score_labels(int n_img, int dim_x, int dim_y, int labels_reduce, int num_classes, const uint16_t *pred,
                     const uint16_t *truth, uint64_t *counts, uint32_t *per_image, void *stream);

/*
 * Labelled depth frames of an articulated triangle mesh over a table plane, n_frames per call: the package's own source of
 * training sets (hand_model.py, hand_scene.py) where the reference renders a rigged hand in Blender (datagen/).  The same
 * software rasteriser as rdf_rerender with per-triangle labels in place of interpolated colours; tests/hand_scene_numpy.py
 * restates the rules below and the kernels match it bit for bit.
 *
 *   verts float32 [n_verts][3], model space; vert_part int32 [n_verts]: the part each vertex belongs to;
 *   tris int32 [n_tris][3]: vertex indices; tri_label uint16 [n_tris];
 *   part_tforms float32 [n_frames][n_parts][12]: rows 0..2 of an affine 4x4, row-major, model space -> camera space;
 *   table float32 [n_frames][4] = (nx, ny, nz, d), the plane n . P = d in camera space; NULL: no table;
 *   f > 0, ppx, ppy, 0 < zmin <= zmax as for rdf_rerender; empty_depth: what a pixel that shows nothing gets, 0 for a raw
 *   camera frame, 65535 for a dataset frame; seed, hole_threshold, noise_amp: rule H;
 *   depth_out, labels_out uint16 [n_frames][dim_y][dim_x] (two different buffers): every pixel of both is written.
 * Every pointer is device memory.  n_frames < 1, a negative count or dimension, f <= 0, an empty or non-finite depth range,
 * noise_amp outside [0, 32767] or a misaligned pointer is RDF_ERR_BAD_ARG; dim_x or dim_y above 32768, or 2^39 pixels and
 * more in the batch, RDF_ERR_TOO_LARGE; zero pixels is a successful no-op; else a NULL workspace or output, or with
 * n_tris > 0 a NULL mesh array or part_tforms, is RDF_ERR_NULL_PTR.  Pixel indices are 64-bit.
 *
 * V. Vertex.  Vertex v of frame n is moved by M = part_tforms[n][vert_part[v]] exactly as rule 2 of rdf_rerender moves a
 *    point: each row as ((m0 * x + m1 * y) + m2 * z) + m3 in fp32, every operation rounded, no fused multiply-add.  A
 *    triangle with a vertex index outside [0, n_verts), or a vertex whose part is outside [0, n_parts), is dropped without
 *    that index being followed; so is one with a vertex whose z' is not > 0.
 * 3, 4. Projection, snapping to 1/256 pixel, the |X|, |Y| <= 2^20 drop, coverage with both windings and the top-left fill
 *    rule, pixel (i, j) sampled at (256 i + 128, 256 j + 128): rules 3 and 4 of rdf_rerender, unchanged.
 * 5. Depth.  Rule 5's z = ((w0 + w1) + w2) / ((w0 / z'0 + w1 / z'1) + w2 / z'2), discarded unless zmin <= z <= zmax.  Nothing
 *    else is interpolated: the label of a fragment of triangle t is tri_label[t].
 * 6. Depth test.  Rule 6 with the key (bits(z) << 32) | t, t the triangle's index in tris: nearest first, then the lowest
 *    index.  Every frame has its own plane of keys.
 * T. Table.  Where table is not NULL, pixel (i, j) of frame n looks along rx = ((i + 0.5f) - ppx) / f, ry = ((j + 0.5f) -
 *    ppy) / f; t = (nx * rx + ny * ry) + nz; if t > 0 and zt = d / t lies within [zmin, zmax] the table is at depth zt there,
 *    else there is no table at that pixel.  All fp32, in that order.  The pixel shows the mesh fragment that won rule 6 if
 *    there is one and (there is no table there or z <= zt), else the table with label 0, else nothing.
 * E. Stored values.  Depth is z (or zt) truncated to uint16, 65535 at most.  A pixel that shows nothing gets empty_depth
 *    and label 0.
 * H. Holes and noise, integer, from a counter-based hash: no generator state, so a pixel's value depends on nothing but
 *    (seed, n, p) with p = j * dim_x + i (< 2^30).  All arithmetic is uint32, wrapping:
 *        mix(x):  x ^= x >> 16;  x *= 0x7feb352d;  x ^= x >> 15;  x *= 0x846ca68b;  x ^= x >> 16;
 *        hash  = mix(mix(seed + n * 0x9e3779b9) ^ p)          hash' = mix(hash ^ 0x85ebca6b)
 *    (frame n under seed s is frame 0 under seed s + n * 0x9e3779b9: a batch can be split into calls).  Only a pixel that
 *    shows mesh or table is touched.  If hole_threshold != 0 and hash < hole_threshold it shows nothing instead
 *    (empty_depth, label 0).  Else, if noise_amp > 0, its stored depth d becomes d + (hash' % (2 * noise_amp + 1)) -
 *    noise_amp, clamped to [1, 65534].  With both zero the image is the clean render.
 *
 * workspace: rdf_hand_scene_workspace_bytes(n_frames, dim_x, dim_y) bytes (one key per pixel and frame; 0 for rejected
 * arguments), 8-byte aligned.  EVERY BYTE MUST BE 0xFF BEFORE THE FIRST CALL; each call leaves it so.  A workspace for more
 * frames serves a call with fewer.  Two launches, neither of which waits for another workgroup: eight lanes per (frame,
 * triangle) move its three vertices, share the rows of its bounding box clipped to the frame and take the 64-bit atomic
 * minimum per covered pixel; one lane per pixel then reads z and the triangle out of the key itself, applies rules T, E and H, writes
 * both images and resets the key.  As for rdf_rerender the first launch costs time in proportion to the summed bounding
 * boxes, which is why the table is analytic and not two frame-sized triangles.
 */
size_t rdf_hand_scene_workspace_bytes(int n_frames, int dim_x, int dim_y);
int rdf_hand_scene_render(int n_frames, int dim_x, int dim_y, int n_verts, const float *verts, const int32_t *vert_part,
                          int n_tris, const int32_t *tris, const uint16_t *tri_label, int n_parts, const float *part_tforms,
                          const float *table, float f, float ppx, float ppy, float zmin, float zmax, uint16_t empty_depth,
                          uint32_t seed, uint32_t hole_threshold, int noise_amp, void *workspace, uint16_t *depth_out,
                          uint16_t *labels_out, void *stream);

/*
 * The pose fit: the hand of hand_model.py fitted to an observed depth frame and its forest labels, on the device.  The
 * reference's pose_fit.py with cuda/fit_mesh.cu (calc_image_cost) renders one candidate cylinder per GUI frame through
 * OpenGL, prices it against the frame and keeps a random perturbation whenever the price drops.  Here a generation is K
 * candidate poses of the whole hand: proposed (rules P and K), drawn by rdf_hand_scene_render, priced (rule C) and selected
 * (rule S) in five launches with nothing read back; tests/pose_fit_numpy.py restates the rules and the kernels match it bit
 * for bit.  A pose is the float64 [26] of hand_model.py: wrist x, y, z; yaw, pitch, roll; per finger (thumb to pinky) a
 * spread and three flexions.
 *
 * C. The cost of a candidate (rdf_pose_cost).  depth uint16 [dim_y][dim_x] and labels uint16 [Hl][Wl], Hl = dim_y / r,
 *    Wl = dim_x / r, r = labels_reduce >= 1, are the observed frame; the observed label of depth pixel (x, y) is
 *    labels[min(y / r, Hl - 1)][min(x / r, Wl - 1)].  The window (x0, y0, ww, wh), ww, wh >= 1, lies inside the frame.
 *    cand_depth, cand_labels uint16 [K][wh][ww] are the K candidates as rendered at window size: rendered pixel (i, j) sits
 *    over observed pixel (x0 + i, y0 + j), and a rendered depth of 0 means that nothing is drawn there.  An observed label l
 *    is "hand" iff l < 64 and bit l of target_mask is set.  Per pixel, d0 and l0 observed, d1 and l1 rendered:
 *      d0 == 0                    nothing: missing data is free (fit_mesh.cu:30);
 *      hand(l0) and d1 == 0       missing += 1;
 *      not hand(l0) and d1 != 0   extra += 1 (the reference's second test falls through to a third that cannot hold);
 *      hand(l0) and d1 != 0       sq += (d0 - d1)^2 and, if l1 != l0, label += 1.
 *    terms uint64 [K][4] = {missing, extra, label, sq}, 8-byte aligned: the call ADDS, the caller zeroes (as
 *    rdf_score_labels).  Every sum is an integer: the result does not depend on the order of arrival.
 *    cost = w_boundary * (missing + extra) + w_label * label + sq in uint64 (weights are uint32; it cannot wrap for a window
 *    of fewer than 2^28 pixels).  With w_label = 0 and one bit in the mask, cost(w_boundary = 10000) is 100 times the
 *    reference's float 100 * mismatches + 0.01 * diff^2, whose own float32 atomic sum depends on arrival order.
 *    One launch, (chunks of the window) x K workgroups: a candidate's image is one contiguous run, read eight pixels per
 *    16-byte load between its first and last 16-byte boundary, one pixel per lane outside; the observed pixels under them
 *    are re-read from cache by all K candidates.  Counters are 32-bit and sq 64-bit in registers, summed per wave, then
 *    per workgroup in LDS; a workgroup adds its non-zero sums to terms once, with 64-bit integer atomics.
 *    K outside 1..RDF_POSE_MAX_CANDIDATES, r < 1, a negative dimension, an empty window or one that leaves the frame, or a
 *    misaligned pointer is RDF_ERR_BAD_ARG; else a NULL pointer RDF_ERR_NULL_PTR; dim_x or dim_y above 32768
 *    RDF_ERR_TOO_LARGE.  Rejected arguments leave terms untouched.
 *
 * The fit's device state (RdfPoseFitState, 256 bytes, 8-byte aligned) holds the incumbent pose, its cost and terms, the
 * generation counter g and the number of accepted candidates.  What does not change during a fit is an RdfPoseFitConfig in
 * HOST memory, read during the call (as rdf_rerender reads its matrix): it is checked on the host and handed to the kernels
 * by value.  sigma >= 0, lo <= hi, all finite; every angle's range (pose numbers 3..25) lies within [-pi, pi], pi the
 * nearest double; cam_from_plane: rows 0..2 of the affine plane space -> camera space matrix, row-major (the inverse of the
 * table plane's matrix); geometry [5][6]: per finger its base x, base y (depth units), rest splay (radians) and three
 * phalanx lengths (depth units); f, ppx, ppy, zmin, zmax as for rdf_hand_scene_render, of the whole frame; anneal_every >= 1.
 * Anything else is RDF_ERR_BAD_ARG.
 *
 * P. Proposals (rdf_pose_propose).  With mix of rule H, all hashing uint32 and wrapping, candidate k of generation g:
 *      h = mix(mix(seed + g * 0x9e3779b9) ^ k);  group = h & 7:  0 wrist x, y, z;  1 yaw, pitch, roll;  2..6 one finger's
 *      spread and three flexions, thumb to pinky;  7 all 26.  For pose number j of the group:
 *      a = mix(h ^ ((2 j + 1) * 0x85ebca6b)),  b = mix(a ^ 0xc2b2ae35),
 *      n = (double)((a & 0xffff) + (a >> 16) + (b & 0xffff) + (b >> 16) - 131070) / 65536       exact, within (-2, 2),
 *      scale = 2^-min(g / anneal_every, 1022)                                                      integer division,
 *      v = inc[j] + (sigma[j] * scale) * n;   p[j] = v < lo[j] ? lo[j] : v > hi[j] ? hi[j] : v
 *    where inc is the incumbent; every operation is one rounded fp64 operation.  Numbers outside the group are copied.
 *    fresh_first != 0 marks the first generation of a fresh fit: it is generation 0 whatever g the state holds, and its
 *    candidate 0 is the incumbent itself, unperturbed and unclamped, which prices the starting pose against a new frame.
 *    poses float64 [K][26] receives the candidates; terms (may be NULL) uint64 [K][4] is zeroed by the same launch.
 * K. Kinematics, in the same launch: part_tforms float32 [K][16][12] of the candidates, what rdf_hand_scene_render takes.
 *    An affine matrix is 12 doubles, rows 0..2 row-major.  The product C = A B is, for every row i and column j,
 *      C[i][j] = (A[i][0] * B[0][j] + A[i][1] * B[1][j]) + A[i][2] * B[2][j],   + A[i][3] after that for j = 3,
 *    with every entry taking part, zeros included.  T(v) is the shift by v; Rx(a), Ry(a), Rz(a) are the rotations of
 *    hand_model.py, e.g. Rz(a) = [c -s 0; s c 0; 0 0 1] with (s, c) = sincos(a) below.
 *      B = cam_from_plane (((T(p[0..2]) Rz(p[3])) Rx(p[4])) Ry(p[5]))           the palm, part 0, is B itself;
 *      finger f: M = T(base x, base y, 0) Rz(rest splay + p[6 + 4 f]);  phalanx 0: M = M Rx(-p[7 + 4 f]);  phalanx q = 1, 2:
 *      M = (M T(0, length[q - 1], 0)) Rx(-p[7 + 4 f + q]);  part 1 + 3 f + q is B M', M' = M, or with `mirrored` M with the
 *      entries [0][1], [0][2], [1][0], [2][0] and [0][3] negated (the conjugate by diag(-1, 1, 1)).
 *    All in fp64, each entry cast to fp32 once (round to nearest even).
 *    sincos(x), no library call: if not |x| <= 2^20 both are NaN; else k = rint(x * 0x1.45f306dc9c883p-1) (ties to even),
 *      r = (x - k * 0x1.921fb544p+0) - k * 0x1.0b4611a626331p-34,  z = r * r,
 *      S = r + (r * z) * (S1 + z * (S2 + z * (S3 + z * (S4 + z * (S5 + z * S6))))),
 *      C = 1 + z * (-0.5 + z * (C1 + z * (C2 + z * (C3 + z * (C4 + z * (C5 + z * C6)))))),
 *      (sin, cos) = (S, C), (C, -S), (-S, -C), (-C, S) for k mod 4 = 0, 1, 2, 3 (k as a two's complement integer);
 *      S1..S6 = -0x1.5555555555549p-3, 0x1.111111110f8a6p-7, -0x1.a01a019c161d5p-13, 0x1.71de357b1fe7dp-19,
 *               -0x1.ae5e68a2b9cebp-26, 0x1.5d93a5acfd57cp-33;
 *      C1..C6 = 0x1.555555555554cp-5, -0x1.6c16c16c15177p-10, 0x1.a01a019cb159p-16, -0x1.27e4f809c52adp-22,
 *               0x1.1ee9ebdb4b1c4p-29, -0x1.8fae9be8838d4p-37    (the coefficients of fdlibm's kernels on [-pi/4, pi/4]).
 *    Every step is one rounded fp64 operation; the library is built without contraction.
 * S. Selection (rdf_pose_select, one wave).  cost_k from terms[k] as in rule C; the best candidate has the lowest cost and
 *    the lowest k among equals.  It replaces the incumbent (pose, cost, terms) iff its cost is strictly lower than the
 *    incumbent's, or unconditionally when fresh_first != 0.  Then g += 1 and accepted += 1 on a replacement; with
 *    fresh_first != 0 they become g = 1, accepted = 1: a fresh fit counts from its own start.  The incumbent's cost after
 *    that is stored to *history_slot when that is not NULL.
 *
 * rdf_pose_fit enqueues `generations` generations on the stream: propose (which zeroes the terms), rdf_hand_scene_render of
 * the K candidates at window size with intrinsics (f, ppx - x0, ppy - y0) in fp32, no table, empty_depth 0, no holes, no
 * noise, then cost, then select; fresh != 0 makes the first of them a fresh first generation.  history (may be NULL) uint64
 * [generations] receives the incumbent's cost after each.  No host read, no synchronisation, no allocation.  Because g
 * lives in the state, a fit of a generations followed by one of b with fresh == 0 is a fit of a + b.  depth, labels: the
 * observed frame of rule C; the mesh arguments are rdf_hand_scene_render's, with 16 parts.
 * workspace: rdf_pose_fit_workspace_bytes(K, ww, wh) bytes (0 for rejected arguments), 16-byte aligned: the renderer's key
 * planes first (rdf_hand_scene_workspace_bytes(K, ww, wh) bytes, EVERY BYTE 0xFF BEFORE THE FIRST CALL, left so by every
 * call; filling the whole workspace with 0xFF is fine), then the candidates' images, transforms, poses and terms.
 * Rejected calls leave the state untouched: a negative generations or a config that breaks the rules above is
 * RDF_ERR_BAD_ARG, as is a misaligned pointer or a window outside the frame; generations == 0 is a successful no-op; else a
 * NULL pointer is RDF_ERR_NULL_PTR and a dimension above 32768 RDF_ERR_TOO_LARGE.
 */
#define RDF_POSE_SIZE 26
#define RDF_POSE_MAX_CANDIDATES 4096

typedef struct RdfPoseFitState {
    double pose[RDF_POSE_SIZE];     /* the incumbent */
    uint64_t cost;
    uint64_t terms[4];              /* missing, extra, label, sq */
    uint32_t generation;            /* g */
    uint32_t accepted;
} RdfPoseFitState;

typedef struct RdfPoseFitConfig {
    int32_t candidates;             /* K */
    int32_t mirrored;
    int32_t anneal_every;
    uint32_t seed;
    int32_t x0, y0, ww, wh;         /* the window */
    uint32_t w_boundary, w_label;
    uint64_t target_mask;
    float f, ppx, ppy, zmin, zmax;
    float reserved;                 /* 0 */
    double sigma[RDF_POSE_SIZE], lo[RDF_POSE_SIZE], hi[RDF_POSE_SIZE];
    double cam_from_plane[12];
    double geometry[30];
} RdfPoseFitConfig;

int rdf_pose_cost(int dim_x, int dim_y, const uint16_t *depth, const uint16_t *labels, int labels_reduce, int x0, int y0,
                  int ww, int wh, int candidates, const uint16_t *cand_depth, const uint16_t *cand_labels,
                  uint64_t target_mask, uint64_t *terms, void *stream);
int rdf_pose_propose(const RdfPoseFitConfig *config_host, const RdfPoseFitState *state, int fresh_first, double *poses,
                     float *part_tforms, uint64_t *terms, void *stream);
int rdf_pose_select(int candidates, const uint64_t *terms, const double *poses, uint32_t w_boundary, uint32_t w_label,
                    int fresh_first, RdfPoseFitState *state, uint64_t *history_slot, void *stream);
size_t rdf_pose_fit_workspace_bytes(int candidates, int ww, int wh);
int rdf_pose_fit(int generations, int fresh, const RdfPoseFitConfig *config_host, RdfPoseFitState *state, int dim_x,
                 int dim_y, const uint16_t *depth, const uint16_t *labels, int labels_reduce, int n_verts,
                 const float *verts, const int32_t *vert_part, int n_tris, const int32_t *tris, const uint16_t *tri_label,
                 void *workspace, uint64_t *history, void *stream);

/*
 * The stereo depth sensor: a clean left-camera render and a clean right-camera render of one scene become the depth frame
 * an active stereo camera (a projected IR dot pattern, two IR imagers, a census block matcher) would report, n_frames per
 * call.  It stands behind rdf_hand_scene_render in place of rule H: the holes and errors are those of matching -- a shadow
 * of missing depth left of whatever stands in front of the table, foreground depth fattened round a silhouette, depth in
 * steps that grow with Z^2, and no depth where there is no texture.  The reference's datagen/stereo_alg.py runs OpenCV's
 * StereoSGBM on two Blender renders for this; nothing of that matcher is restated, the rules below are this library's own.
 * Integer arithmetic throughout; tests/stereo_numpy.py restates the rules and the kernels match it bit for bit.
 *
 *   depth_l, labels_l, depth_r uint16 [n_frames][dim_y][dim_x]: the clean renders, depth_r from a camera moved by the
 *   baseline along +x, labels_l the truth labels of the left frame.  A pixel shows a surface iff 0 < Z < 65535.
 *   RdfStereoConfig, by value: fb16 = round(16 f B), fbp16 = round(16 f Bp), B the baseline and Bp the projector's offset
 *   from the left imager, in depth units, 0 <= fbp16 <= fb16 < 2^31 - 2^15; 1 <= max_disparity (D below) <= 256;
 *   0 <= ambient, ir_noise_amp, census_margin, lr_max <= 255; 0 <= uniqueness <= 100; 1 <= dq_min <= 65535.
 *   All hashing is rule H's mix, uint32 and wrapping.  The frame is pixel p = y * dim_x + x of frame n.
 *
 * I. The two IR images.  Camera c (0 left, 1 right), with Z the depth that camera's render has at (x, y): if the pixel
 *    shows a surface, s = -((fbp16 + Z / 2) / Z) for the left camera and s = +(((fb16 - fbp16) + Z / 2) / Z) for the right
 *    (integer divisions), sq = 16 x + s, u = sq >> 4 (arithmetic) as a uint32, fr = sq & 15.  The projector's texel is
 *      tex(u, y) = h < dot_threshold ? 64 + (h & 127) : 0,   h = mix(mix(pattern_seed + y * 0x9e3779b9) ^ u):
 *    the pattern belongs to the projector, not to the frame.  The intensity is
 *      I = ambient + (surface ? ((16 - fr) * tex(u, y) + fr * tex(u + 1, y)) >> 4 : 0) + noise,  clamped to [0, 255],
 *      noise = (mix(mix(seed + n * 0x9e3779b9 + c * 0x632be5ab) ^ p) % (2 a + 1)) - a  for a = ir_noise_amp > 0, else 0
 *    (frame n under seed s is frame 0 under seed s + n * 0x9e3779b9, as in rule H).
 * N. Census.  Bit k of a pixel's 62-bit census, k counting from 0 over dy = -3..3 (outer) and dx = -4..4 (inner) without
 *    the centre, is set iff I(x + dx, y + dy) > I(x, y) + census_margin; I outside the image is 0.  (With a margin of
 *    about twice ir_noise_amp, noise alone sets no bit: an untextured surface has an all-zero census.)
 * M. Cost.  ham(x, y, d) = popcount(censusL(x, y) ^ censusR(x - d, y)) where 0 <= x - d, 0 <= x < dim_x and 0 <= y < dim_y,
 *    else 62.  C(x, y, d) is the sum of ham over the 5 x 5 box round (x, y), for any integer x (<= 1550).  Disparities are
 *    0 <= d < D.  The right-referenced cost is C_R(xr, y, d) = C(xr + d, y, d): the box moves with the pixel.
 * W. Winners and checks, per left pixel.  d* is the d of least C, the lowest among equals.  second is the least C over
 *    |d - d*| >= 2; the pixel is unique iff there is no such d or C* * 100 < second * (100 - uniqueness).  dR(xr, y) is the
 *    winner of C_R found the same way; the pixel passes the left-right check iff x - d* >= 0 and |dR(x - d*, y) - d*| <=
 *    lr_max.  Sub-pixel, the equiangular fit: if 1 <= d* <= D - 2 and C* > 0, with cm = C(d* - 1), cp = C(d* + 1) and den =
 *    max(cm - C*, cp - C*) > 0, sub = floor((16 * (cm - cp) + den) / (2 * den)) clamped to [-8, 8]; else sub = 0 (C* = 0 is an
 *    exact match of all 25 windows: the disparity is whole, whatever the neighbours cost).  dq = 16 d* + sub.
 *    The pixel is valid iff it is unique, passes the left-right check and dq >= dq_min.
 * Z. Stored values.  A valid pixel gets depth = clamp((fb16 + dq / 2) / dq, 1, 65534) and the label labels_l(x, y); any
 *    other pixel gets empty_depth and label 0, as in rule E.  Every pixel of depth_out and labels_out is written.
 *
 * Optional outputs, each may be NULL: ir_out uint8 [n_frames][2][dim_y][dim_x], the images of rule I; dq_out uint16
 * [n_frames][dim_y][dim_x], dq of every pixel, valid or not; reason_out uint8 [n_frames][dim_y][dim_x]: 0 for a valid
 * pixel, else bit 0 not unique, bit 1 left-right check failed, bit 2 dq < dq_min.  rdf_stereo_ir is rule I alone.
 * n_frames < 1, a negative dimension, a config outside the ranges above or a misaligned pointer is RDF_ERR_BAD_ARG; dim_x or
 * dim_y above 32768, or 2^39 pixels and more in the batch, RDF_ERR_TOO_LARGE; zero pixels is a successful no-op; else a
 * NULL input, workspace, depth_out or labels_out (rdf_stereo_ir: ir_out) is RDF_ERR_NULL_PTR.  Rejected arguments leave
 * the outputs untouched.  Pixel indices are 64-bit.
 * workspace: rdf_stereo_workspace_bytes(n_frames, dim_x, dim_y, D) bytes (21 per pixel and frame: both census images, the
 * left winners, the IR images, the right winners; 0 for rejected arguments), 8-byte aligned, contents irrelevant before and
 * after; a workspace for more frames serves a call with fewer.  Five launches, stream-ordered, nothing read back, none of
 * which waits for another workgroup: rule I with one lane per pixel and camera; both census images from an LDS tile; the
 * matcher once per direction (a workgroup of four waves owns 60 columns x 32 rows: the other image's census, widened by
 * D - 1 columns, is its LDS tile; a lane owns a column, keeps its own census of the wave's 12 rows in registers, takes one
 * popcount per row and d, slides the vertical 5-sum in registers and takes the horizontal 5-sum from its neighbour lanes;
 * winner, second, cm and cp stay in registers across the d loop); then the resolve pass of rules W (left-right) and Z.
 */
typedef struct RdfStereoConfig {
    int32_t fb16, fbp16;
    int32_t max_disparity;          /* D */
    uint32_t dot_threshold;         /* dot density * 2^32 */
    uint32_t pattern_seed;
    int32_t ambient, ir_noise_amp, census_margin;
    int32_t uniqueness, lr_max, dq_min;
} RdfStereoConfig;

size_t rdf_stereo_workspace_bytes(int n_frames, int dim_x, int dim_y, int max_disparity);
int rdf_stereo_ir(int n_frames, int dim_x, int dim_y, const uint16_t *depth_l, const uint16_t *depth_r, RdfStereoConfig config,
                  uint32_t seed, uint8_t *ir_out, void *stream);
int rdf_stereo_sense(int n_frames, int dim_x, int dim_y, const uint16_t *depth_l, const uint16_t *labels_l,
                     const uint16_t *depth_r, RdfStereoConfig config, uint32_t seed, uint16_t empty_depth, void *workspace,
                     uint16_t *depth_out, uint16_t *labels_out, uint8_t *ir_out, uint16_t *dq_out, uint8_t *reason_out,
                     void *stream);

/*
 * Leaf refit: the leaf distributions of a trained forest re-estimated from labelled depth frames -- the frames the camera
 * will really deliver, or more of them than the trainer can hold -- while the tree structure stays as it is.  The reference
 * has no counterpart; the rules below are this library's own, tests/refit_numpy.py restates them, and the kernels match that
 * bit for bit: every count is an integer, so no result depends on the order in which pixels are visited.
 *
 *   forest  float32 [T][N][E], N = 2^D - 1 nodes in heap order, E = 7 + 2C: the reference layout, what rdf_eval_forest takes
 *           (ux, uy, vx, vy, thresh, l_next, r_next, l_pdf[C], r_pdf[C]).  1 <= T, 1 <= D <= 30, 1 <= C <= 65535.
 *   slot    (t, n, s): side s (0 left, 1 right) of node n of tree t.  It is a LEAF SLOT iff floor(rec[5 + s]) != -1 with the
 *           floor of rule R2 -- the test inference makes, at every level, D - 1 included.
 *   counts  uint64 [T][N][2][C];  totals uint64 [4].  Both 8-byte aligned.
 *
 * R1. Pixels (rdf_labels_refit_count).  depth, labels uint16 [n_img][dim_y][dim_x].  For every pixel, with l its label and
 *     d its depth:  l == 0: ignored.  l >= C: totals[1] += 1, ignored.  d == 0 or d == 65535: totals[2] += 1, ignored (what
 *     inference skips: a leaf's PDF only matters for pixels inference evaluates).  Else totals[0] += 1 and the pixel walks
 *     every tree from the root.
 * R2. The walk, as inference walks (rdf_eval_forest): at node rec, for each of the offsets o = rec[0..3], q = floor((scale_factor
 *     * o) / (float)d) -- one multiply and one IEEE divide, each rounded to nearest, then floor to int32 with saturation and NaN
 *     -> 0; the probes are at (x + q_ux, y + q_uy) and (x + q_vx, y + q_vy), the adds wrapping in int32; a probe outside
 *     [0, dim_x) x [0, dim_y), checked per axis (no wrap into the next row or image), reads 65535.0, any other reads the
 *     frame's value as a float, a 0 included; f = du - dv.  f < rec[4] goes to side 0, anything else (NaN included) to side
 *     1.  If that side is a leaf slot, counts[t][n][s][l] += 1 and the walk ends; else it goes on at child 2g + s of the
 *     next level (g the node's index within its level), and if there is no next level totals[3] += 1 and nothing is counted.
 *     So counts sums to T * totals[0] - totals[3].
 *     The call ADDS onto counts and totals; the caller zeroes them (as rdf_score_labels).  A negative dimension, T, D or C
 *     outside the ranges above or a misaligned pointer is RDF_ERR_BAD_ARG; zero pixels is a successful no-op; else a NULL
 *     pointer is RDF_ERR_NULL_PTR; n_img * dim_y * dim_x >= 2^31 (callers split the batch by images) or N * 2 * C >= 2^32 is
 *     RDF_ERR_TOO_LARGE.  Rejected arguments leave counts and totals untouched.
 *     One launch, nothing read back.  A wave whose 64 pixels carry no label does nothing.  Leaf slots of the first L levels
 *     (L the largest with T * (2^L - 1) * 2 * C <= 4096) are counted in a 32-bit LDS histogram that a workgroup adds to counts
 *     once; below that the lanes of a wave that reached the same (slot, class) share one add, into a hashed table of 2048
 *     (cell, count) pairs in LDS that a workgroup also adds to counts once, or, where another cell holds the bucket, as a
 *     64-bit atomic straight into counts.
 * R3. PDFs (rdf_labels_refit_apply).  A leaf slot is REACHABLE iff every ancestor's flag on the way to it floors to -1.  The
 *     call rewrites rec[7 + s * C + c], c = 0..C-1, of reachable leaf slots and nothing else: rec[0..6], unreachable nodes and
 *     "go on" sides keep their bytes.  With S the sum of the slot's own counts over the classes and min_count >= 1:
 *       S >= min_count:  pdf[c] = (float)cnt[c] / (float)S -- uint64 to fp32 rounded to nearest even, one IEEE divide, the
 *                        trainer's expression.  No pixel has label 0, so entry 0 is 0.
 *       else, fallback RDF_REFIT_FALLBACK_KEEP:  the old entries stay, bit for bit.
 *       else, RDF_REFIT_FALLBACK_ANCESTOR:  sub[t][a][c] = over both sides s of node a, cnt[t][a][s][c] where (a, s) is a leaf
 *                        slot, else sub[t][child 2g + s][c], else (level D - 1) nothing: the class counts of the leaf slots
 *                        below a, in integers.  Of the chain n, parent(n), ..., root the nearest a with Z = sum_c sub[t][a][c]
 *                        >= min_count gives pdf[c] = (float)sub[t][a][c] / (float)Z; if not even the root has that many, the
 *                        old entries stay.
 *     report uint64 [4], overwritten: leaf slots written from their own counts, written from an ancestor, kept, and reachable
 *     leaf slots (the sum of the three).  workspace: rdf_labels_refit_workspace_bytes(T, D, C) bytes (0 for a rejected
 *     shape), 8-byte aligned, contents irrelevant before and after.  min_count == 0, an unknown fallback, a shape outside the
 *     ranges or a misaligned pointer is RDF_ERR_BAD_ARG, else a NULL pointer RDF_ERR_NULL_PTR; nothing is launched then.
 *     One launch per level top-down, after one per level bottom-up with the ancestor fallback; stream-ordered, nothing read
 *     back.  A packed table made of this forest (rdf_forest_pack) holds the old PDFs: pack again.
 */
#define RDF_REFIT_FALLBACK_KEEP 0
#define RDF_REFIT_FALLBACK_ANCESTOR 1
int rdf_labels_refit_count(const uint16_t *depth, const uint16_t *labels, int n_img, int dim_x, int dim_y, const float *forest,
                           int n_trees, int max_depth, int n_classes, float scale_factor, uint64_t *counts, uint64_t *totals,
                           void *stream);
size_t rdf_labels_refit_workspace_bytes(int n_trees, int max_depth, int n_classes);
int rdf_labels_refit_apply(float *forest, int n_trees, int max_depth, int n_classes, const uint64_t *counts, uint64_t min_count,
                           int fallback, void *workspace, uint64_t *report, void *stream);

/*
 * Pruning: reduced-error (cost-complexity) pruning of a trained forest on held-out counts.  The trainer grows every tree until
 * a side is pure or the depth is used up; a subtree that a handful of training pixels asked for costs a dependent node fetch
 * per level and gives the least reliable leaves.  rdf_labels_prune_plan decides, from the counts of rule R2 taken on frames the
 * trainer has not seen, which subtrees label those frames no better than one leaf would; rdf_labels_prune_apply folds them.
 * The reference has no counterpart; the rules below are this library's own, tests/prune_numpy.py restates them, and the kernels
 * match that bit for bit.  Layout, leaf slot, the floor of a flag, "reachable" and sub[t][a][c] are those of the leaf refit
 * above.  level(n) = floor(log2(n + 1)); node n has the children 2n + 1 + s.  All arithmetic is in unsigned 64-bit integers
 * except the final PDFs.  Parameters: 0 <= cost_per_leaf < 2^32, min_count >= 0, 1 <= max_levels <= D.
 *
 * P1. A leaf slot's error.  For a leaf slot (t, n, s) with counts cnt[c] and S their sum, k* is the argmax of the slot's current
 *     PDF by the evaluator's rule: start at 0.0f, strict >, the first index wins, NaN never wins, none above 0 gives class 0.
 *     err_slot = S - cnt[k*].
 * P2. Bottom-up, per node a.  For each side s: a leaf slot gives e_s = err_slot, l_s = 1; else, if the child c = 2a + 1 + s
 *     exists and collapse(c), e_s = Z(c) - max_k sub[c][k], l_s = 1; else, if the child exists, e_s = err(c), l_s = leaves(c);
 *     else (a "go on" at level D - 1, where walks fall off) e_s = 0, l_s = 0.  err(a) = e_0 + e_1, leaves(a) = l_0 + l_1; errB(a)
 *     and leavesB(a) are the same recursion with no collapse anywhere.  Z(a) = sum_k sub[a][k], err_leaf(a) = Z(a) - max_k
 *     sub[a][k].  collapse(a) is true iff a is not the root and level(a) >= max_levels, or Z(a) < min_count, or
 *     err_leaf(a) <= err(a) + cost_per_leaf * max(leaves(a) - 1, 0).  Note the <=: a tie collapses.
 * P3. Top-down (rdf_labels_prune_apply).  Reachability is made again on the way down: the root is reachable; for a reachable
 *     node n and a "go on" side s whose child c exists, if collapse(c) then rec[5 + s] := +0.0f, the side's PDF becomes
 *     (float)sub[a][k] / (float)Z(a) -- uint64 to fp32 rounded to nearest even, one IEEE divide -- with a the nearest of c,
 *     parent(c), ..., root that has Z(a) >= 1, or all +0.0f if there is none, and counts[t][n][s][:] := sub[c][:]; else c is
 *     reachable.  After the call every node that is not reachable has a record of all +0.0f and counts of 0.  rec[0..4] of
 *     reachable nodes, PDFs of leaf slots that were leaf slots before, and "go on" flags at level D - 1 keep their bytes.  Where
 *     the counts were 0 outside reachable leaf slots (as rule R2 leaves them), their sum is unchanged.
 * P4. report uint64 [8], written by the plan: [0] reachable leaf slots before, [1] after, [2] "go on" slots turned into leaf
 *     slots, [3] the new depth D' = 1 + the deepest level that holds a reachable node after, [4] sum_t errB(root), [5] sum_t
 *     err(root), [6] sum_t Z(root), [7] reachable nodes after.  The first 2^D' - 1 records of each tree are a forest of depth D'
 *     that labels every pixel as the pruned one does.
 *
 * rdf_labels_prune_plan reads forest and counts and writes workspace and report; it may be called any number of times, with
 * other parameters, before one rdf_labels_prune_apply, which uses the workspace of the last plan and must be given the forest
 * and counts that plan read, unchanged.  workspace: rdf_labels_prune_workspace_bytes(T, D, C) bytes (0 for a rejected shape),
 * 8-byte aligned, contents irrelevant before a plan.  After a plan it begins with one byte per node, uint8 [T][N]: bit 0
 * reachable before, bit 1 collapse(n) (made for the nodes reachable before only), bit 2 reachable after.  A shape outside the
 * ranges of the leaf refit, cost_per_leaf >= 2^32, max_levels outside 1..D or a misaligned pointer (4 bytes for forest, 8 for
 * the others) is RDF_ERR_BAD_ARG, else a NULL pointer RDF_ERR_NULL_PTR; nothing is launched then and every buffer keeps its
 * bytes.  Stream-ordered, nothing read back.  A plan is four launches and two memsets whatever the depth: the levels with T *
 * 2^j <= 1024 are swept by one workgroup with a barrier between levels, in both directions; every node of the first level
 * below them roots a subtree that one workgroup sweeps the same way.  apply is two launches.  A packed table made of this
 * forest (rdf_forest_pack) holds the old tree: pack again.
 */
size_t rdf_labels_prune_workspace_bytes(int n_trees, int max_depth, int n_classes);
int rdf_labels_prune_plan(const float *forest, int n_trees, int max_depth, int n_classes, const uint64_t *counts,
                          uint64_t cost_per_leaf, uint64_t min_count, int max_levels, void *workspace, uint64_t *report,
                          void *stream);
int rdf_labels_prune_apply(float *forest, int n_trees, int max_depth, int n_classes, uint64_t *counts, const void *workspace,
                           void *stream);

/*
 * Forest posteriors: what rdf_eval_forest sums per pixel and discards.  rdf_labels_forest_posterior evaluates a forest as
 * rdf_eval_forest does and writes, per evaluated pixel, the label, a 16-bit confidence (the winning class's share of the
 * summed leaf distributions) and, on request, the sums themselves; a pixel whose confidence is below min_conf is left out of
 * the label map (a reject option).  rdf_labels_confidence_counts bins (prediction, confidence, truth) into a reliability
 * histogram.  The reference has no counterpart; the rules below are this library's own, tests/posterior_numpy.py restates
 * them, and the kernels match that bit for bit: the sums are made in a stated order and the counts are integers.
 *
 *   forest  float32 [T][N][E], the reference layout of the leaf refit above.  1 <= T, 1 <= D <= 30, 1 <= C <=
 *           RDF_POSTERIOR_MAX_CLASSES.
 *   depth   uint16 [n_img][dim_y][dim_x].  With r = labels_reduce >= 1, Hl = dim_y / r, Wl = dim_x / r:
 *   filter, labels_out, conf_out  uint16 [n_img][Hl][Wl];  sums_out float32 [n_img][C][Hl][Wl], planar.
 *           Each of the three outputs may be NULL, not all of them.
 *
 * Q1. Pixels, as rdf_eval_forest chooses them.  Label pixel (x, y) of image i reads depth pixel (x * r, y * r).  If filter_class
 *     != -1 and filter[i][y][x] != filter_class the pixel is skipped; if its depth d is 0 or 65535 it is skipped.  A skipped
 *     pixel is written in none of the three outputs: callers pre-fill, as with rdf_eval_forest.
 * Q2. Walk and sums.  For t = 0 .. T-1 the pixel walks tree t exactly as rule R2 describes: one multiply and one IEEE divide
 *     per offset, floor with saturation and NaN -> 0, a wrapping add, a per-axis out-of-range probe reads 65535.0, f < thresh
 *     goes left and anything else right, and the leaf-slot test floor(rec[5 + s]) != -1 is made at every level.  At a leaf
 *     slot acc[c] = acc[c] + rec[7 + s * C + c] for every c: one fp32 add each, rounded to nearest, no contraction; acc starts
 *     at +0.0f and the trees are taken in index order.  A walk that is told to go on at level D - 1 adds nothing.
 * Q3. Label.  best = 0.f, label = 0; for c ascending, acc[c] > best replaces both.  The inference argmax: ties go to the
 *     lowest class, an all <= 0 or NaN vote gives 0, NaN never wins.
 * Q4. Confidence.  S = (..((0.f + acc[0]) + acc[1]) + ..) in fp32, in class order.  If !(S > 0.f), conf = 0; else q = best / S
 *     (one IEEE divide), v = floor(q * 65535.0f) with rule R2's floor (saturating, NaN -> 0), conf = min(max(v, 0), 65535).
 *     A one-hot vote gives 65535, a two-way tie of equal halves 32767.
 * Q5. Outputs, for every evaluated pixel: conf_out = conf; sums_out[i][c][y][x] = acc[c] for all c < C; labels_out = label iff
 *     conf >= min_conf, else labels_out keeps the caller's bytes.  With min_conf == 0 the label map is byte for byte what
 *     rdf_eval_forest writes for the same arguments.
 * Q6. Arguments.  T < 1, D outside 1..30, C < 1, r < 1, a negative dimension, filter_class outside -1..65535, min_conf outside
 *     0..65535 or a misaligned pointer (2 bytes for the maps, 4 for forest and sums_out) is RDF_ERR_BAD_ARG; C >
 *     RDF_POSTERIOR_MAX_CLASSES or n_img * dim_y * dim_x >= 2^31 (callers split the batch by images) RDF_ERR_TOO_LARGE; zero
 *     label pixels is a successful no-op; else a NULL depth or forest, all three outputs NULL, or a NULL filter with
 *     filter_class != -1 is RDF_ERR_NULL_PTR.  A rejected call launches nothing and writes nothing.  An accepted call makes
 *     one launch, is stream-ordered and reads nothing back: one lane per label pixel, a wave leaves at once when none of
 *     its 64 pixels is evaluated, the sums stay in registers, no LDS, no atomics.
 * Q7. Confidence counts (rdf_labels_confidence_counts).  pred, conf uint16 [n_img][Hl][Wl]; truth uint16 [n_img][dim_y][dim_x],
 *     sampled at (x * r, y * r) as rdf_score_labels samples it.  counts uint64 [2 * bins + 2], 8-byte aligned: the call ADDS,
 *     the caller zeroes.  Per label pixel, with the raw values p, k (the confidence) and t:  t == 0: ignored.  Else
 *     counts[2 * bins + 1] += 1 (labelled pixels); if p == 65535, counts[2 * bins + 0] += 1 (labelled, not classified); else,
 *     with b = (k * bins) >> 16, counts[2 * b + (p == t)] += 1.  bins outside 1..1024 is RDF_ERR_BAD_ARG; the other error rules
 *     are rdf_score_labels': r < 1, a negative dimension or a misaligned pointer RDF_ERR_BAD_ARG, zero label pixels a successful
 *     no-op, else a NULL pointer RDF_ERR_NULL_PTR and n_img * dim_y * dim_x >= 2^31 RDF_ERR_TOO_LARGE.  One launch; 32-bit LDS
 *     histograms, each workgroup adds its non-zero cells once with 64-bit integer atomics: the result does not depend on the
 *     order of arrival.
 */
#define RDF_POSTERIOR_MAX_CLASSES 16
int rdf_labels_forest_posterior(const uint16_t *depth, int n_img, int dim_x, int dim_y, const float *forest, int n_trees,
                                int max_depth, int n_classes, const uint16_t *filter, int filter_class, int labels_reduce,
                                float scale_factor, int min_conf, uint16_t *labels_out, uint16_t *conf_out, float *sums_out,
                                void *stream);
int rdf_labels_confidence_counts(int n_img, int dim_x, int dim_y, int labels_reduce, int bins, const uint16_t *pred,
                                 const uint16_t *conf, const uint16_t *truth, uint64_t *counts, void *stream);

/*
 * Soft modes: mean-shift mode finding in which every pixel pulls with a weight -- the forest's confidence in it -- where
 * rdf_mean_shift (librdf_hip.so) lets every pixel of a class pull equally.  rdf_labels_composite_weights makes the weight
 * map of a layered stack from the per-layer labels and confidences that the gated stack leaves (rules Q); for a plain
 * forest the confidence map of rdf_labels_forest_posterior is the weight map.  rdf_labels_weighted_modes finds the modes
 * and, on request, the fingertip heights of any number of frames in one launch.  The reference keeps no posterior and has
 * no counterpart; the rules below are this library's own and tests/soft_modes_numpy.py restates them.
 *
 * Composite weights.  layer_labels, layer_conf: DEVICE tables of n_layers device pointers, each to a uint16
 * [n_img][dim_y][dim_x] map.  cond int32 [n_cond][2], the conditions table of rdf_composite.  weights_out uint16
 * [n_img][dim_y][dim_x].
 * S1. Path: exactly rdf_composite's walk.  off = 0; for layer j = 0 .. n_layers - 1: l = layer_labels[j][i][y][x]; if l is 0 or
 *     65535, stop: nothing is written.  e = off + l - 1; if e is outside 0 .. n_cond - 1, stop: nothing is written.  (t, v) =
 *     cond[e]; t == 0: the pixel is final; else off = v and the walk goes on.  Falling off the last layer writes nothing.  A
 *     weight is written exactly where rdf_composite writes a label, and nowhere else: callers pre-fill.
 * S2. Weight: w = 65535; at every layer visited, the final one included, with k = layer_conf[j][i][y][x]:
 *     w = (w * k + 32767) / 65535 in unsigned 32-bit integers (65535^2 + 32767 < 2^32).  One layer gives w = k; 65535 is
 *     neutral, 0 absorbs.
 * S3. Store: weights_out[i][y][flip_x ? dim_x - 1 - x : x] = w, the mirror rdf_layered_run_hand applies to the composite.
 *
 * Weighted modes.  labels, weights uint16 [n_img][dim_y][dim_x]; weights may be NULL: every weight is 1.  means_out float64
 * [n_img][num_classes][2] = (x, y); variances float32 [num_classes].
 * S4. Pixels.  The pixels p of class c = 1 .. num_classes in image i are those with labels[p] == c; each has the integer
 *     weight w_p.  Labels 0, 65535 and anything above num_classes are ignored.  A pixel with w_p = 0 contributes nothing; the
 *     others are the class's COUNTED pixels.
 * S5. Round 0: m = (sum w x / sum w, sum w y / sum w).  For maps below 2^21 pixels the three sums are integers below 2^53, exact
 *     in fp64 in any order, followed by one IEEE divide each: a bit-exact target.  sum w == 0 gives NaN (0 / 0), as a class
 *     without pixels does in rdf_mean_shift.
 * S6. Round r >= 1: v2 = (double)(float)(var * var), as rdf_mean_shift; g_p = exp(-((x - mx)^2 + (y - my)^2) / (2 v2)), which
 *     the kernel takes as the product of a column and a row factor, exp(-(x - mx)^2 / (2 v2)) * exp(-(y - my)^2 / (2 v2)), from
 *     two tables per round when dim_x + dim_y <= 3072 and v2 > 0; m += (sum (w g) dx / sum w g, sum (w g) dy / sum w g) with dx
 *     = x - mx, dy = y - my.  The sums are taken in an order fixed by the code (below), with no floating-point atomics: the
 *     result is the same bits from run to run and from any pointer alignment.  num_rounds == 0 returns zeros.  v2 == 0 (a
 *     variance whose float square is 0) takes no tables: exp(-d / 0) is 0 off the mean and NaN on it, so such a class is NaN
 *     from round 1 on, as in rdf_mean_shift.
 * S7. Heights, when n_ids > 0: heights_out[f * heights_stride + k], k < n_ids, from frame f's final mean of class class_ids[k]
 *     by the rule of rdf_fingertip_heights (truncate, times labels_reduce, off-frame or NaN gives NaN, fp32 deprojection, fp64
 *     plane row; depth uint16 [n_img][depth_dim_y][depth_dim_x]): bit for bit what that call returns for the same means.  An
 *     id outside 1 .. num_classes gives NaN.  n_ids == 0: no heights, and the height arguments are not looked at.
 * S8. Arguments.  n_layers < 1, a negative dimension or count, num_classes outside 1..64, dim_x or dim_y above 65535, num_rounds
 *     < 0, n_ids outside 0..1024, with n_ids > 0 labels_reduce < 1 or heights_stride < n_ids, or a misaligned pointer (2 bytes
 *     for the maps, 4 for cond, variances, class_ids and plane, 8 for the pointer tables, means_out and heights_out) is
 *     RDF_ERR_BAD_ARG; n_img * dim_y * dim_x >= 2^31 (of the labels or of the depth frames) or n_img > 65535 frames in one
 *     weighted_modes call RDF_ERR_TOO_LARGE; zero pixels is a successful no-op; else a NULL pointer (weights excepted, and the
 *     height arguments when n_ids == 0) is RDF_ERR_NULL_PTR.  A rejected call launches nothing.
 * Each call is one launch, stream-ordered, with nothing read back; means_out and heights_out may be mapped pinned host memory.
 * composite_weights: one lane per pixel, a wave leaves at once when none of its 64 pixels starts a path.  weighted_modes:
 * one workgroup of 1024 threads per (class, frame), grid (num_classes, n_img).  The workgroup lists the class's counted pixels
 * once in LDS -- x | y << 16 plus the 16-bit weight, 6 bytes an entry; pixels of weight 0 are skipped at listing time and take
 * no slot -- and runs all rounds on the list.  The list order is fixed: the map is cut into batches of 106 496 pixels, step k
 * = 0 .. 12 of wave w = 0 .. 15 covers the 512 pixels from (k * 16 + w) * 512 of the batch on, eight consecutive ones a lane; a
 * lane's pixels of all its steps take consecutive slots, and the lanes of a wave, the waves and the batches follow in index
 * order (positions from scans, never from arrival).  Thread t sums entries t, t + 1024, ...; a wave's 64 partial sums are added
 * by a shift-add scan inside each row of 16 lanes and the four rows in order, the 16 waves in order.  A class with more than
 * rdf_labels_weighted_modes_list_cap() counted pixels (20 480: the list and the tables fill 148 288 B of a compute unit's 160
 * KB) is not listed: thread t visits pixels t, t + 1024, ... of the maps in every round.
 */
int rdf_labels_composite_weights(const uint16_t *const *layer_labels, const uint16_t *const *layer_conf, int n_layers, int n_img,
                                 int dim_x, int dim_y, const int32_t *cond, int n_cond, int flip_x, uint16_t *weights_out,
                                 void *stream);
int rdf_labels_weighted_modes(const uint16_t *labels, const uint16_t *weights, int n_img, int dim_x, int dim_y, int num_classes,
                              const float *variances, int num_rounds, double *means_out, const int *class_ids, int n_ids,
                              const uint16_t *depth, int depth_dim_x, int depth_dim_y, int labels_reduce, float fx, float fy,
                              float ppx, float ppy, const float *plane, double *heights_out, int heights_stride, void *stream);
uint32_t rdf_labels_weighted_modes_list_cap(void);

/*
 * Joint votes: a second use of a trained forest's structure.  Classification finds a fingertip only where pixels of its class
 * are seen; here every leaf slot stores, per joint, a depth-normalised offset towards the joint, every hand pixel of a frame,
 * whatever its label, casts the votes of the leaf slots it reaches into a coarse accumulator per (frame, joint), and the joint
 * is the accumulator's mode -- also where the joint itself is hidden.  rdf_labels_votes_count sums offsets on frames whose
 * joints are known, rdf_labels_votes_fit turns the sums into a vote table, rdf_labels_votes_cast casts and finds the modes.
 * The reference has no counterpart; the rules below are this library's own, tests/votes_numpy.py restates them, and the
 * kernels match that bit for bit: all arithmetic is in integers, so no result depends on the order in which pixels are visited.
 *
 *   forest   float32 [T][N][E], the reference layout of the leaf refit above, with its leaf slots, rule R2's walk and rule R3's
 *            "reachable".  1 <= T, 1 <= D <= 30, 1 <= C <= 65535 (the classes' PDFs are not read).
 *   J        n_joints, 1 .. RDF_VOTES_MAX_JOINTS;  radius 0 .. RDF_VOTES_MAX_RADIUS.
 *   sums     uint64 [T][N][2][J][5]: count, sum ox, sum oy, sum oz, sum (ox^2 + oy^2).  The three signed sums are kept in two's
 *            complement: the adds wrap.  totals uint64 [4].  Both 8-byte aligned.
 *   votes    int32 [T][N][2][J][4] = (mx, my, mz, w), 16-byte aligned; w == 0: no vote.
 *   targets  int32 [n_img][J][3] = (tx, ty, tz): pixel x, pixel y, depth units; 4-byte aligned.  (tx, ty) may lie outside the
 *            frame.  Joint j is ABSENT from frame i iff tz <= 0 or tz >= 65535.
 *   floordiv(a, b), b > 0: the integer floor of a / b (towards minus infinity), exact, in 64 bits.
 *
 * V1. Pixels of the count (rdf_labels_votes_count).  depth, labels uint16 [n_img][dim_y][dim_x].  For every pixel (x, y) of
 *     image i, with l its label and d its depth:  l == 0: ignored; any other l is "hand" (the class is not used: l >= C is
 *     fine).  d == 0 or d == 65535: totals[1] += 1, ignored.  Else totals[0] += 1 and the pixel walks every tree by rule R2,
 *     unchanged.  A walk that is told to go on at level D - 1 does totals[2] += 1 and adds nothing.  At the leaf slot (t, n, s)
 *     a walk ends in, for every joint j not absent from frame i: dx = tx - x, dy = ty - y; if |dx| > radius or |dy| > radius
 *     the joint is skipped; else ox = floordiv(dx * d, 64), oy = floordiv(dy * d, 64), oz = tz - d, the five words of
 *     sums[t][n][s][j] get +1, +ox, +oy, +oz, +(ox^2 + oy^2), and totals[3] += 1.  With radius <= 255, |ox| < 2^18, so one
 *     square term is below 2^37 and a slot of fewer than 2^26 pixels cannot wrap the last word.
 *     The call ADDS onto sums and totals; the caller zeroes them.  A negative dimension, T, D or C outside the ranges, J or
 *     radius outside theirs or a misaligned pointer is RDF_ERR_BAD_ARG; zero pixels is a successful no-op; else a NULL pointer
 *     is RDF_ERR_NULL_PTR; n_img * dim_y * dim_x >= 2^31 (callers split the batch by images) or N * 2 * J * 5 >= 2^32 is
 *     RDF_ERR_TOO_LARGE.  Rejected arguments leave sums and totals untouched.  One launch, nothing read back: one lane per
 *     pixel, a wave whose 64 pixels carry no label does nothing, five 64-bit atomics per (pixel, tree, joint in reach).
 * V2. Votes (rdf_labels_votes_fit).  Every element of votes is written.  A slot that is not a reachable leaf slot gets zeros.
 *     For a reachable leaf slot and joint j, with n the count:  n < min_count or n >= 2^26: (0, 0, 0, 0), DROPPED FOR SUPPORT
 *     (the upper bound is what keeps the sum of squares from wrapping).  Else mx = floordiv(sum ox, n), my and mz alike (the
 *     sums read as signed); var = max(0, floordiv(sum (ox^2 + oy^2), n) - (mx^2 + my^2)); var > max_var: (0, 0, 0, 0), DROPPED
 *     FOR SPREAD; else w = 256 - floordiv(var * 256, max_var + 1), which is in 1..256, and the entry is (mx, my, mz, w).
 *     min_count >= 1, max_var <= 2^38.  Sums that rule V1 cannot have made (a mean outside int32) give an unspecified entry,
 *     never an access out of range.  report uint64 [4], overwritten: reachable leaf slots, (slot, joint) pairs with a vote,
 *     pairs dropped for support, pairs dropped for spread; the last three sum to J times the first.  A shape, J, min_count or
 *     max_var outside the ranges or a misaligned pointer (4 bytes for forest, 8 for sums and report, 16 for votes) is
 *     RDF_ERR_BAD_ARG, N * 2 * J * 5 >= 2^32 RDF_ERR_TOO_LARGE, else a NULL pointer RDF_ERR_NULL_PTR; nothing is launched then.
 *     One launch whatever the depth (a lane owns a node and climbs to the root for its reachability), stream-ordered, nothing
 *     read back.  A table belongs to the forest's structure: after rdf_labels_prune_apply, fit again.
 * V3. Pixels of the cast (rdf_labels_votes_cast).  depth uint16 [n_img][dim_y][dim_x]; with r = labels_reduce >= 1, Hl = dim_y
 *     / r, Wl = dim_x / r, pixels are chosen as rule Q1 chooses them: label pixel (x, y) of image i reads depth pixel (xd, yd) =
 *     (x * r, y * r).  gate uint16 [n_img][Hl][Wl] may be NULL; with a gate a pixel takes part iff its gate value is neither 0
 *     nor 65535, so a label map, a composite or a gated posterior's label map serves as it is.  A pixel whose depth d is 0 or
 *     65535 does not take part.  A pixel that takes part walks every tree by rule R2 at (xd, yd); a walk that falls off casts
 *     nothing.
 * V4. A vote.  At the slot reached, for every j whose w is in 1..256 (any other w, which rule V2 never writes, is no vote):
 *     vx = xd + floordiv(128 * mx + d, 2 * d) and vy alike with my -- the inverse of V1's normalisation, rounded half up --
 *     and vz = d + mz.  The vote is dropped if vx is outside [0, dim_x), vy outside [0, dim_y) or vz outside [1, 65534].  Else,
 *     with a = cell_shift (0 .. RDF_VOTES_MAX_CELL_SHIFT), (cx, cy) = (vx >> a, vy >> a), Wa = ((dim_x - 1) >> a) + 1 and Ha
 *     alike:  acc[i][j][cy][cx] += w (uint32) and zacc[i][j][cy][cx] += w * vz (uint64).
 * V5. A joint.  Per (i, j), with b = box (0 .. RDF_VOTES_MAX_BOX):  S(cx, cy) = the sum of acc over |ex| <= b, |ey| <= b,
 *     clipped to the grid, in 64 bits; best = max S; the winner is the first cell in row-major order (lowest cy, then lowest
 *     cx) with S == best.  best < max(min_support, 1): joints_out[i][j] = (-1, -1, 0, 0).  Else, over the winner's clipped box:
 *     X = floordiv(sum acc * (16 * (cx << a) + 8 * 2^a), best) and Y alike, in 1/16 pixel with a pixel's centre at +8 (the
 *     renderer's half-pixel convention); Z = floordiv(sum zacc, best); joints_out[i][j] = (X, Y, Z, min(best, 2^31 - 1)).
 *     joints_out int32 [n_img][J][4], 16-byte aligned; every element is written.
 * V6. Workspace, arguments, launches.  rdf_labels_votes_workspace_bytes(n_img, dim_x, dim_y, n_joints, cell_shift) bytes, 8-byte
 *     aligned: zacc, then acc; contents irrelevant before and after; 0 for a rejected shape.  A negative dimension, r < 1, a
 *     shape, J, cell_shift or box outside the ranges or a misaligned pointer (2 bytes for depth and gate, 4 for forest, 16 for
 *     votes and joints_out, 8 for workspace) is RDF_ERR_BAD_ARG; dim_x or dim_y above 65535, n_img * dim_y * dim_x >= 2^31,
 *     n_img * J >= 2^31 or Hl * Wl * T * 256 >= 2^32 (acc could wrap, and best stays below 2^32) RDF_ERR_TOO_LARGE; zero frames
 *     is a successful no-op; else a NULL pointer (gate excepted) RDF_ERR_NULL_PTR.  A rejected call launches nothing and writes
 *     nothing.  An accepted call is one clear of the workspace, one vote launch (one lane per label pixel, a wave leaves at
 *     once when none of its 64 pixels takes part, one 16-byte load and two atomics per vote) and one mode launch (one workgroup
 *     per (frame, joint)) on the caller's stream; nothing is read back, and any number of frames goes in one call.
 */
#define RDF_VOTES_MAX_JOINTS 16
#define RDF_VOTES_MAX_RADIUS 255
#define RDF_VOTES_MAX_CELL_SHIFT 4
#define RDF_VOTES_MAX_BOX 4
int rdf_labels_votes_count(const uint16_t *depth, const uint16_t *labels, const int32_t *targets, int n_img, int dim_x, int dim_y,
                           const float *forest, int n_trees, int max_depth, int n_classes, float scale_factor, int n_joints,
                           int radius, uint64_t *sums, uint64_t *totals, void *stream);
int rdf_labels_votes_fit(const float *forest, int n_trees, int max_depth, int n_classes, int n_joints, const uint64_t *sums,
                         uint64_t min_count, uint64_t max_var, int32_t *votes, uint64_t *report, void *stream);
size_t rdf_labels_votes_workspace_bytes(int n_img, int dim_x, int dim_y, int n_joints, int cell_shift);
int rdf_labels_votes_cast(const uint16_t *depth, int n_img, int dim_x, int dim_y, const uint16_t *gate, int labels_reduce,
                          const float *forest, int n_trees, int max_depth, int n_classes, float scale_factor, const int32_t *votes,
                          int n_joints, int cell_shift, int box, uint32_t min_support, void *workspace, int32_t *joints_out,
                          void *stream);

/*
 * The hand's shape: the forest's per-pixel votes pooled over a frame.  Every consumer above is per pixel or per joint; here the
 * leaf distributions a hand pixel reaches vote for a class of the WHOLE frame -- with a forest trained on frames labelled by
 * hand shape (open, fist, ...), the shape classification forest of Keskin et al. -- the votes of a frame are pooled, and the
 * pooled vote names the shape.  rdf_labels_shape_pool pools; rdf_labels_shape_decide turns a sequence of pooled votes into a
 * decision that is stable from frame to frame.  The reference has no counterpart; the rules below are this library's own,
 * tests/shape_numpy.py restates them, and the kernels match that byte for byte: a pixel's sums are made in a stated order and
 * everything added across pixels is an integer, so no result depends on the order in which pixels are visited.
 *
 *   forest  float32 [T][N][E], the reference layout.  1 <= T, 1 <= D <= 30, 1 <= C <= RDF_POSTERIOR_MAX_CLASSES.
 *   depth   uint16 [n_img][dim_y][dim_x];  filter uint16 [n_img][Hl][Wl] with r = labels_reduce, Hl = dim_y / r, Wl = dim_x / r.
 *   pool    uint64 [n_img][2 C + 2], 8-byte aligned: C soft sums, C hard votes, voting pixels, dead pixels.
 *   state   int32 [4] = (held, candidate, run, miss); a fresh state is (-1, -1, 0, 0).
 *   out     int32 [n_frames][4] = (raw, conf, held, changed).
 *
 * G1. Pixels: exactly rule Q1.  Label pixel (x, y) of image i reads depth pixel (x * r, y * r); the filter is tested first
 *     (filter_class != -1 and filter[i][y][x] != filter_class: skipped), then the pixel's own depth (0 or 65535: skipped).  A
 *     skipped pixel adds nothing to any word.
 * G2. Sums: exactly rule Q2 (rule R2's walk, acc fp32, trees in index order, the leaf slot's PDF added class by class, a walk
 *     that falls off adds nothing).  S is rule Q4's fp32 sum of acc in class order, label rule Q3's argmax.
 * G3. Shares.  If S > 0: q[c] = min(max(floor((acc[c] / S) * 65535.0f), 0), 65535) for every c < C -- rule Q4's expression (one
 *     IEEE divide, one multiply, rule R2's floor: saturating, NaN -> 0) per class.  Otherwise (S is 0, negative or NaN) the
 *     pixel is DEAD.
 * G4. Pool.  A pixel with S > 0: pool[i][c] += q[c] for every c, pool[i][C + label] += 1, pool[i][2 C] += 1.  A dead pixel:
 *     pool[i][2 C + 1] += 1.  The call ADDS; the caller zeroes.  Everything added is an integer: the row is the same bytes in
 *     any visiting order.
 * G5. Arguments of rdf_labels_shape_pool.  T < 1, D outside 1..30, C outside 1..RDF_POSTERIOR_MAX_CLASSES, r < 1, a negative
 *     dimension, filter_class outside -1..65535 or a misaligned pointer (2 bytes for depth and filter, 4 for forest, 8 for
 *     pool) is RDF_ERR_BAD_ARG; n_img * dim_y * dim_x >= 2^31 RDF_ERR_TOO_LARGE; zero label pixels is a successful no-op; else
 *     a NULL depth, forest or pool, or a NULL filter with filter_class != -1, is RDF_ERR_NULL_PTR.  A rejected call launches
 *     nothing and leaves pool untouched.  An accepted call is one launch on the caller's stream, nothing read back: one lane
 *     per label pixel, a wave leaves at once when none of its 64 pixels is evaluated, the sums stay in registers; the lanes of
 *     a wave that belong to one image sum their shares and counts across the wave, and lane w adds word w of the row, if it is
 *     not zero, with one 64-bit integer atomic (a wave that straddles two images does so once per image).  No
 *     floating-point atomics.
 * G6. Raw (rdf_labels_shape_decide), per frame f:  total = the sum over c < C of pool[f][c].  If pool[f][2 C] < min_pixels or
 *     total == 0: raw = -1, conf = 0.  Else raw = the first class with the greatest soft sum (best = 0; for c ascending,
 *     pool[f][c] > pool[f][best] replaces best: rule Q3's tie rule) and conf = floordiv(pool[f][raw] * 65535, total) in 64-bit
 *     integers (below 2^63 for a frame of fewer than 2^31 pixels pooled once).
 * G7. Hold, frames in index order.  valid = raw != -1 and conf >= min_conf.  Not valid: candidate = -1, run = 0, miss += 1
 *     (it stays at 2^31 - 1); if release > 0, miss >= release and held != -1: held = -1, changed = 1.  Valid: miss = 0; if raw
 *     == held: candidate = -1, run = 0; else if raw == candidate, run += 1, else candidate = raw, run = 1; then if run >=
 *     hold: held = raw, candidate = -1, run = 0, changed = 1.  changed is 0 otherwise.  out[f] = (raw, conf, held, changed)
 *     with held as it is AFTER frame f.  state is read at the start of the call and written at its end: two calls over frames
 *     [0, a) and [a, n) equal one call over [0, n).
 * G8. Arguments of rdf_labels_shape_decide.  n_frames < 0, C outside 1..RDF_POSTERIOR_MAX_CLASSES, min_pixels < 0, min_conf
 *     outside 0..65535, hold < 1, release < 0 or a misaligned pointer (8 bytes for pool, 4 for state and out) is
 *     RDF_ERR_BAD_ARG; n_frames == 0 is a successful no-op; else a NULL pointer is RDF_ERR_NULL_PTR.  A rejected call launches
 *     nothing and leaves state and out untouched.  An accepted call is one launch of one lane on the caller's stream -- the
 *     frames are a sequence, and few -- and reads nothing back.  Neither call needs a workspace.
 */
int rdf_labels_shape_pool(const uint16_t *depth, int n_img, int dim_x, int dim_y, const float *forest, int n_trees, int max_depth,
                          int n_classes, const uint16_t *filter, int filter_class, int labels_reduce, float scale_factor,
                          uint64_t *pool, void *stream);
int rdf_labels_shape_decide(const uint64_t *pool, int n_frames, int n_classes, int min_pixels, int min_conf, int hold,
                            int release, int32_t *state, int32_t *out, void *stream);

/*
 * Voted fingertips: the label route and the joint votes joined.  rdf_labels_vote_tips runs behind the mode launch of a hand's
 * chain (rdf_mean_shift_heights, rdf_mean_shift_heights_batch or rdf_labels_weighted_modes) and behind rdf_labels_votes_cast:
 * per frame and fingertip it chooses between the mode of the tip's class and the voted position of the tip's joint, finds a
 * depth for the chosen pixel and writes the tip's height where the mode launch wrote it -- a tip whose class has no pixel gets
 * a height from its vote.  The reference has no counterpart; tests/vote_tips_numpy.py restates the rules bit for bit.
 *
 *   means       float64 [n_img][L][2] = (x, y), L = num_classes: the mode finder's output, in label pixels, never flipped.
 *   class_ids   int [n_ids], 1-based classes;  tip_joints int [n_ids], a joint index each (anything outside 0 .. J - 1, -1 by
 *               convention: this tip never takes a vote).
 *   joints      int32 [n_img][J][4] = (X, Y, Z, S): rdf_labels_votes_cast's output (rule V5), in the frame the voter saw --
 *               mirrored in x when flip_x is set, as the hand's chain mirrors the left hand's frame.
 *   depth       uint16 [n_img][dim_y][dim_x]: the frame heights are looked up in (the raw camera frame, never flipped).
 *   plane       float32 [16], the calibrated plane's 4x4 matrix, row-major;  fx, fy, ppx, ppy: the depth camera.
 *   heights_out float64, heights_out[f * heights_stride + i]; what lies between the rows is not touched.
 *   tips_out    int32 [n_img][n_ids][4] = (px, py, z, source); may be NULL.
 *   floordiv and clamp as in rules V.  means and heights_out may be mapped pinned host memory.
 *
 * Per frame f and tip i:
 * T1. The mode candidate.  c = class_ids[i]; none if c is outside 1 .. L.  Else (mx, my) = means[f][c - 1]; none if either is
 *     NaN or |.| >= 1e9.  Else (pxm, pym) = (trunc(mx) * r, trunc(my) * r) with r = labels_reduce; none if that is off the
 *     frame.  Exactly the conditions under which rule S7 (rdf_fingertip_heights) gives a height.
 * T2. The vote candidate.  j = tip_joints[i]; none if j is outside 0 .. J - 1.  Else (X, Y, Z, S) = joints[f][j]; none if S
 *     <= 0, and none on a frame without pixels.  Else Xu = flip_x ? 16 * dim_x - X : X (a pixel centre is at +8, so the
 *     centre of pixel p maps to the centre of pixel dim_x - 1 - p); pxv = clamp(floordiv(Xu, 16), 0, dim_x - 1), pyv =
 *     clamp(floordiv(Y, 16), 0, dim_y - 1): the centre of a border cell can lie past the frame when the frame is no multiple
 *     of the cell.
 * T3. The choice.  RDF_TIPS_FILL: the mode if there is one, else the vote.  RDF_TIPS_GUARD: with both candidates, the mode if
 *     max(|pxm - pxv|, |pym - pyv|) <= max_dist, else the vote; with one candidate, that one.  RDF_TIPS_VOTES: the vote if
 *     there is one, else the mode.  With neither, the height is NaN and the tip (-1, -1, 0, 0): source 0.
 * T4. The depth.  From a mode: z = depth[f][pym][pxm] as it is, 0 and 65535 included, as rule S7 takes it; source 1.  From a
 *     vote, with zs = depth[f][pyv][pxv]: if zs is neither 0 nor 65535 and |zs - Z| <= z_tol, z = zs, source 2 (the tip is
 *     seen, and the sensor knows its depth better than the regression does); else z = Z, source 3 (hidden, or in a hole).
 * T5. The height.  Rule S7's arithmetic on (px, py, z): x = ((float)px - ppx) / fx and y alike in fp32, the point ((float)z * x,
 *     (float)z * y, (float)z, 1) promoted to fp64, height = -(plane[8] * pt[0] + plane[9] * pt[1] + plane[10] * pt[2] + plane[11]
 *     * pt[3]) summed from 0.0 in that order with the plane promoted to fp64.  A mode-sourced height is bit for bit what the
 *     mode launch wrote.  tips_out[f][i] = (px, py, z, source).
 * T6. Arguments.  A negative size, labels_reduce < 1, policy outside 0 .. 2, max_dist or z_tol outside 0 .. 65535,
 *     heights_stride < n_ids, n_ids or num_classes of 0, n_joints outside 1 .. RDF_VOTES_MAX_JOINTS, dim_x or dim_y above 65535
 *     or a misaligned pointer (8 bytes for means and heights_out, 4 for class_ids, tip_joints and plane, 2 for depth, 16 for
 *     joints and tips_out) is RDF_ERR_BAD_ARG; n_img * n_ids >= 2^31 or n_img * dim_y * dim_x >= 2^31 RDF_ERR_TOO_LARGE; n_img
 *     == 0 is a successful no-op; else a NULL pointer (tips_out excepted) is RDF_ERR_NULL_PTR.  A rejected call launches and
 *     writes nothing.  An accepted call is one launch on the caller's stream, one lane per (frame, tip) on a capped grid that
 *     strides over the pairs; nothing is read back.
 */
#define RDF_TIPS_FILL 0
#define RDF_TIPS_GUARD 1
#define RDF_TIPS_VOTES 2
int rdf_labels_vote_tips(const double *means, int n_img, int num_classes, const int *class_ids, const int *tip_joints,
                         int n_ids, const int32_t *joints, int n_joints, int flip_x, const uint16_t *depth, int dim_x,
                         int dim_y, int labels_reduce, float fx, float fy, float ppx, float ppy, const float *plane,
                         int policy, int max_dist, int z_tol, double *heights_out, int heights_stride,
                         int32_t *tips_out, void *stream);

int rdf_labels_abi_version(void);
const char *rdf_labels_build_id(void);
const char *rdf_labels_error_string(int code);

#ifdef __cplusplus
}
#endif

#endif /* RDF_LABELS_H */
