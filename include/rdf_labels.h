/*
 * rdf_labels.h -- C ABI of librdf_labels.so: colour-glove recordings to training labels on MI355X (gfx950).  The kernels
 * behind the reference's src/live_data_convert.py: split_pixels_by_nearest_color, apply_point_mapping and
 * depths_from_points (src/cuda/points_ops.cu:207-255, 167-205, 39-63), the whole of its make_color_mapping
 * (live_data_convert.py:156-204) as device work, and the per-frame labelling of its tick() (:413-458) as one pass.
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
 * Arithmetic is integer throughout, so every result is independent of the order in which pixels are visited:
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

/* 1: first version. */
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

int rdf_labels_abi_version(void);
const char *rdf_labels_build_id(void);
const char *rdf_labels_error_string(int code);

#ifdef __cplusplus
}
#endif

#endif /* RDF_LABELS_H */
