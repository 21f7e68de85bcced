/* fdn_sharpness.h -- deblurring evaluation of 8-bit image pairs: the entry points of libfdn_sharpness.so, which measure what the blur
 * half of FDN's job is judged by.  a is the ground truth, b the restored image.
 *   edge   the reference's EdgeLoss (basicsr/models/losses/losses.py:661-687) as an evaluation figure, exact up to one square root;
 *   GMSD   gradient magnitude similarity deviation (Xue, Zhang, Mou, Bovik 2014, as their MATLAB code);
 *   mean gradient   the sharpness of each image on its own, on GMSD's grid and from the same launch.
 * A header of its own with a version of its own, in a library of its own built beside libfdn_hip.so: fdn_hip.h, the other headers, their
 * versions and libfdn_hip.so stand still.  Conventions as in fdn_lowlight.h: raw device pointers, nothing allocated or synchronised, work
 * enqueued on `stream`, FDN_OK or an FDN_ERR_* code returned; FDN_ERR_ARG before any launch.  No memory has to be zeroed by the caller: a
 * launch writes every word it later reads.  No floating-point atomic is used: sums run as per-tile partials in the workspace (a fixed
 * tree over the tile's threads), then one fold per image in a fixed order, so an image's result does not depend on the other images of
 * the batch and has the same bits on every call.
 *
 * images: uint8 [B][h][w][3], as fdn_post_u8 writes them and fdn_pair_*_u8 take them.
 *
 * Edge error.  The reference computes mean sqrt((L(x) - L(y))^2 + 1e-6) with L(x) = x - G(U(G(x))) on images in [0, 1]: G the 5 x 5
 * separable filter [.05 .25 .4 .25 .05] with replicate padding, U keeps even rows and even columns times 4 and zeroes the rest.  L is
 * linear, so only d = a - b is needed, an integer in [-255, 255] per channel, and with the weights written k / 20, k = [1 5 8 5 1],
 * everything up to the square root is an integer.  Per channel, clamp(.) clamping a coordinate into the image:
 *     F(q) = sum over the 5 x 5 window of k_i k_j d(clamp(q + (i, j)))                    (400 G(d))
 *     Z(q) = 4 F(q) where both coordinates of q are even, else 0
 *     N(p) = 160000 d(p) - sum over the 5 x 5 window of k_i k_j Z(clamp(p + (i, j)))
 * The second filter's replicate padding acts on the zero-stuffed field: a padded coordinate takes the value at its clamped coordinate,
 * which is non-zero only if that coordinate is even in both axes (the last row replicates as non-zero when h - 1 is even, as zero when it
 * is odd).  |N| <= 204000000, so int32 holds it.  The residual is N / 40800000 (160000 * 255), the error of an element
 *     e = sqrt((N / 40800000.0)^2 + 1e-6)       in double,
 * and the figure of an image the sum of e over its 3 h w elements divided by 3 h w (the host divides).  The reference's mean runs over
 * the whole batch; the batch mean of these per-image values is that mean for images of equal size.  The channel order does not matter.
 *
 * GMSD.  Gray y = 299 R + 587 G + 114 B, an integer, 1000 times the luma.  Grid hd = (h + 1) / 2, wd = (w + 1) / 2 (rounded down).
 * Block sum s(i, j) = the sum of y over rows 2i, 2i + 1 and columns 2j, 2j + 1, samples outside the image counting 0 (MATLAB's
 * conv2(., ones(2) / 4, 'same') followed by (1:2:end, 1:2:end), times 4000).  Prewitt on s with zero outside the grid:
 *     gx(i, j) = sum over r = -1 .. 1 of s(i + r, j + 1) - s(i + r, j - 1),     gy the same, transposed,
 *     A = gx^2 + gy^2, exact in int64                                           ((12000 m)^2, m the paper's gradient magnitude)
 * and with T' = 170 * 144e6 = 24480000000
 *     q = (2 sqrt((double)A_a * (double)A_b) + T') / (double)(A_a + A_b + T')   in double, one rounding per operation;
 * the denominator is an exact integer below 2^53.  Equal images give q == 1.0 exactly.  GMSD is the sample standard deviation (n - 1,
 * MATLAB's std2) of q over the n = hd wd grid points: the device returns the sums of q and of q^2, the host forms
 * sqrt(max(0, (S2 - S1^2 / n) / (n - 1))), exactly 0.0 for equal images.
 *
 * Mean gradient.  m = sqrt((double)A) / 12000 on the same grid; the device returns the sums of m of a and of b, the host divides by n.
 */
#ifndef FDN_SHARPNESS_H
#define FDN_SHARPNESS_H

#include "fdn_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* version of this header: bumped on any signature change below */
#define FDN_SHARPNESS_ABI_VERSION 1
int fdn_sharpness_abi_version(void);

/* the tiles of the two kernels: FDN_EDGE_TILE x FDN_EDGE_TILE pixels, FDN_GMSD_TILE x FDN_GMSD_TILE grid points.  They size the workspaces
 * and are where a test looks for an edge. */
enum { FDN_EDGE_TILE = 32, FDN_GMSD_TILE = 32 };

/* doubles of workspace fdn_edge_u8 needs: one per tile of every image; 0 = bad arguments (B < 1, h < 1, w < 1, h * w > 2^31 - 1) */
long fdn_edge_ws(int B, int h, int w);

/* a, b [B][h][w][3] -> out [B] float64 = the sum of e over the image's 3 h w elements.  resid: NULL, or int32 [B][h][w][3] = N of every
 * element.  One tiled launch (a tile of d with a 4-pixel apron in LDS, F at the even-even points only) and the fold.
 *   ws: fdn_edge_ws(B, h, w) doubles of device memory, 8-byte aligned.
 * FDN_ERR_ARG: a, b, ws or out NULL, ws not 8-byte aligned, B < 1, h < 1, w < 1, h * w > 2^31 - 1.
 * FDN_ERR_UNSUPPORTED: B * tiles > 2^31 - 1 (more workgroups than a grid holds).  FDN_ERR_LAUNCH: no device, or a launch failed. */
int fdn_edge_u8(const unsigned char* a, const unsigned char* b, int B, int h, int w, int* resid, double* ws, double* out,
                fdn_stream_t stream);

/* hd, wd = GMSD's grid of an h x w image (the rule above).  Host arithmetic only (no HIP call: answers without a GPU); hd, wd are HOST
 * pointers.  FDN_ERR_ARG: a NULL pointer, h < 1, w < 1, h * w > 2^31 - 1. */
int fdn_gmsd_dims(int h, int w, int* hd, int* wd);

/* doubles of workspace fdn_gmsd_u8 needs: four per tile of every image's grid; 0 = bad arguments (B < 1, h < 1, w < 1,
 * h * w > 2^31 - 1, hd * wd < 2) */
long fdn_gmsd_ws(int B, int h, int w);

/* a, b [B][h][w][3] -> out [B][4] float64 = {sum of q, sum of q^2, sum of m of a, sum of m of b} over the image's n = hd wd grid points.
 * bgr != 0: the bytes of a pixel are B, G, R, else R, G, B.  grad2: NULL, or int64 [B][2][hd][wd] = A of a and of b.  map: NULL, or
 * float32 [B][hd][wd] = q rounded once.  One tiled launch (a tile of s with a 1-point apron in LDS, from the 2 x 2 byte blocks) and the fold.
 *   ws: fdn_gmsd_ws(B, h, w) doubles of device memory, 8-byte aligned.
 * FDN_ERR_ARG: a, b, ws or out NULL, ws not 8-byte aligned, B < 1, h < 1, w < 1, h * w > 2^31 - 1, hd * wd < 2 (a standard deviation
 * of one point).  FDN_ERR_UNSUPPORTED: B * tiles > 2^31 - 1.  FDN_ERR_LAUNCH: no device, or a launch failed. */
int fdn_gmsd_u8(const unsigned char* a, const unsigned char* b, int B, int h, int w, int bgr, long* grad2, float* map, double* ws,
                double* out, fdn_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
