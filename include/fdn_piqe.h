/* fdn_piqe.h -- PIQE, the perception-based no-reference image quality evaluator (Venkatanath, Praneeth, Chandrasekhar, Channappayya,
 * Medasani: "Blind image quality evaluation using perception based features", NCC 2015; the `piqe` of MATLAB), of 8-bit images and of
 * video luma planes: the entry points of libfdn_piqe.so.  It needs no ground truth, no trained model and no data file, and it prices two
 * failure modes per 16 x 16 block: blocking / flat-segment artefacts and amplified noise.  0 is best, 100 is worst.
 *
 * THIS TEXT IS THE DEFINITION.  It is written out from the paper and from the constants MATLAB documents.  Where MATLAB's piqe differs in
 * a detail, this header wins (the known example: the gray code below is not rgb2gray's exact coefficients).  No comparison against MATLAB
 * or pyiqa has been made.
 *
 * A header of its own with a version of its own, in a library of its own built beside libfdn_hip.so: fdn_hip.h, the other headers, their
 * versions and libfdn_hip.so stand still.  Conventions as in fdn_msssim.h: raw device pointers, nothing allocated or synchronised, work
 * enqueued on `stream`, FDN_OK or an FDN_ERR_* code returned; FDN_ERR_ARG before any launch.  No memory has to be zeroed by the caller: a
 * launch writes every word it later reads.  No floating-point atomic is used, so a plane's bits do not depend on its batch neighbours or
 * on the call.
 *
 * Constants.  Block 16, activity threshold 0.1, impaired threshold 0.1, segment length 6 (11 segments per edge), C = 1.
 *
 * Plane.  An h x w array of integer codes with a divisor q; the double sample is I = (double)code / q, exact for all of these:
 *   8-bit image uint8 [B][h][w][3]: code = (299 R + 587 G + 114 B + 500) / 1000 in integer division (the integer of fdn_gmsd_u8 rounded to
 *     a code in 0 .. 255); bgr != 0: the bytes of a pixel are B, G, R.  q = 1.
 *   Video luma: the Y plane of frame f starts at sample f * stride, as fdn_msssim_luma takes it.  bits 8: uint8, q = 1.  bits 10: uint16, a
 *     code above 1023 counts as 1023, q = 4: the constants above belong to a 0 .. 255 scale, and 10 bit keeps its two extra bits as quarters.
 *
 * Padding.  H = 16 * ceil(h / 16), W = 16 * ceil(w / 16).  Position (y, x) of the padded plane, and any position the filter reaches
 * beyond it, reads sample (min(max(y, 0), h - 1), min(max(x, 0), w - 1)): padarray(., 'replicate', 'post'), then imfilter(., 'replicate').
 *
 * MSCN.  g = taps7: exp(-t^2 / (2 (7/6)^2)) for t = -3 .. 3, normalised, float64; the host passes it in.  Everything is float64, one
 * rounding per operation, no FMA contraction.
 *     row pass     r = 0, then r = r + g_t * x(y, x + t - 3) for t = 0 .. 6;
 *     column pass  m = 0, then m = m + g_t * r(y + t - 3, x) for t = 0 .. 6;
 * applied to I (giving mu) and to I * I (giving m2; the product is exact).  Then
 *     sd = sqrt(fabs(m2 - mu * mu)),   n = (I - mu) / (sd + 1.0).
 *
 * Per block, b[i][j] the block's 16 x 16 values of n, i the row.  Every sum below starts at 0.0 and adds its terms one at a time.
 *   1. Variance.  rs_i = the sum of b[i][0 .. 15] left to right; total = rs_0 + ... + rs_15 top to bottom; mean = total / 256.
 *      ds_i = the sum of (b[i][j] - mean) * (b[i][j] - mean) left to right; v = (ds_0 + ... + ds_15, top to bottom) / 255.
 *      The block is ACTIVE when v > 0.1.  An inactive block contributes nothing and has class 0.
 *   2. Noticeable distortion WNDC.  The four edges are row 0, column 15, row 15, column 0, each read in ascending index.  For each start
 *      s = 0 .. 10 the six samples e[s .. s + 5]: sum left to right, mean = sum / 6, the squared deviations summed left to right,
 *      std = sqrt(that / 5).  WNDC = 1 when any of the 44 stds is < 0.1.
 *   3. Noise WNC.  sigma = sqrt(v).  The centre is column 7 top to bottom, then column 8 top to bottom: 32 samples in ONE running sum,
 *      mean = sum / 32, the squared deviations in the same order, std_centre = sqrt(that / 31).  The surround is the other 224 samples,
 *      summed as the variance is: per row the 14 samples left to right skipping columns 7 and 8, the 16 row sums added top to bottom,
 *      mean = total / 224, the squared deviations the same way, std_surround = sqrt(that / 223).
 *      csd = std_centre / std_surround, a NaN counts as 0.  beta = fabs(sigma - csd) / fmax(sigma, csd).  WNC = sigma > 2 * beta; a
 *      comparison with NaN is false, so an infinite csd gives WNC = 0.
 *   4. d = (WNDC ? 1 - v : 0) + (WNC ? v : 0), the two terms added in that order.
 *
 * Result.  Per plane the device returns D, the sum of d over the active blocks, and NHSA, their count.  THE ORDER OF D: a tile is
 * FDN_PIQE_TILE_H x FDN_PIQE_TILE_W samples (2 x 4 blocks), tiles in row-major order over the padded plane.  A tile's partial starts at 0.0
 * and adds the d of its active blocks inside the padded plane in row-major order within the tile.  The fold has 256 slots: slot t starts at
 * 0.0 and adds the partials of tiles t, t + 256, t + 512, ... in that order; then for st = 128, 64, ..., 1 slot t < st becomes slot t +
 * slot (t + st); D is slot 0.  NHSA is an integer and exact in any order.
 * The host forms score = (D + 1) / (1 + NHSA) * 100, left to right.  A flat image has no active block and scores exactly 100.0: that is
 * the published behaviour (the score of an image PIQE has nothing to say about is its worst), not an error.
 */
#ifndef FDN_PIQE_H
#define FDN_PIQE_H

#include "fdn_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* version of this header: bumped on any signature change below */
#define FDN_PIQE_ABI_VERSION 1
int fdn_piqe_abi_version(void);

/* the block, and the tile of the kernel: FDN_PIQE_TILE_H rows by FDN_PIQE_TILE_W columns of samples per workgroup, whole blocks (its codes
 * with the 3-sample apron as uint16 and the row pass of I and I * I as doubles are about 5 KB + 39 KB of LDS; the MSCN values then take
 * the place of the row pass).  The tile sizes the workspace, fixes the order of D and is where a test looks for an edge. */
enum { FDN_PIQE_BLOCK = 16, FDN_PIQE_TILE_H = 32, FDN_PIQE_TILE_W = 64 };

/* the bits of a block's class byte: MATLAB's three masks at block resolution */
enum { FDN_PIQE_ACTIVE = 1, FDN_PIQE_WNDC = 2, FDN_PIQE_WNC = 4 };

/* dims [6] = H, W, H / 16, W / 16, tile rows, tile columns of an h x w plane.  Host arithmetic only (no HIP call: answers without a GPU);
 * dims is a HOST pointer.  FDN_ERR_ARG: dims NULL, h < 1, w < 1, H * W > 2^31 - 1. */
int fdn_piqe_dims(int h, int w, int* dims);

/* doubles of workspace the scoring entries need for B planes of h x w: two per tile; 0 = bad arguments (B < 1, h < 1, w < 1,
 * H * W > 2^31 - 1) */
long fdn_piqe_ws(int B, int h, int w);

/* The optional outputs of the two scoring entries, NULL when not wanted, P = B the number of planes:
 *   mscn     float64 [P][H][W], n at every position of the padded plane;
 *   var      float64 [P][H / 16][W / 16], v of every block;
 *   cls      uint8   [P][H / 16][W / 16], FDN_PIQE_ACTIVE | FDN_PIQE_WNDC | FDN_PIQE_WNC of every block (0 for an inactive one).
 * ws: fdn_piqe_ws(B, h, w) doubles of device memory, 8-byte aligned.  taps7: HOST pointer to the 7 taps (read before the call returns).
 * out [P][2] float64 = per plane {D, NHSA}.  One call is one tiled launch and one fold for the whole batch. */

/* img uint8 [B][h][w][3]; bgr as above.
 * FDN_ERR_ARG: img, taps7, ws or out NULL, ws not 8-byte aligned, B < 1, h < 1, w < 1, H * W > 2^31 - 1.
 * FDN_ERR_UNSUPPORTED: more workgroups than a grid holds: B times the plane's tiles above 2^24 - 1, since HIP holds a launch to 2^32 - 1
 * threads and a workgroup has 256.  FDN_ERR_LAUNCH: no device, or a launch failed. */
int fdn_piqe_u8(const unsigned char* img, int B, int h, int w, int bgr, const double* taps7, double* mscn, double* var, unsigned char* cls,
                double* ws, double* out, fdn_stream_t stream);

/* frames: B frames, the h x w Y plane of frame f at sample f * stride (stride = h * w * 3 / 2 for 4:2:0 frames); bits 8 (uint8) or 10
 * (uint16, clamped to 1023, q = 4).
 * FDN_ERR_ARG: as above, bits not 8 or 10, stride < h * w.  FDN_ERR_UNSUPPORTED, FDN_ERR_LAUNCH: as above. */
int fdn_piqe_luma(const void* frames, int B, int h, int w, int bits, long stride, const double* taps7, double* mscn, double* var,
                  unsigned char* cls, double* ws, double* out, fdn_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
