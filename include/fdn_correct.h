/* fdn_correct.h -- brightness-corrected PSNR / SSIM of 8-bit image pairs: the entry points of libfdn_correct.so, which score a restored
 * image after an affine correction per channel towards its ground truth.  The coefficients are the host's (fdn_hip/correct.py):
 *   mean_var  every channel of the restored image shifted and scaled to the ground truth's mean and standard deviation, what the
 *             reference's scripts/metrics/calculate_psnr_ssim.py does under --correct_mean_var (:38-54; in exact arithmetic its "correct
 *             twice" is one affine map);
 *   gt_mean   the restored image times mean(gray(gt)) / mean(gray(restored)), clipped to [0, 255] (the --GT_mean convention of KinD, LLFlow
 *             and Retinexformer; not in the reference).
 * A header of its own with a version of its own, in a library of its own built beside libfdn_hip.so: fdn_hip.h, the other headers, their
 * versions and libfdn_hip.so stand still.  Conventions as in fdn_hip.h: raw device pointers, nothing allocated or synchronised, work
 * enqueued on `stream`, FDN_OK or an FDN_ERR_* code returned; FDN_ERR_ARG before any launch.  No floating-point atomic is used and every
 * sum is a fixed tree: an image's result does not depend on the other images of the batch and has the same bits on every call.
 *
 * images: gt, restored uint8 [B][h][w][3], as fdn_post_u8 writes them and fdn_pair_*_u8 take them.  crop: pixels cut from every edge
 * before scoring.  The statistics and the correction are of the WHOLE image (the reference corrects before it crops).
 *
 * coef [B][3][5] doubles on the device, per image and per channel (in the byte order of a pixel): m_r, s, m_g, lo, hi.  The corrected
 * sample of a byte x of `restored` is, in double with one rounding per operation and no FMA contraction,
 *     t = (double)x - m_r;  t = t * s;  t = t + m_g;  t = t < lo ? lo : t;  t = t > hi ? hi : t;  z = (float)t
 * in code units 0 .. 255.  A NaN coefficient gives NaN samples, hence NaN scores for that image alone.
 *
 * FDN_ERR_ARG of every entry point that takes them: a NULL pointer, B < 1, B > 65535, h < 1, w < 1, h * w > 2^31 - 1; with a crop also
 * crop < 0, h <= 2 crop, w <= 2 crop.  FDN_ERR_LAUNCH: no device, or a launch failed.
 */
#ifndef FDN_CORRECT_H
#define FDN_CORRECT_H

#include "fdn_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* version of this header: bumped on any signature change below */
#define FDN_CORRECT_ABI_VERSION 1
int fdn_correct_abi_version(void);

/* int64 words per part of fdn_pair_moments_u8 and per image of fdn_pair_moments_fold, with S = sum x, Q = sum x^2 over the whole image
 * and c the channel:  [c] S of gt, [3 + c] Q of gt, [6 + c] S of restored, [9 + c] Q of restored, [12] the maximum of gt over the
 * cropped region (it picks the peak value and the SSIM constants, as the maximum of fdn_pair_sse_u8 does). */
enum { FDN_PAIR_MOMENTS = 13 };

/* moments [B][FDN_PAIR_PARTS][FDN_PAIR_MOMENTS] int64: part p of image b covers the rows p, p + FDN_PAIR_PARTS, ... of the whole image.
 * Integers, so the sums are exact in any order; 64-bit, so no image that fits in memory overflows them.
 * FDN_ERR_ARG: gt, restored or moments NULL, B < 1, B > 65535, h < 1, w < 1, h * w > 2^31 - 1, crop < 0, h <= 2 crop, w <= 2 crop. */
int fdn_pair_moments_u8(const unsigned char* gt, const unsigned char* restored, int B, int h, int w, int crop, long* moments,
                        fdn_stream_t stream);

/* folded [B][FDN_PAIR_MOMENTS] int64: the sums (the maximum for [12]) of an image's FDN_PAIR_PARTS parts, what the host copies back to
 * form the coefficients.  FDN_ERR_ARG: moments or folded NULL, B < 1, B > 65535. */
int fdn_pair_moments_fold(const long* moments, int B, long* folded, fdn_stream_t stream);

/* doubles of workspace fdn_pair_corrected_u8 needs: two per 32 x 32 tile of the cropped images; 0 = bad arguments (those of
 * fdn_pair_corrected_u8) */
long fdn_pair_corrected_ws(int B, int h, int w, int crop);

/* out2 [B][2] doubles = {sum over the cropped region and the three channels of (gt - (double)z)^2, mean of the 3-D SSIM map of (gt, z)}:
 * calculate_psnr's sum before the division and calculate_ssim (ssim3d=True) of basicsr/metrics/psnr_ssim.py on img1 = gt, img2 = z.
 * One tiled launch over (tiles, B) on the bytes (32 x 32 tiles, 42 x 42 apron, replicate padding at the cropped border; z is formed
 * when the apron is loaded and never stored), float32 maps with the roundings of fdn_pair_ssim3d_u8, then a per-image finish that folds
 * the tiles' partial sums in a fixed order.
 *   is255 [B] int32 on the device: != 0 picks the SSIM constants of peak value 255, 0 those of peak value 1 (gt.max() <= 1);
 *   taps11, chmix9: HOST pointers, as fdn_pair_ssim3d_u8 takes them;  ws: fdn_pair_corrected_ws(B, h, w, crop) doubles.
 * FDN_ERR_ARG: any pointer NULL, B < 1, B > 65535, h < 1, w < 1, h * w > 2^31 - 1, crop < 0, h <= 2 crop, w <= 2 crop. */
int fdn_pair_corrected_u8(const unsigned char* gt, const unsigned char* restored, int B, int h, int w, int crop, const double* coef,
                          const int* is255, const double* taps11, const double* chmix9, double* ws, double* out2, fdn_stream_t stream);

/* out [B][3][h][w] float32 = z, the corrected image as planes in the byte order of a pixel: for callers who want the image, and for the
 * branches scored plane by plane (test_y_channel, ssim3d=False).
 * FDN_ERR_ARG: restored, coef or out NULL, B < 1, B > 65535, h < 1, w < 1, h * w > 2^31 - 1. */
int fdn_pair_apply_u8(const unsigned char* restored, const double* coef, int B, int h, int w, float* out, fdn_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
