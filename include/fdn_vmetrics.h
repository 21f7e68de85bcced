/* fdn_vmetrics.h -- video evaluation straight from codec samples: the entry points of libfdn_hip.so that score a stream of Y'CbCr 4:2:0
 * frames against a ground-truth stream without a detour through 8-bit RGB - squared errors per plane (PSNR), luma sums (mean luma and
 * brightness flicker) and SSIM on luma, the reference's _ssim_cly (basicsr/metrics/psnr_ssim.py:202-240) applied to the luma codes.
 * A header of its own with a version of its own, as include/fdn_video.h and include/fdn_temporal.h: fdn_hip.h, fdn_video.h,
 * fdn_temporal.h and their versions stand still.  Conventions as in fdn_hip.h: raw device pointers, nothing allocated or synchronised,
 * work enqueued on `stream`, FDN_OK or an FDN_ERR_* code returned.
 *
 * frames, as fdn_pre_yuv420 takes them: B contiguous frames of h * w * 3 / 2 samples each; h and w even.
 *   bits   8: samples are uint8;  10: little-endian uint16 with the value in the low bits; a 10-bit word above 1023 counts as 1023.
 *   layout 0: planar, Y [h][w] then U [h/2][w/2] then V [h/2][w/2];  1: semi-planar, Y [h][w] then UV [h/2][w/2][2], 8 bit only.
 * A frame starts at b * h * w * 3 / 2 samples: no alignment beyond that of a sample is assumed.
 *
 * FDN_ERR_ARG before any launch: a NULL pointer where one is required, B < 1, B >= 65536, h or w odd or < 2, bits not 8 / 10, layout
 * not 0 / 1, layout 1 with bits 10, h * w >= 2^30.
 */
#ifndef FDN_VMETRICS_H
#define FDN_VMETRICS_H

#include "fdn_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* version of this header: bumped on any signature change below */
#define FDN_VMETRICS_ABI_VERSION 1
int fdn_vmetrics_abi_version(void);

/* frames a, b -> stats [B][5] int64 = { SSE_Y, SSE_Cb, SSE_Cr, sum of a's luma codes, sum of b's luma codes } per frame pair: the sums
 * of squared code differences over each plane (for layout 1 the interleaved plane gives the two sums the planar planes give) and the
 * sums of the luma codes.  All integer, accumulated in 64 bits: exact, whatever the order.  stats is overwritten (cleared on `stream`
 * here, not by the caller).  b == NULL: single-stream use - only word 3 is computed, the others are written as 0. */
int fdn_yuv420_pair_stats(const void* a, const void* b, long* stats, int B, int h, int w, int layout, int bits, fdn_stream_t stream);

/* doubles of workspace fdn_yuv420_ssim_y needs (one partial per tile and frame); 0 = bad arguments */
long fdn_yuv420_ssim_y_ws(int B, int h, int w);

/* frames a, b -> out [B] float64 = the mean over all h * w pixels of the SSIM map of the two luma planes (chroma is never read, so the
 * layout needs no flag): the 11 x 11 Gaussian window outer(taps11, taps11) over a, b, a^2, b^2 and a b with the border replicated, no
 * valid-region crop, C1 = (0.01 L)^2, C2 = (0.03 L)^2, L = 2^bits - 1; float64 from the integer codes on.  For 8 bit this is the
 * reference's _ssim_cly on the Y plane.  The map is summed in a fixed order - per-tile partials in ws, then one fixed fold - so a frame's
 * score has the same bits on every call, in every slot of a batch, next to whatever other frames.
 *   ws:     fdn_yuv420_ssim_y_ws(B, h, w) doubles of device memory;
 *   taps11: HOST pointer, cv2.getGaussianKernel(11, 1.5) in float64 (read before the call returns). */
int fdn_yuv420_ssim_y(const void* a, const void* b, double* out, double* ws, const double* taps11, int B, int h, int w, int bits,
                      fdn_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
