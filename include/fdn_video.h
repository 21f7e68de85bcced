/* fdn_video.h -- video frames in and out of the FDN path: the entry points of libfdn_hip.so between a decoder's or encoder's
 * Y'CbCr 4:2:0 frame layout and the network's fp32 R'G'B' planes.  A header of its own with a version of its own, so that
 * include/fdn_hip.h and its ABI version stand still while this part grows.  Conventions as in fdn_hip.h: raw device pointers,
 * nothing allocated or synchronised, work enqueued on `stream`, FDN_OK or an FDN_ERR_* code returned.  (The reference reads PNGs
 * only: no counterpart.)
 *
 * frames: B contiguous frames of h * w * 3 / 2 samples each; h and w even.
 *   bits   8: samples are uint8;  10: little-endian uint16 with the value in the low bits (ffmpeg's yuv420p10le).
 *   layout 0: planar, Y [h][w] then U [h/2][w/2] then V [h/2][w/2] (yuv420p);
 *          1: semi-planar, Y [h][w] then UV [h/2][w/2][2] (nv12), 8 bit only.
 *   matrix 0: BT.601 (Kr 0.299, Kb 0.114);  1: BT.709 (Kr 0.2126, Kb 0.0722);  Kg = 1 - Kr - Kb.
 *   full_range 0: Y' = (y - 16 s) / (219 s), C = (c - 128 s) / (224 s) with s = 2^(bits - 8);
 *              1: Y' = y / (2^bits - 1), C = (c - 2^(bits - 1)) / (2^bits - 1).
 *   chroma_loc 0: left - chroma sample k sits on luma column 2 k (H.264 / HEVC default);  1: center - on luma column 2 k + 0.5
 *              (JPEG / MPEG-1).  Vertically chroma row j sits on luma row 2 j + 0.5 in both.
 *
 * FDN_ERR_ARG before any launch: a NULL pointer, B < 1, h or w odd or < 2, bits not 8 / 10, layout 1 with bits 10, layout, matrix,
 * full_range or chroma_loc outside {0, 1}, H < h, W < w, B >= 65536; fdn_pre_yuv420 also H - h >= h, W - w >= w (reflect padding needs
 * pad < size) and H >= 65536; fdn_post_yuv420 also h >= 65536.
 */
#ifndef FDN_VIDEO_H
#define FDN_VIDEO_H

#include "fdn_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* version of this header: bumped on any signature change below */
#define FDN_VIDEO_ABI_VERSION 1
int fdn_video_abi_version(void);

/* frames -> out [B][3][H][W] fp32 R', G', B' in [0, 1].  Output pixel (y, x) is the conversion at source position (sy, sx), reflected
 * bottom / right as fdn_pre_u8 reflects (sy = y < h ? y : 2 (h - 1) - y), so the padding is the reflection of the converted image.
 *   - a 10-bit code above 1023 counts as 1023;
 *   - chroma is interpolated bilinearly at the luma position, indices clamped at the frame's edge: vertically weights 3/4 (row sy / 2)
 *     and 1/4 (the row above for even sy, below for odd); horizontally, left: even sx takes sample k = sx / 2, odd sx the mean of k and
 *     k + 1; center: 3/4 and 1/4 as vertically.  The weighted sum of the codes is formed in integers, so it is exact;
 *   - R = Y' + 2 (1 - Kr) Cr, B = Y' + 2 (1 - Kb) Cb, G = Y' - (2 Kb (1 - Kb) / Kg) Cb - (2 Kr (1 - Kr) / Kg) Cr, the constants
 *     computed in double and rounded once to fp32, every operation rounded once (no FMA contraction);
 *   - R, G, B are clamped to [0, 1]: a legal code triple outside the RGB gamut would otherwise hand FDN's 1 - pow(1 - x, .) a negative
 *     base, i.e. NaN through the whole frame. */
int fdn_pre_yuv420(const void* frames, float* out, int B, int h, int w, int H, int W, int layout, int bits, int matrix, int full_range,
                   int chroma_loc, fdn_stream_t stream);

/* res [B][3][H][W] fp32 -> frames: crop [:h, :w], clamp R, G, B to [0, 1], Y' = Kr R + Kg G + Kb B, Cb = (B - Y') / (2 (1 - Kb)),
 * Cr = (R - Y') / (2 (1 - Kr)); chroma is downsampled from the cropped region only (the padding is never read): the mean of the two rows,
 * then, left: (c[2k-1] + 2 c[2k] + c[2k+1]) / 4 with the column clamped to the frame; center: the mean of the two columns; scaled back by
 * the inverse of the formulas above, rintf (half to even), clamped to [0, 2^bits - 1].  Every operation rounded once (no FMA contraction). */
int fdn_post_yuv420(const float* res, void* frames, int B, int h, int w, int H, int W, int layout, int bits, int matrix, int full_range,
                    int chroma_loc, fdn_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
