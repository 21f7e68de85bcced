/* fdn_mctf.h -- motion-compensated temporal denoising of enhanced video: the entry point of libfdn_mctf.so.  fdn_motion.h measures what
 * the ratio filter of fdn_temporal.h leaves behind - boiling noise, local tone shifts, deblurring that lands differently from frame to
 * frame; this filters it: a recursive temporal filter on the enhanced fp32 R'G'B' frames, before the one rounding to codec samples, along
 * the block vectors fdn_motion_search writes.  The prediction is overlapped between the four nearest blocks, so the 16 x 16 grid does not
 * show; the filter switches itself off per pixel where the prediction does not fit and per frame at a scene cut.  Every operation is
 * ordered and rounded once in fp32 (no FMA contraction), so a float32 restatement equals the device bit for bit.
 * A header of its own with a version of its own, in a library of its own built beside libfdn_hip.so, as fdn_motion.h: fdn_hip.h, the
 * other headers, their versions and libfdn_hip.so stand still.  Conventions as in fdn_motion.h: raw device pointers, nothing allocated
 * or synchronised, work enqueued on `stream`, FDN_OK or an FDN_ERR_* code returned.
 *
 * Definition, per frame b of the batch and per pixel p = (y, x) of its top-left h x w.  nby = ceil(h / 16), nbx = ceil(w / 16) as in
 * fdn_motion.h; P is the predecessor: out[b - 1] for b > 0, `prev` for b = 0.
 *   1. c      = fminf(fmaxf(cur, 0), 1) per channel (a NaN becomes 0).
 *   2. bypass   with no predecessor (b = 0 and prev NULL), or with stats[b][0] > cut_limit (a scene cut: an integer comparison on the
 *               device, nothing synchronised):  out = c,  k = 0  everywhere.
 *   3. pred     along y:  b0 = floor((y - 8) / 16),  b1 = b0 + 1,  both clamped to [0, nby - 1];  r = (y + 8) mod 16,
 *               wy1 = (2 r + 1) / 32,  wy0 = 1 - wy1 (both exact);  the same along x.  Per channel, starting from pred = 0 and in the order
 *               (by0, bx0), (by0, bx1), (by1, bx0), (by1, bx1), all four always taken:
 *                   pred = pred + (wy * wx) * P(clamp(y + dy, 0, h - 1), clamp(x + dx, 0, w - 1))
 *               with (dy, dx) that block's vector.  wy * wx is a multiple of 1 / 1024, hence exact; the product and the sum round once
 *               each.  y + dy and x + dx are formed in int, so any short keeps the read inside the frame.
 *   4. d(p)   = fmaxf(fmaxf(|c_0 - pred_0|, |c_1 - pred_1|), |c_2 - pred_2|).
 *   5. D(p)   = s * (1.0f / 9.0f),  s the sum of d over the 3 x 3 neighbourhood of p with a replicated border, taken row-major
 *               (y - 1, x - 1), (y - 1, x), ... (y + 1, x + 1) starting from 0.
 *   6. t      = D * inv_threshold;   k = strength * fmaxf(1 - t * t, 0).
 *   7. out_c  = c_c + k * (pred_c - c_c).
 *
 * FDN_ERR_ARG before any launch: a NULL cur, mv, stats or out; B < 1 or B >= 65536; h or w < 1, H < h, W < w, h * w >= 2^30; strength
 * outside [0, 1] (a NaN is outside); inv_threshold not finite or <= 0; cut_limit < 0.  FDN_ERR_LAUNCH: no device, or a launch failed.
 */
#ifndef FDN_MCTF_H
#define FDN_MCTF_H

#include "fdn_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* version of this header: bumped on any signature change below */
#define FDN_MCTF_ABI_VERSION 1
int fdn_mctf_abi_version(void);

/* cur   float [B][3][H][W], the forward's result; only the top-left h x w of every plane is read
 * prev  float [3][h][w] dense: the FILTERED frame before frame 0;                                NULL: none
 * mv    short [B][nby][nbx][2] = (dy, dx), as fdn_motion_search writes it; read as given
 * stats long  [B][4] of fdn_motion_search; only word 0 (the sum of the chosen SADs) is read
 * out   float [B][3][h][w] dense; must not overlap cur or prev
 * kmap  float [B][h][w], the weight k of every pixel;                                            NULL: not wanted
 * Frame i > 0 is filtered against out[i - 1], so the B launches are enqueued one after the other on `stream`. */
int fdn_mctf_blend(const float* cur, const float* prev, const short* mv, const long* stats, float* out, float* kmap, int B, int h, int w,
                   int H, int W, float strength, float inv_threshold, long cut_limit, fdn_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
