/* fdn_temporal.h -- video across frames: the entry points of libfdn_hip.so that keep the brightness ratio FDN is fed steady from one
 * frame of a stream to the next.  LPNet predicts the ratio from one frame alone; on noisy low-light footage the prediction moves with
 * the noise and the output flickers.  fdn_luma_hist takes a luma histogram of every codec frame, fdn_ratio_smooth filters the ratio
 * causally (an exponential moving average) and starts afresh at a scene cut, which it finds by the distance between the histograms
 * of neighbouring frames.  A header of its own with a version of its own, as include/fdn_video.h: fdn_hip.h, fdn_video.h and their
 * versions stand still.  Conventions as in fdn_hip.h: raw device pointers, nothing allocated or synchronised, work enqueued on
 * `stream`, FDN_OK or an FDN_ERR_* code returned.  (The reference reads PNGs only: no counterpart.)
 */
#ifndef FDN_TEMPORAL_H
#define FDN_TEMPORAL_H

#include "fdn_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* words of the filter's carried state in device memory, all uint32:
 *   [0 .. 255] the luma histogram of the last frame seen;
 *   [256]      the bits of the last finite filtered ratio (fp32);
 *   [257]      flags: bit 0 "has a frame" (words 0 .. 255 are valid), bit 1 "has a ratio" (word 256 is valid).
 * All zeros is the reset state: the caller resets a stream by zero-filling the words. */
#define FDN_TEMPORAL_STATE_WORDS 258

/* version of this header: bumped on any signature change below */
#define FDN_TEMPORAL_ABI_VERSION 1
int fdn_temporal_abi_version(void);

/* frames, as fdn_pre_yuv420 takes them: B contiguous frames of h * w * 3 / 2 samples; bits 8: uint8, 10: little-endian uint16 with the
 * value in the low bits -> hist [B][256] uint32, the histogram of each frame's luma plane.  Only the first h * w samples of a frame are
 * read, so planar and semi-planar frames need no flag.  The bin of a sample is code >> (bits - 8); a 10-bit word above 1023 counts as
 * 1023.  hist is overwritten (cleared on `stream` here, not by the caller); every row sums to h * w.
 * FDN_ERR_ARG before any launch: a NULL pointer, B < 1, B >= 65536, h or w odd or < 2, bits not 8 / 10, h * w >= 2^30 (so that the
 * distance between two histograms, at most 2 h w, fits an int). */
int fdn_luma_hist(const void* frames, unsigned* hist, int B, int h, int w, int bits, fdn_stream_t stream);

/* hist [B][256] of B frames in stream order, ratio [B] fp32, state [FDN_TEMPORAL_STATE_WORDS] -> ratio_out [B] fp32, dist [B] uint32,
 * cut [B] int32, and the state advanced by B frames; one launch.  For t = 0 .. B - 1, with the previous histogram that of frame t - 1, or
 * the state's for t = 0:
 *   dist[t] = sum_i |hist[t][i] - previous[i]|, in integers; 0 when there is no previous frame;
 *   cut[t]  = 1 when there is no previous frame or dist[t] > cut_above, else 0;
 *   ratio_out[t] = ratio[t] when cut[t] is set or the state has no ratio, else prev + alpha * (ratio[t] - prev) in fp32, the subtraction,
 *   the product and the sum each rounded once (no FMA contraction), prev the last finite filtered ratio.  alpha = 1 hands ratio[t] out
 *   as it is (in fp32 prev + (ratio[t] - prev) need not give ratio[t] back): nothing is filtered, cuts are still found.
 * A non-finite ratio[t] (or result) is handed out as it is and does not enter the state: the next frame filters against the last finite
 * value, also across a cut that fell on such a frame.  The histogram part of the state advances regardless.  ratio_out may be ratio.
 * FDN_ERR_ARG before any launch: a NULL pointer, B < 1, B >= 65536, alpha not in (0, 1], cut_above < 0. */
int fdn_ratio_smooth(const unsigned* hist, const float* ratio, unsigned* state, float alpha, int cut_above, int B, float* ratio_out,
                     unsigned* dist, int* cut, fdn_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
