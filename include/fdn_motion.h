/* fdn_motion.h -- motion-compensated temporal consistency for video evaluation: the entry points of libfdn_motion.so.  The one temporal
 * figure of fdn_vmetrics.h, flicker, is the change of a frame's MEAN luma: it sees a global brightness pump and nothing local - boiling
 * noise, local tone shifts, deblurring that lands differently from frame to frame.  A plain frame difference charges camera and object
 * motion to the method.  Here the motion is taken from a guide stream (the ground truth, as a rule) by full-search block matching on
 * luma, and the frame-to-frame change of a stream is measured along those vectors.  Everything is an integer: exact, whatever the order.
 * A header of its own with a version of its own, in a library of its own built beside libfdn_hip.so, as fdn_fusion.h: fdn_hip.h, the
 * other headers, their versions and libfdn_hip.so stand still.  Conventions as in fdn_vmetrics.h: raw device pointers, nothing allocated
 * or synchronised, work enqueued on `stream`, FDN_OK or an FDN_ERR_* code returned.
 *
 * frames: B contiguous 4:2:0 frames of h * w * 3 / 2 samples each, h and w even.  Only the luma plane [h][w] at the start of each frame
 * is read, so the chroma layout needs no flag.  bits 8: samples are uint8;  10: little-endian uint16, a word above 1023 counts as 1023.
 * A frame starts at b * h * w * 3 / 2 samples: no alignment beyond that of a sample is assumed.
 *
 * Definitions.
 *   blocks      the luma plane is cut into 16 x 16 blocks from the top-left corner: nby = ceil(h / 16) rows of nbx = ceil(w / 16).  A
 *               block at the right or bottom edge holds only its pixels inside the frame.
 *   candidates  the displacements d = (dy, dx) of [-R, R]^2, R = radius.
 *   cost        SAD(b, d) = sum over the block's pixels (y, x) of |cur(y, x) - prev(clamp(y + dy, 0, h - 1), clamp(x + dx, 0, w - 1))|:
 *               the border is replicated.
 *   choice      the block's vector is the candidate with the smallest (SAD, dy^2 + dx^2, dy, dx) in lexicographic order: the lowest cost;
 *               among equals the shortest vector, then the smaller dy, then the smaller dx.  (A SAD is at most 256 * 1023 < 2^18 and the
 *               33^2 = 1089 candidates of R = 16, ranked in that order, need 11 bits: SAD << 11 | rank is a 29-bit key, a candidate of a
 *               smaller R keeps its place among them, and one unsigned min-reduction decides, the same on every call.)
 *   sign        a block at p in frame t matches p + d in frame t - 1: content that moved by +s gives d = -s.
 *   predecessor frame i > 0 of a batch is held against frame i - 1 of the batch, frame 0 against the one frame `*_prev` points to.
 *
 * FDN_ERR_ARG before any launch: a NULL pointer where one is required, B < 1, B >= 65536, h or w odd or < 2, h * w >= 2^30, bits not
 * 8 / 10, radius outside 0 .. 16, exactly one of frames_prev and guide_prev NULL.  FDN_ERR_LAUNCH: no device, or a launch failed.
 */
#ifndef FDN_MOTION_H
#define FDN_MOTION_H

#include "fdn_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* version of this header: bumped on any signature change below */
#define FDN_MOTION_ABI_VERSION 1
int fdn_motion_abi_version(void);

/* the side of a block and the largest search radius */
enum { FDN_MOTION_BLOCK = 16, FDN_MOTION_MAX_RADIUS = 16 };

/* guide -> the block vectors of every frame against its predecessor.
 *   mv    short    [B][nby][nbx][2] = (dy, dx);                                             NULL: not wanted
 *   sad   unsigned [B][nby][nbx][2] = { SAD of the chosen vector, SAD of the zero vector };  NULL: not wanted
 *   stats long     [B][4] = { sum of the chosen SADs, sum of the zero-vector SADs, sum of |dy| + |dx|, blocks with a non-zero vector };
 *         required; cleared on `stream` here, not by the caller.
 * guide_prev NULL: frame 0 has no predecessor, its rows of mv, sad and stats are written as 0. */
int fdn_motion_search(const void* guide, const void* guide_prev, short* mv, unsigned* sad, long* stats, int B, int h, int w, int bits,
                      int radius, fdn_stream_t stream);

/* With m(p) the vector in mv of the block p lies in:  rD(p) = frames_t(p) - frames_{t-1}(clamp(p + m(p))), rG(p) the same on the guide.
 *   stats long [B][5] = { sum |rD|, sum rD^2, sum |rG|, sum rG^2, sum (rD - rG)^2 } over all h * w pixels; cleared on `stream` here.
 * mv is read as given (any short: the clamp keeps every read inside the frame).  guide == frames with guide_prev == frames_prev is
 * allowed: words 2 - 3 then equal words 0 - 1 and word 4 is 0.  Both prevs NULL: frame 0's row is 0.  The search is an entry point of
 * its own so that one search on the ground truth serves any number of scored streams. */
int fdn_motion_residual(const void* frames, const void* frames_prev, const void* guide, const void* guide_prev, const short* mv,
                        long* stats, int B, int h, int w, int bits, fdn_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
