/* fdn_ensemble.h -- geometric self-ensemble around the FDN forward: the entry points of libfdn_hip.so that make the flipped and
 * transposed copies of a frame and fold the network's results on them back into one.  A header of its own with a version of its own,
 * so that include/fdn_hip.h and its ABI version stand still while this part grows.  Conventions as in fdn_hip.h: raw device pointers,
 * nothing allocated or synchronised, work enqueued on `stream`, FDN_OK or an FDN_ERR_* code returned.  (The reference has no such
 * option: no counterpart.)
 *
 * Codes k = 0 .. 7: bit 1 mirrors the columns, bit 2 mirrors the rows, bit 4 transposes; T_k applies the mirrors first, then the
 * transposition, so T_k of an h x w image is h' x w' = w x h when k & 4, else h x w:
 *     T_k(s)(y, x) = s(k & 2 ? h - 1 - u : u,  k & 1 ? w - 1 - v : v)   with (u, v) = k & 4 ? (x, y) : (y, x).
 * The inverse transposes first and then applies the same mirrors:
 *     T_k^-1(r)(y, x) = r(k & 4 ? (v, u) : (u, v))                      with u = k & 2 ? h - 1 - y : y,  v = k & 1 ? w - 1 - x : x.
 * mask: the set of codes, bit k of 1 .. 255; its K codes are taken in ascending k.
 *
 * FDN_ERR_ARG before any launch: a NULL pointer where data is required, mask outside 1 .. 255, B (N) < 1 or >= 65536, h or w < 1;
 * fdn_d4_pre_u8 / fdn_d4_apply also a mask with codes on both sides of bit 4 (one call makes one output shape), H < h', W < w',
 * H - h' >= h', W - w' >= w' (reflect padding needs pad < size) and H >= 65536; fdn_d4_mean / fdn_d4_post_u8 also a buffer that is
 * NULL while its part of the mask is not empty or the reverse, Ha < h, Wa < w, Hb < w, Wb < h (for the buffers present) and h >= 65536.
 */
#ifndef FDN_ENSEMBLE_H
#define FDN_ENSEMBLE_H

#include "fdn_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* version of this header: bumped on any signature change below */
#define FDN_ENSEMBLE_ABI_VERSION 1
int fdn_ensemble_abi_version(void);

/* img uint8 [B][h][w][3] -> out fp32 [K][B][3][H][W], one copy per code of mask in ascending k.  Output pixel (y, x) of copy k is
 * T_k(img) at (y, x), reflected bottom / right within h' x w' as fdn_pre_u8 reflects (y < h' ? y : 2 (h' - 1) - y), divided by 255
 * with true division, channels swapped with swap_rb as in fdn_pre_u8: bit for bit fdn_pre_u8 of the transformed image. */
int fdn_d4_pre_u8(const unsigned char* img, float* out, int B, int h, int w, int H, int W, int mask, int swap_rb, fdn_stream_t stream);

/* x fp32 [N][3][h][w] -> out fp32 [K][N][3][H][W]: the same movement and the same reflection, nothing computed. */
int fdn_d4_apply(const float* x, float* out, int N, int h, int w, int H, int W, int mask, fdn_stream_t stream);

/* res_a fp32 [Ka][B][3][Ha][Wa]: the results on the codes of mask & 0x0F; res_b fp32 [Kb][B][3][Hb][Wb]: on those of mask & 0xF0;
 * each NULL exactly when its part of the mask is empty.  out fp32 [B][3][h][w] = (sum over ascending k of T_k^-1(res_k cropped to
 * h' x w')) / (float)K: the sum starts from its first term and runs in fp32, every add and the division rounded once (no FMA
 * contraction, no reciprocal). */
int fdn_d4_mean(const float* res_a, const float* res_b, float* out, int B, int h, int w, int Ha, int Wa, int Hb, int Wb, int mask,
                fdn_stream_t stream);

/* The same sum and division, then fdn_post_u8's clamp to [0, 1], * 255, rintf (half to even) and channel order into out uint8
 * [B][h][w][3]: bit for bit fdn_d4_mean followed by fdn_post_u8. */
int fdn_d4_post_u8(const float* res_a, const float* res_b, unsigned char* out, int B, int h, int w, int Ha, int Wa, int Hb, int Wb,
                   int mask, int swap_rb, fdn_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
