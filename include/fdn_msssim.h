/* fdn_msssim.h -- multi-scale SSIM (Wang, Simoncelli, Bovik 2003) of 8-bit image pairs and of video luma planes: the entry points of
 * libfdn_msssim.so.  Contrast and structure are measured over five octaves and luminance only at the coarsest, which tells residual blur
 * (lost at the fine levels) from a tone shift over a region (lost at the coarse ones) where single-scale SSIM scores both alike.
 * A header of its own with a version of its own, in a library of its own built beside libfdn_hip.so: fdn_hip.h, the other headers, their
 * versions and libfdn_hip.so stand still.  Conventions as in fdn_sharpness.h: raw device pointers, nothing allocated or synchronised, work
 * enqueued on `stream`, FDN_OK or an FDN_ERR_* code returned; FDN_ERR_ARG before any launch.  No memory has to be zeroed by the caller: a
 * launch writes every word it later reads.  No floating-point atomic is used: sums run as per-tile partials in the workspace (a fixed
 * tree over the tile's threads), then one fold per plane and level in a fixed tile order, so a plane's result does not depend on its
 * batch neighbours and has the same bits on every call.
 *
 * Planes.  A plane is an h x w array of integer samples with a scale factor q0 and a peak L.
 *   8-bit image pair: uint8 [B][h][w][3], as fdn_pair_*_u8 and fdn_gmsd_u8 take them.
 *     mode FDN_MSSSIM_RGB:  three planes per image, in the order R, G, B (bgr != 0: the bytes of a pixel are B, G, R, so plane k reads
 *                           byte 2 - k; else plane k reads byte k).  q0 = 1, L = 255.  The image's score is the mean of the three planes'
 *                           MS-SSIM values, added in the order R, G, B (the host's step).
 *     mode FDN_MSSSIM_GRAY: one plane y = 299 R + 587 G + 114 B, the integer of fdn_gmsd_u8; bgr says where R sits.  q0 = 1000, L = 255.
 *   Video luma: the Y plane of frames laid out as fdn_pre_yuv420 and fdn_yuv420_ssim_y take them, Y first, frame f starting at sample
 *     f * stride (planar and nv12 do not differ for Y).  bits 8: uint8; bits 10: uint16, a code above 1023 counts as 1023.  q0 = 1,
 *     L = 2^bits - 1: 10 bit is scored as 10 bit.
 *
 * Pyramid.  Five levels; level 0 is the plane, h_0 = h, w_0 = w, and h_(s+1) = (h_s + 1) / 2, w_(s+1) = (w_s + 1) / 2, rounded down.
 * Level s + 1 holds at (i, j) the integer sum of level s over rows 2i, 2i + 1 and columns 2j, 2j + 1, where a row or column index equal
 * to the size is taken at size - 1: Wang's MATLAB code, imfilter(., ones(2) / 4, 'symmetric', 'same') followed by (1:2:end, 1:2:end),
 * times 4.  For even sizes it is the 2 x 2 mean every common implementation uses; for odd sizes the last row or column counts twice.
 * A level-s sample is an exact int32, q = q0 * 4^s times the mean it stands for: at most 1000 * 255 * 256 < 2^31.  Its square, and the
 * product of two samples, is exact in double: at most (6.528e7)^2 < 2^53.
 *
 * Per level.  The window is the 11 x 11 Gaussian g_i g_j, g = taps11 (sigma 1.5, normalised, float64; the host passes it in, as
 * fdn_yuv420_ssim_y takes its taps).  Positions are 'valid' only: the map of level s is mh_s x mw_s = (h_s - 10) x (w_s - 10).
 * With A, B the integer samples as doubles and q = q0 * 4^s, the five windowed moments m_a, m_b, m_aa, m_bb, m_ab of A, B, A * A, B * B,
 * A * B (the products exact) are each formed in float64 in a fixed order, one rounding per operation (no FMA contraction):
 *     row pass     r = 0, then r = r + g_t * x(y, x + t) for t = 0 .. 10;
 *     column pass  m = 0, then m = m + g_t * r(y + t, x) for t = 0 .. 10.
 * Then with C1' = (0.01 L) * (0.01 L) * q * q and C2' = (0.03 L) * (0.03 L) * q * q, multiplied left to right in double,
 *     va = m_aa - m_a * m_a,   vb = m_bb - m_b * m_b,   vab = m_ab - m_a * m_b,
 *     cs = (2 * vab + C2') / (va + vb + C2'),
 *     l  = (2 * (m_a * m_b) + C1') / (m_a * m_a + m_b * m_b + C1'),
 *     ss = l * cs.
 * Equal planes give cs == l == 1.0 exactly: the moments of a and b are then the same doubles, so vab == va == vb, and 2 * x and x + x are
 * the same double, so each numerator has the bits of its denominator.
 *
 * Result.  The device returns, per plane and level, the sum of cs and the sum of ss over the level's map.  The host divides by the map's
 * size mh_s * mw_s and forms
 *     MS-SSIM = prod over s = 0 .. 3 of max(mean cs_s, 0)^w_s, times max(mean ss_4, 0)^w_4,  w = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333).
 *
 * Smallest size.  The coarsest map needs h_4 >= 11 and w_4 >= 11, that is h, w >= FDN_MSSSIM_MIN_SIDE = 161.  Anything smaller is
 * refused: no scale is dropped silently.
 */
#ifndef FDN_MSSSIM_H
#define FDN_MSSSIM_H

#include "fdn_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* version of this header: bumped on any signature change below */
#define FDN_MSSSIM_ABI_VERSION 1
int fdn_msssim_abi_version(void);

/* the levels, the smallest side, and the tile of the window kernel: FDN_MSSSIM_TILE_H rows by FDN_MSSSIM_TILE_W columns of map positions
 * per workgroup (its samples with the 10-sample apron and the row pass of the five moments fit 64 KB of LDS: about 9 KB + 33 KB).  The
 * tile sizes the workspace and is where a test looks for an edge. */
enum { FDN_MSSSIM_LEVELS = 5, FDN_MSSSIM_MIN_SIDE = 161, FDN_MSSSIM_TILE_H = 16, FDN_MSSSIM_TILE_W = 32 };

/* the modes of fdn_msssim_u8 */
enum { FDN_MSSSIM_RGB = 0, FDN_MSSSIM_GRAY = 1 };

/* lh, lw, mh, mw [5] = the level sizes h_s, w_s and the map sizes h_s - 10, w_s - 10 of an h x w plane.  Host arithmetic only (no HIP
 * call: answers without a GPU); the four are HOST pointers.  FDN_ERR_ARG: a NULL pointer, h < 161, w < 161, h * w > 2^31 - 1. */
int fdn_msssim_dims(int h, int w, int* lh, int* lw, int* mh, int* mw);

/* doubles of workspace the scoring entries need for B images of `planes` planes each (3 for FDN_MSSSIM_RGB, else 1): two per tile of
 * every plane's five maps, then room for the int32 pyramids of a and b; 0 = bad arguments (B < 1, planes not 1 or 3, h < 161, w < 161,
 * h * w > 2^31 - 1) */
long fdn_msssim_ws(int B, int planes, int h, int w);

/* The optional outputs of the two scoring entries, NULL when not wanted, P = B * planes the number of planes:
 *   pyr_a, pyr_b   int32, levels 1 .. 4 one after the other, level s as [P][h_s][w_s]: P * (h_1 w_1 + ... + h_4 w_4) words each;
 *   cs_map, ss_map float64, levels 0 .. 4 one after the other, level s as [P][mh_s][mw_s]: cs and ss at every map position.
 * ws: fdn_msssim_ws(B, planes, h, w) doubles of device memory, 8-byte aligned.  taps11: HOST pointer to the 11 window taps (read before
 * the call returns).  out [P][5][2] float64 = per plane and level {the sum of cs, the sum of ss} over the map.
 * One call is four pyramid launches, five window launches and one fold for the whole batch. */

/* a, b uint8 [B][h][w][3]; mode FDN_MSSSIM_RGB (planes = 3) or FDN_MSSSIM_GRAY (planes = 1); bgr as above.
 * FDN_ERR_ARG: a, b, taps11, ws or out NULL, ws not 8-byte aligned, B < 1, h < 161, w < 161, h * w > 2^31 - 1, mode not one of the two.
 * FDN_ERR_UNSUPPORTED: more workgroups than a grid holds (2^31 - 1).  FDN_ERR_LAUNCH: no device, or a launch failed. */
int fdn_msssim_u8(const unsigned char* a, const unsigned char* b, int B, int h, int w, int mode, int bgr, const double* taps11, int* pyr_a,
                  int* pyr_b, double* cs_map, double* ss_map, double* ws, double* out, fdn_stream_t stream);

/* a, b: B frames each, the h x w Y plane of frame f at sample f * stride (stride = h * w * 3 / 2 for 4:2:0 frames); bits 8 (uint8) or 10
 * (uint16, clamped to 1023); planes = 1.
 * FDN_ERR_ARG: as above, bits not 8 or 10, stride < h * w.  FDN_ERR_UNSUPPORTED, FDN_ERR_LAUNCH: as above. */
int fdn_msssim_luma(const void* a, const void* b, int B, int h, int w, int bits, long stride, const double* taps11, int* pyr_a, int* pyr_b,
                    double* cs_map, double* ss_map, double* ws, double* out, fdn_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
