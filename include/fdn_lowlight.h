/* fdn_lowlight.h -- low-light evaluation: the entry points of libfdn_hip.so that score what a low-light enhancer is judged by.
 *   LOE    lightness order error (after Wang et al. 2013) of an input image against its enhanced version: how often the enhancement
 *          reversed the relative order of two pixels' lightness.  Needs no ground truth.
 *   dE00   the CIEDE2000 colour difference (Sharma, Wu, Dalal 2005; kL = kC = kH = 1) of a restored image against its ground truth.
 * A header of its own with a version of its own, as include/fdn_spectral.h: fdn_hip.h, the other headers and their versions stand still.
 * Conventions as in fdn_hip.h: raw device pointers, nothing allocated or synchronised, work enqueued on `stream`, FDN_OK or an
 * FDN_ERR_* code returned; FDN_ERR_ARG before any launch.  No memory has to be zeroed by the caller: a launch zeroes what it accumulates
 * into.  An image's result does not depend on the other images of the batch and has the same bits on every call.
 *
 * images: uint8 [B][h][w][3], as fdn_post_u8 writes them and fdn_pair_*_u8 takes them.
 *
 * LOE of a pair a (input), b (enhanced).  The lightness of a pixel is L = max(R, G, B), a byte (the channel order does not matter).
 * Over the sample set S of m pixels
 *     RD(p) = #{q in S : [La(p) >= La(q)] != [Lb(p) >= Lb(q)]},      LOE = (1 / m) sum_p RD(p).
 * The sample set, decided in integers (`/` rounds down):
 *     size == 0 or min(h, w) <= size :  S is every pixel, Md = h, Nd = w;
 *     otherwise, with s = min(h, w)  :  Md = (2 h size + s) / (2 s),  Nd = (2 w size + s) / (2 s)   (h size / s, w size / s rounded half up)
 *                                       sample row i is source row ((2 i + 1) h) / (2 Md), sample column j source column ((2 j + 1) w) / (2 Nd).
 * No pair of pixels is compared.  With J[x][y] the number of samples with (La, Lb) = (x, y), C the inclusive 2-D prefix sum of J,
 * R[x] = C[x][255] and K[y] = C[255][y], a sample with the values (x, y) has RD = R[x] + K[y] - 2 C[x][y], and the numerator is
 *     sum_{x,y} J[x][y] (R[x] + K[y] - 2 C[x][y]),
 * exact in 64-bit integers: O(m + 65536) work, so size = 0 (full resolution) costs little more than a thumbnail.
 *
 * dE00 of a pair a (ground truth), b (restored), per pixel and all in float64 from the bytes: sRGB decoded per IEC 61966-2-1 (threshold
 * 0.04045, exponent 2.4), linear RGB to XYZ by the D65 matrix
 *     0.4124564 0.3575761 0.1804375 / 0.2126729 0.7151522 0.0721750 / 0.0193339 0.1191920 0.9503041,
 * each row summed left to right and divided by the white point (0.95047, 1, 1.08883), CIELAB with delta = 6/29, then CIEDE2000 with its
 * hue conventions (h = 0 where a' = b = 0; dh' = 0 and the mean hue h1 + h2 where C1' C2' = 0; the +-360 folds).
 */
#ifndef FDN_LOWLIGHT_H
#define FDN_LOWLIGHT_H

#include "fdn_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* version of this header: bumped on any signature change below */
#define FDN_LOWLIGHT_ABI_VERSION 1
int fdn_lowlight_abi_version(void);

/* md, nd = the sample grid Md x Nd of an h x w image at `size` (the rule above).  Host arithmetic only (no HIP call: answers without a
 * GPU); md, nd are HOST pointers.  FDN_ERR_ARG: a NULL pointer, h < 1, w < 1, size < 0, h * w > 2^31 - 1. */
int fdn_loe_sample_dims(int h, int w, int size, int* md, int* nd);

/* 8-byte words of workspace fdn_loe_u8 needs; 0 = bad arguments.  Per image 65792 words:
 *     uint32 J [256][256], uint32 C [256][256], uint32 R [256], uint32 K [256]     (the tables above, in this order) */
long fdn_loe_ws(int B, int h, int w, int size);

/* a (input), b (enhanced) [B][h][w][3] -> out [B][2] int64 = {numerator, m}; LOE = numerator / m, the host divides.  The tables J, C, R, K
 * of every image stay in ws for fdn_loe_map_u8.  Integer atomics only (their result does not depend on order).
 *   ws: fdn_loe_ws(B, h, w, size) 8-byte words of device memory, 16-byte aligned.
 * FDN_ERR_ARG: a NULL pointer, ws not 16-byte aligned, B < 1, h < 1, w < 1, size < 0, h * w > 2^31 - 1.
 * FDN_ERR_UNSUPPORTED: B * ceil(m / 32768) > 2^31 - 1 (more workgroups than a grid holds).  FDN_ERR_LAUNCH: no device, or a launch failed. */
int fdn_loe_u8(const unsigned char* a, const unsigned char* b, int B, int h, int w, int size, void* ws, long* out, fdn_stream_t stream);

/* rd [B][Md][Nd] uint32 = RD of every sample of the same a, b, size, looked up in the tables a preceding fdn_loe_u8 left in ws: the
 * picture of where the order broke.  It sums to the numerator.  FDN_ERR_ARG as for fdn_loe_u8; FDN_ERR_UNSUPPORTED: B > 65535; FDN_ERR_LAUNCH: a launch failed. */
int fdn_loe_map_u8(const unsigned char* a, const unsigned char* b, int B, int h, int w, int size, const void* ws, unsigned* rd,
                   fdn_stream_t stream);

/* 8-byte words of workspace fdn_deltae00_u8 needs; 0 = bad arguments */
long fdn_deltae00_ws(int B, int h, int w);

/* a (ground truth), b (restored) [B][h][w][3] -> out [B][2] float64 = {sum of dE00 over the pixels, maximum dE00}; the host divides the
 * sum by h * w.  bgr != 0: the bytes of a pixel are B, G, R, else R, G, B.  map: NULL, or float32 [B][h][w], the dE00 of every pixel
 * rounded once.  The sum runs in a fixed order - partials per tile of pixels in ws, then one fixed fold - and no floating-point atomic
 * is used.  Two equal images give exactly 0.0 in out and in map.
 *   ws: fdn_deltae00_ws(B, h, w) doubles of device memory.
 * FDN_ERR_ARG: a, b, ws or out NULL, B < 1, h < 1, w < 1, h * w > 2^31 - 1.  FDN_ERR_UNSUPPORTED: B * ceil(h w / 1024) > 2^31 - 1.
 * FDN_ERR_LAUNCH: a launch failed. */
int fdn_deltae00_u8(const unsigned char* a, const unsigned char* b, int B, int h, int w, int bgr, float* map, double* ws, double* out,
                    fdn_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
