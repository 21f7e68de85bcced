/* fdn_fusion.h -- exposure fusion (Mertens, Kautz, Van Reeth 2007) of K renderings of one frame: the entry points of libfdn_fusion.so.
 * FDN's brightness is one scalar per frame (ratio_i); K forwards of one frame at a bracket of ratios are blended here into one locally
 * exposed frame: per-pixel weights from contrast, saturation and well-exposedness, blended level by level through Laplacian pyramids.
 * A header of its own with a version of its own, in a library of its own built beside libfdn_hip.so, as fdn_sharpness.h: fdn_hip.h, the
 * other headers, their versions and libfdn_hip.so stand still.  Conventions as in fdn_hip.h: raw device pointers, nothing allocated or
 * synchronised, every kernel of a call enqueued on the one `stream`, FDN_OK or an FDN_ERR_* code returned; FDN_ERR_ARG before any launch.
 * No memory has to be zeroed by the caller.  No floating-point atomic is used and every sum runs in a fixed order: a frame fuses to the
 * same bits on every call, whatever H, W surround the crop.
 *
 * imgs: fp32 [K][3][H][W], R, G, B planes: the results of K forwards on one padded frame.  Only [:h, :w] is read (H >= h, W >= w), every
 * offset in 64 bits.  A sample v is clamped as it is read, in the weights and in the pyramids alike, as fdn_post_u8 clamps:
 *     clamp(v) = v < 0 ? 0 : (v > 1 ? 1 : v).
 * reflect(i, n), an index into an axis of length n, reflected without repeating the edge sample, repeatedly until in range: n == 1 -> 0;
 * else with p = 2 (n - 1), r = i mod p taken non-negative: r < n ? r : p - r.
 *
 * Weights (fdn_fuse_weights), per pixel in double from the clamped fp32 samples R, G, B, one rounding per operation, left to right:
 *     g = 0.2989 R + 0.587 G + 0.114 B                                                       (harness._gray_mean's coefficients)
 *     C = |4 g(y,x) - g(reflect(y-1,h),x) - g(reflect(y+1,h),x) - g(y,reflect(x-1,w)) - g(y,reflect(x+1,w))|
 *     m = (R + G + B) / 3,  S = sqrt(((R-m)^2 + (G-m)^2 + (B-m)^2) / 3)
 *     E = exp(-((R-.5)^2 + (G-.5)^2 + (B-.5)^2) / 0.08000000000000002)                       (2 * 0.2^2 in double)
 *     W_k = 1 * f(C, wc) * f(S, ws) * f(E, we) + 1e-12,   f(v, e) = 1 for e == 0 (the factor is left out), v for e == 1, else pow(v, e)
 *     weight_k = (float)(W_k / (W_0 + W_1 + ... + W_{K-1}))        summed from 0 in k order, divided in double, rounded once to fp32
 *
 * Pyramid (fdn_fuse_pyramid), fp32, one rounding per operation (no fused multiply-add), in exactly this order:
 *   sizes  per axis n_0 = n, n_{l+1} = (n_l + 1) / 2 (rounded down); L = min(floor(log2(min(h, w))), FDN_FUSION_MAX_LEVELS) levels.
 *   tap5(a0, a1, a2, a3, a4) = (((a0 + a4) + 4 * (a1 + a3)) + 6 * a2) * 0.0625f
 *   An axis of length 1 returns its one sample: along such an axis the pass of down, and of up from a coarse axis of length 1, is the
 *   identity, and no arithmetic touches the value.
 *   down   rows first: t(y, j) = tap5 of s(y, reflect(2j + d, ws)), d = -2 .. 2, for every source row y; then
 *          out(i, j) = tap5 of t(reflect(2i + d, hs), j), d = -2 .. 2.
 *   up     to (n_y, n_x) from a level c of ((n_y + 1) / 2, (n_x + 1) / 2).  Along x on a coarse row r = reflect(., hc):
 *              u(r, x) = x even, x = 2j:     ((c(r, reflect(j-1, wc)) + c(r, reflect(j+1, wc))) + 6 * c(r, j)) * 0.125f
 *                        x odd,  x = 2j + 1: (c(r, j) + c(r, reflect(j+1, wc))) * 0.5f
 *          then along y with the same two rules on u(reflect(i-1, hc), x), u(i, x), u(reflect(i+1, hc), x), y = 2i or 2i + 1.
 *   blend  Gi_{k,0} = clamp(imgs_k), Gw_{k,0} = weights_k, Gi_{k,l+1} = down(Gi_{k,l}), Gw_{k,l+1} = down(Gw_{k,l});
 *          B_l = (((0 + Gw_{0,l} * D_0) + Gw_{1,l} * D_1) + ...),  D_k = Gi_{k,l} - up(Gi_{k,l+1}) for l < L, D_k = Gi_{k,L} at l = L;
 *          out_L = B_L, out_l = B_l + up(out_{l+1}); the result is out_0, not clamped: fdn_post_u8 with H = h, W = w finishes it.
 * No Laplacian level is stored: one kernel per level walks k and reads Gi_{k,l}, Gi_{k,l+1} and Gw_{k,l}.
 */
#ifndef FDN_FUSION_H
#define FDN_FUSION_H

#include "fdn_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* version of this header: bumped on any signature change below */
#define FDN_FUSION_ABI_VERSION 1
int fdn_fusion_abi_version(void);

/* the most renderings and the most pyramid levels of a call; the output tile of the `down` kernel, FDN_FUSION_TILE x FDN_FUSION_TILE
 * samples (its source tile with the apron, 2 * FDN_FUSION_TILE + 3 a side, is staged in LDS), which is where a test looks for an edge */
enum { FDN_FUSION_MAX_K = 16, FDN_FUSION_MAX_LEVELS = 16, FDN_FUSION_TILE = 32 };

/* levels = L of an h x w frame (the rule above).  Host arithmetic only (no HIP call: answers without a GPU); levels is a HOST pointer.
 * FDN_ERR_ARG: levels NULL, h < 1, w < 1, h * w > 2^31 - 1. */
int fdn_fusion_dims(int h, int w, int* levels);

/* bytes of workspace fdn_fuse_pyramid needs for K renderings of h x w: levels 1 .. L of the K image pyramids, the K weight pyramids and
 * the collapse, (4 K + 3) floats per sample of those levels (0 when L = 0); -1 = bad arguments (K < 1, K > FDN_FUSION_MAX_K, h < 1,
 * w < 1, h * w > 2^31 - 1) */
long fdn_fusion_ws(int K, int h, int w);

/* imgs [K][3][H][W] -> weights [K][h][w] fp32, the normalised weights above.  One launch, one thread per pixel across all K.
 * FDN_ERR_ARG: imgs or weights NULL, K < 1, K > FDN_FUSION_MAX_K, h < 1, w < 1, H < h, W < w, h * w > 2^31 - 1, an exponent negative or
 * not finite.  FDN_ERR_LAUNCH: no device, or a launch failed. */
int fdn_fuse_weights(const float* imgs, float* weights, int K, int h, int w, int H, int W, double wc, double ws, double we,
                     fdn_stream_t stream);

/* imgs [K][3][H][W], weights [K][h][w] (any fp32 planes: a partition of unity fuses without a change of brightness) -> out [3][h][w].
 *   work: fdn_fusion_ws(K, h, w) bytes of device memory, 16-byte aligned (NULL allowed when that is 0).
 * FDN_ERR_ARG: imgs, weights or out NULL, work NULL where bytes are needed or not 16-byte aligned, K < 1, K > FDN_FUSION_MAX_K, h < 1,
 * w < 1, H < h, W < w, h * w > 2^31 - 1.  FDN_ERR_LAUNCH: no device, or a launch failed. */
int fdn_fuse_pyramid(const float* imgs, const float* weights, float* out, float* work, int K, int h, int w, int H, int W,
                     fdn_stream_t stream);

/* the two resampling steps alone.  down: in [C][H][W], of which [:h, :w] is read (clamped as above with clamp01 != 0), -> out
 * [C][(h + 1) / 2][(w + 1) / 2].  up: in [C][(h + 1) / 2][(w + 1) / 2] -> out [C][h][w].
 * FDN_ERR_ARG: in or out NULL, C < 1, h < 1, w < 1, H < h, W < w, h * w > 2^31 - 1.  FDN_ERR_UNSUPPORTED: C * tiles > 2^31 - 1 (down) or
 * C > 65535 (up).  FDN_ERR_LAUNCH: no device, or a launch failed. */
int fdn_pyr_down(const float* in, float* out, int C, int h, int w, int H, int W, int clamp01, fdn_stream_t stream);
int fdn_pyr_up(const float* in, float* out, int C, int h, int w, fdn_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
