/* fdn_spectral.h -- Fourier evaluation: the entry points of libfdn_hip.so that hand out the complex spectrum of a real image and split
 * the error of a restored image against its ground truth, bin by bin, into an amplitude part and a phase part per radial frequency band.
 * With Xa, Xb the spectra of the two images, for every bin
 *     |Xa - Xb|^2  =  (|Xa| - |Xb|)^2  +  2 (|Xa| |Xb| - Re(Xa conj(Xb)))
 *        total         amplitude part            phase part  (= 2 |Xa| |Xb| (1 - cos dphi) >= 0)
 * and by Parseval the left side, summed over the full spectrum and divided by (H W)^2, is the mean squared error of the image pair.
 * A header of its own with a version of its own, as include/fdn_video.h, fdn_temporal.h, fdn_vmetrics.h and fdn_ensemble.h: fdn_hip.h,
 * those headers and their versions stand still.  Conventions as in fdn_hip.h: raw device pointers, nothing allocated or synchronised,
 * work enqueued on `stream`, FDN_OK or an FDN_ERR_* code returned; FDN_ERR_ARG before any launch.
 *
 * spectra: [planes][H][row_bins] interleaved complex float32, the half spectrum of a real H x W image (kx = 0 .. W/2), unscaled
 * (norm='backward'), as fdn_rfft_rows followed by fdn_fft_cols_c2c writes it.
 *
 * The band of bin (ky, kx) of an H x W image with nb bands (csrc/spectral_bands.hpp, decided in 64-bit integers):
 *     ky' = min(ky, H - ky),  q = 4 nb^2 (ky'^2 W^2 + kx^2 H^2),  D = H^2 W^2,  r0 = the largest integer with r0^2 D <= q
 *     (r0 = floor(2 nb rho), rho the radial frequency in cycles per pixel);
 *     band 0 is the zero-frequency bin alone, every other bin lies in band 1 + min(r0, nb - 1): a bin exactly on a band edge belongs to
 *     the upper band, and the corners beyond rho = 0.5 fall into band nb.
 * The Hermitian weight h of a bin is 1 for kx = 0 and kx = W/2, else 2: the half spectrum stands for the full one.
 */
#ifndef FDN_SPECTRAL_H
#define FDN_SPECTRAL_H

#include "fdn_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* version of this header: bumped on any signature change below */
#define FDN_SPECTRAL_ABI_VERSION 1
int fdn_spectral_abi_version(void);

/* forward FFT along H, in place, of z [planes][H][Wf] interleaved complex, unscaled: with fdn_rfft_rows before it, rfft2.  Wf may be a
 * padded pitch (the padding columns are transformed like any other).  Runs the generic column kernel for every length, also one with a
 * compile-time plan; accepts every H fdn_fft_cols_fwd accepts, FDN_ERR_UNSUPPORTED where that one refuses.
 * FDN_ERR_ARG: z NULL, planes < 1, H < 1, Wf < 1. */
int fdn_fft_cols_c2c(float* z, long planes, int H, int Wf, fdn_stream_t stream);

/* counts [nb + 1] = the Hermitian-weighted number of bins per band of an H x W image; they sum to H * W.  Host arithmetic only (no HIP
 * call: answers without a GPU); counts is a HOST pointer.  FDN_ERR_ARG as for fdn_spectrum_pair_bands. */
int fdn_spectrum_band_counts(int H, int W, int nb, long* counts);

/* doubles of workspace fdn_spectrum_pair_bands needs; 0 = bad arguments */
long fdn_spectrum_pair_bands_ws(long planes, int H, int W, int nb);

/* spectra za (restored), zb (ground truth) [planes][H][row_bins] -> out [planes][nb + 1][5] float64, per band
 *     0  sum h |Xa - Xb|^2                                    the total error
 *     1  sum h (|Xa| - |Xb|)^2                                its amplitude part
 *     2  sum h max(0, 2 (|Xa| |Xb| - Re(Xa conj(Xb))))        its phase part (a bin's term is also held at or below that bin's total,
 *                                                             which bounds it in exact arithmetic: two equal bins give exactly 0)
 *     3  sum h |Xb|^2                                         the ground truth's energy
 *     4  sum (|dRe| + |dIm|), unweighted                      the numerator of the reference's FFTLoss (losses.py:109-115: L1 on rfft2)
 * row_bins = 0: dense rows of W/2 + 1 bins.  Bins past W/2 of a row are never read.  Every bin's terms are formed in float64 from the
 * float32 values.  The sums run in a fixed order - partials per group of rows in ws, then one fixed fold - and no floating-point atomic
 * is used, so a plane's result has the same bits on every call and in every slot of a batch.  A band without a bin is exactly 0.
 *   ws: fdn_spectrum_pair_bands_ws(planes, H, W, nb) doubles of device memory.
 * FDN_ERR_ARG: a NULL pointer, planes < 1, H < 1 or > 4096, W odd or < 2 or > 10240, nb < 1 or > 32, 0 < row_bins < W/2 + 1. */
int fdn_spectrum_pair_bands(const float* za, const float* zb, double* out, double* ws, long planes, int H, int W, long row_bins, int nb,
                            fdn_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
