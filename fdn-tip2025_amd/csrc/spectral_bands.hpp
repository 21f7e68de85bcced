// The band rule of include/fdn_spectral.h, once: the radial frequency band of bin (ky, kx) of the half spectrum of an H x W image.
// spectral.hip's kernel and its host entry fdn_spectrum_band_counts call it and nothing else does.
#pragma once
#include <hip/hip_runtime.h>

// H <= 4096, W <= 10240, nb <= 32, 0 <= ky < H, 0 <= kx <= W / 2.  With ky' = min(ky, H - ky):
//   q = 4 nb^2 (ky'^2 W^2 + kx^2 H^2) <= 4 * 1024 * 2 * 2048^2 * 10240^2 < 3.7e18  and  D = H^2 W^2 < 1.8e15  fit 64 bits;
//   r0 = floor(sqrt(q / D)) <= floor(nb sqrt 2) = 45, so the candidates (r0 + 1)^2 D < 47^2 * 1.8e15 < 4e18 the search forms fit as well.
// The float square root is the first guess only (good to +-1); the two loops settle r0^2 D <= q < (r0 + 1)^2 D in integers, so a bin
// exactly on a band edge goes to the upper band whatever the rounding of the guess.
__host__ __device__ inline int fdn_spectral_band(int ky, int kx, int H, int W, int nb) {
    if (ky == 0 && kx == 0) return 0;
    const long kyp = ky < H - ky ? ky : H - ky;
    const long h2 = (long)H * H, w2 = (long)W * W;
    const long q = 4L * nb * nb * (kyp * kyp * w2 + (long)kx * kx * h2), D = h2 * w2;
    long r = (long)sqrtf((float)q / (float)D);
    if (r > 46) r = 46;
    while (r > 0 && r * r * D > q) --r;
    while ((r + 1) * (r + 1) * D <= q) ++r;
    return 1 + (int)(r < nb - 1 ? r : nb - 1);
}

// the Hermitian weight of column kx of the half spectrum: the bins it stands for in the full one
__host__ __device__ inline int fdn_spectral_weight(int kx, int W) { return (kx == 0 || kx == W / 2) ? 1 : 2; }
