// Fourier evaluation (include/fdn_spectral.h): the error between two spectra, bin by bin, split into an amplitude part and a phase part
// and summed per radial frequency band.
//   fdn_spectrum_band_counts : the Hermitian-weighted number of bins per band; host arithmetic, no HIP call
//   fdn_spectrum_pair_bands  : per plane and band the five sums of the header, float64, in ONE launch over (group of rows, plane) and a
//                              per-plane fold
// A workgroup of four waves owns ROWS rows of one plane pair; a wave walks its rows 64 bins at a time, lane = kx, so every request is a
// run of consecutive 8-byte bins of one row.  Every bin's five terms are formed in float64 from the float32 values.  Along a row the band
// never decreases with kx, so the 64 lanes of a step hold a few runs of equal band (one, mostly): per run the terms are summed over the
// wave by a fixed shuffle tree with the other lanes contributing 0, and lane 0 adds the five sums to the wave's own accumulators in LDS.
// No atomics on doubles: a wave's sums are a fixed walk over its rows, a workgroup's a fixed walk over its waves, a plane's a fixed walk
// over its partials in ws, and the geometry depends on (H, W, nb) alone - so a plane's result has the same bits on every call and in
// every slot of a batch.
// 16 B per bin pair read once; the float64 square roots and the shuffles, not the memory, set the pace.
#include "common.hpp"
#include "spectral_bands.hpp"

#include "../../include/fdn_spectral.h"

#pragma clang fp contract(off)

namespace {

constexpr int THREADS = 256, WAVES = THREADS / 64, ROWS = 8;      // rows per workgroup: wave w takes rows w, w + 4 of the group
constexpr int MAX_NB = 32, TERMS = 5;

bool shape_ok(int H, int W, int nb) { return H >= 1 && H <= 4096 && W >= 2 && W <= 10240 && W % 2 == 0 && nb >= 1 && nb <= MAX_NB; }

// grid (groups of rows * planes); part [plane][group][nb + 1][5]
__global__ __launch_bounds__(THREADS) void pair_bands_kernel(const float2* __restrict__ za, const float2* __restrict__ zb, int H, int W,
                                                             long pitch, int nb, int groups, double* __restrict__ part) {
    __shared__ double acc[WAVES][MAX_NB + 1][TERMS];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const long plane = blockIdx.x / groups;
    const int group = (int)(blockIdx.x - plane * groups);
    const int nslot = (nb + 1) * TERMS;
    for (int i = tid; i < WAVES * (MAX_NB + 1) * TERMS; i += THREADS) (&acc[0][0][0])[i] = 0.0;
    __syncthreads();
    const int Wh = W / 2;
    for (int r = wave; r < ROWS; r += WAVES) {
        const int ky = group * ROWS + r;
        if (ky >= H) break;                                          // wave-uniform
        const long row = (plane * H + ky) * pitch;
        for (int k0 = 0; k0 <= Wh; k0 += 64) {
            const int kx = k0 + lane;
            const bool in = kx <= Wh;
            double v[TERMS] = {0.0, 0.0, 0.0, 0.0, 0.0};
            int band = -1;
            if (in) {
                const float2 fa = za[row + kx], fb = zb[row + kx];
                const double ar = (double)fa.x, ai = (double)fa.y, br = (double)fb.x, bi = (double)fb.y;
                const double dr = ar - br, di = ai - bi;
                const double ma = sqrt(ar * ar + ai * ai), mb = sqrt(br * br + bi * bi);
                const double dm = ma - mb;
                const double ph = 2.0 * (ma * mb - (ar * br + ai * bi));
                const double h = (double)fdn_spectral_weight(kx, W);
                const double tot = dr * dr + di * di;
                v[0] = h * tot;
                v[1] = h * (dm * dm);
                v[2] = h * (ph > 0.0 ? (ph < tot ? ph : tot) : 0.0);      // the phase part lies in [0, total]: equal bins give exactly 0
                v[3] = h * (br * br + bi * bi);
                v[4] = fabs(dr) + fabs(di);
                band = fdn_spectral_band(ky, kx, H, W, nb);
            }
            unsigned long long todo = __ballot(in);
            while (todo) {                                           // one turn per run of equal band among the 64 lanes
                const int cur = __shfl(band, __ffsll((long long)todo) - 1);
                const bool mine = in && band == cur;
                double s[TERMS];
#pragma unroll
                for (int t = 0; t < TERMS; ++t) s[t] = mine ? v[t] : 0.0;
#pragma unroll
                for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
                    for (int t = 0; t < TERMS; ++t) s[t] += __shfl_down(s[t], off);
                }
                if (lane == 0) {
#pragma unroll
                    for (int t = 0; t < TERMS; ++t) acc[wave][cur][t] += s[t];
                }
                todo &= ~__ballot(mine);
            }
        }
    }
    __syncthreads();
    if (tid < nslot) {
        double s = (&acc[0][0][0])[tid];
#pragma unroll
        for (int w = 1; w < WAVES; ++w) s += (&acc[w][0][0])[tid];
        part[(long)blockIdx.x * nslot + tid] = s;
    }
}

// one workgroup per plane: out[plane][slot] = the plane's partials of that slot, walked in order
__global__ __launch_bounds__(THREADS) void pair_bands_fold_kernel(const double* __restrict__ part, int groups, int nslot,
                                                                  double* __restrict__ out) {
    const int tid = threadIdx.x;
    if (tid >= nslot) return;
    const double* p = part + (long)blockIdx.x * groups * nslot + tid;
    double s = 0.0;
    for (int g = 0; g < groups; ++g) s += p[(long)g * nslot];
    out[(long)blockIdx.x * nslot + tid] = s;
}

}  // namespace

extern "C" int fdn_spectral_abi_version(void) { return FDN_SPECTRAL_ABI_VERSION; }

extern "C" int fdn_spectrum_band_counts(int H, int W, int nb, long* counts) {
    FDN_CHECK_ARG(counts && shape_ok(H, W, nb));
    for (int b = 0; b <= nb; ++b) counts[b] = 0;
    for (int ky = 0; ky < H; ++ky)
        for (int kx = 0; kx <= W / 2; ++kx) counts[fdn_spectral_band(ky, kx, H, W, nb)] += fdn_spectral_weight(kx, W);
    return FDN_OK;
}

extern "C" long fdn_spectrum_pair_bands_ws(long planes, int H, int W, int nb) {
    if (planes < 1 || planes >= (1L << 31) || !shape_ok(H, W, nb)) return 0;
    return planes * cdiv(H, ROWS) * (nb + 1) * TERMS;
}

extern "C" int fdn_spectrum_pair_bands(const float* za, const float* zb, double* out, double* ws, long planes, int H, int W, long row_bins,
                                       int nb, fdn_stream_t stream) {
    FDN_CHECK_ARG(za && zb && out && ws && planes >= 1 && shape_ok(H, W, nb) && (row_bins == 0 || row_bins >= W / 2 + 1));
    static_assert(THREADS >= (MAX_NB + 1) * TERMS, "one thread per (band, term) in the two folds");
    const int groups = cdiv(H, ROWS);
    if (planes * groups > 0x7FFFFFFFL) return FDN_ERR_UNSUPPORTED;
    const long pitch = row_bins ? row_bins : W / 2 + 1;
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(pair_bands_kernel, dim3((unsigned)(planes * groups)), dim3(THREADS), 0, s, reinterpret_cast<const float2*>(za),
                       reinterpret_cast<const float2*>(zb), H, W, pitch, nb, groups, ws);
    hipLaunchKernelGGL(pair_bands_fold_kernel, dim3((unsigned)planes), dim3(THREADS), 0, s, (const double*)ws, groups, (nb + 1) * TERMS, out);
    return fdn_launch_status();
}
