// Brightness-corrected PSNR / SSIM of batches of 8-bit image pairs (include/fdn_correct.h, ABI 1; linked into libfdn_correct.so, beside
// libfdn_hip.so): the restored image is scored after an affine map per channel towards its ground truth - the reference's
// --correct_mean_var (scripts/metrics/calculate_psnr_ssim.py:38-54) or the GT-mean convention - whose coefficients the host forms from
// exact integer sums.
//   fdn_pair_moments_u8   : per image the sum and the sum of squares of every channel of both images over the WHOLE image and the maximum
//                           of the ground truth over the cropped region, as FDN_PAIR_PARTS integer partials; fdn_pair_moments_fold adds them up
//   fdn_pair_corrected_u8 : per image the sum of (gt - z)^2 and the mean of the 3-D SSIM map of (gt, z) in ONE tiled launch on the bytes of
//                           the two images, then a per-image finish; z, the corrected sample, is formed when the apron is loaded and
//                           exists in LDS only
//   fdn_pair_apply_u8     : z as fp32 planes
// The 3-D SSIM tile is that of metrics_pair.hip's pair_ssim3d_u8_kernel (its comment has the why of every step): the same 32 x 32 tiles,
// 42 x 42 apron with replicate padding at the cropped border, W pass into LDS, H pass into registers, 3 x 3 channel matrix, float32 with
// explicit fmaf taps.  The body is carried here, not shared through a header, so that metrics_pair.hip and the code object of its kernel
// stay what they were.
// No atomics: a tile's sums are fixed trees over its 256 threads, an image's sums a fixed walk over its tiles, so a score has the same
// bits on every call and whatever else is in the batch.  The correction is double arithmetic with one rounding per operation, and the
// float32 roundings of the reference's map are part of what it computes, so contraction into FMAs is off in this file.
#include "common.hpp"

#include "../../include/fdn_correct.h"

#pragma clang fp contract(off)

namespace {

constexpr int TILE = 32, RAD = 5, APR = TILE + 2 * RAD;     // 42
constexpr int APR_LD = APR + 1;                             // 43: the W pass reads 4 rows x 8 column groups of 4 per 32 lanes, conflict-free at an odd stride
constexpr int ROW_LD = TILE + 1;                            // 33: its writes (4 rows x 8 groups) land on 32 different banks
constexpr int PARTS = FDN_PAIR_PARTS, NMOM = FDN_PAIR_MOMENTS;

struct G11 { float w[11]; };
struct M33 { float m[3][3]; };
struct SsimC { float c1_unit, c2_unit, c1_255, c2_255; };   // (0.01 L)^2, (0.03 L)^2 for L = 1 and L = 255 (psnr_ssim.py:176-177)
struct Coef { double m_r, s, m_g, lo, hi; };                // one channel of one image: coef [B][3][5]

__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// the corrected sample of a byte (fdn_correct.h): comparisons, not fmin / fmax, so that a NaN coefficient stays a NaN sample
__device__ __forceinline__ float corrected(unsigned char x, const Coef& k) {
    double t = (double)x - k.m_r;
    t = t * k.s;
    t = t + k.m_g;
    t = t < k.lo ? k.lo : t;
    t = t > k.hi ? k.hi : t;
    return (float)t;
}

__device__ __forceinline__ Coef load_coef(const double* __restrict__ coef, long b, int c) {
    const double* p = coef + (b * 3 + c) * 5;
    return Coef{p[0], p[1], p[2], p[3], p[4]};
}

// moments [B][PARTS][NMOM]: part p of image b covers the rows p, p + PARTS, ... of the whole image.  Integers: exact in any order.
__global__ __launch_bounds__(256) void pair_moments_u8_kernel(const unsigned char* __restrict__ gt, const unsigned char* __restrict__ rs, int h,
                                                              int w, int cb, long long* __restrict__ moments) {
    __shared__ unsigned long long red[256];
    const int tid = threadIdx.x;
    const long img = (long)blockIdx.y * h * w * 3;
    unsigned long long v[NMOM];
#pragma unroll
    for (int k = 0; k < NMOM; ++k) v[k] = 0;
    for (int r = blockIdx.x; r < h; r += PARTS) {
        const long row = img + (long)r * w * 3;
        const bool rin = r >= cb && r < h - cb;
        for (int i = tid; i < w; i += 256) {
            const bool in = rin && i >= cb && i < w - cb;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const unsigned g = gt[row + (long)i * 3 + c], x = rs[row + (long)i * 3 + c];
                v[c] += g;
                v[3 + c] += g * g;
                v[6 + c] += x;
                v[9 + c] += x * x;
                if (in && g > v[12]) v[12] = g;
            }
        }
    }
    long long* o = moments + ((long)blockIdx.y * PARTS + blockIdx.x) * NMOM;
#pragma unroll 1
    for (int k = 0; k < NMOM; ++k) {
        red[tid] = v[k];
        __syncthreads();
        for (int st = 128; st > 0; st >>= 1) {
            if (tid < st) red[tid] = k == 12 ? (red[tid] > red[tid + st] ? red[tid] : red[tid + st]) : red[tid] + red[tid + st];
            __syncthreads();
        }
        if (tid == 0) o[k] = (long long)red[0];
        __syncthreads();
    }
}

// one workgroup per image, one part per thread: folded [B][NMOM]
__global__ __launch_bounds__(256) void pair_moments_fold_kernel(const long long* __restrict__ moments, long long* __restrict__ folded) {
    __shared__ unsigned long long red[256];
    const int tid = threadIdx.x;
    const long long* p = moments + ((long)blockIdx.x * PARTS + tid) * NMOM;
#pragma unroll 1
    for (int k = 0; k < NMOM; ++k) {
        red[tid] = (unsigned long long)p[k];
        __syncthreads();
        for (int st = 128; st > 0; st >>= 1) {
            if (tid < st) red[tid] = k == 12 ? (red[tid] > red[tid + st] ? red[tid] : red[tid + st]) : red[tid] + red[tid + st];
            __syncthreads();
        }
        if (tid == 0) folded[(long)blockIdx.x * NMOM + k] = (long long)red[0];
        __syncthreads();
    }
}

// grid (tiles, B); part [B][tiles][2] = the tile's sum of (gt - z)^2 over its own pixels and the three channels, and its sum of the SSIM
// map.  a = gt, b = restored.  43.5 KB of LDS lets three workgroups share a CU, as in pair_ssim3d_u8_kernel.
__global__ __launch_bounds__(256, 3) void pair_corrected_u8_kernel(const unsigned char* __restrict__ a, const unsigned char* __restrict__ b, int h,
                                                                int w, int cb, int tiles_x, const double* __restrict__ coef,
                                                                const int* __restrict__ is255p, G11 g, M33 mix, SsimC cc,
                                                                double* __restrict__ part) {
    __shared__ float ax[APR * APR_LD], ay[APR * APR_LD];        // one channel of the apron: gt, corrected restored
    __shared__ float rowf[5][APR * ROW_LD];                     // the five fields after the W pass
    __shared__ double red[256];
    const int tid = threadIdx.x;
    const int hc = h - 2 * cb, wc = w - 2 * cb;
    const long img = (long)blockIdx.y * h * w * 3;
    const int y0 = ((int)blockIdx.x / tiles_x) * TILE, x0 = ((int)blockIdx.x % tiles_x) * TILE;   // in the cropped image
    const int is255 = is255p[blockIdx.y];
    const float C1 = is255 ? cc.c1_255 : cc.c1_unit, C2 = is255 ? cc.c2_255 : cc.c2_unit;
    const int px = tid & 31, py = (tid >> 5) * 4;               // H pass and map: column px, rows py .. py + 3 of the tile
    float acc[4][3][5];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int co = 0; co < 3; ++co)
#pragma unroll
            for (int f = 0; f < 5; ++f) acc[j][co][f] = 0.f;
    double sse = 0.0;                                           // of this thread's apron items that are the tile's own pixels inside the image

#pragma unroll 1
    for (int ci = 0; ci < 3; ++ci) {
        const Coef k = load_coef(coef, blockIdx.y, ci);
        for (int i = tid; i < APR * APR; i += 256) {
            const int r = i / APR, c = i - r * APR;
            const int yy = clampi(y0 + r - RAD, hc - 1) + cb, xx = clampi(x0 + c - RAD, wc - 1) + cb;   // padding_mode='replicate' (:158)
            const long off = img + ((long)yy * w + xx) * 3 + ci;
            const unsigned char ga = a[off];
            const float z = corrected(b[off], k);
            ax[r * APR_LD + c] = (float)ga;
            ay[r * APR_LD + c] = z;
            if (r >= RAD && r < RAD + TILE && c >= RAD && c < RAD + TILE && y0 + r - RAD < hc && x0 + c - RAD < wc) {
                const double d = (double)ga - (double)z;
                sse += d * d;
            }
        }
        __syncthreads();
        // W pass: an item is 4 neighbouring columns of one apron row, from a 14-wide window
        for (int it = tid; it < APR * (TILE / 4); it += 256) {
            const int r = it >> 3, c0 = (it & 7) * 4;
            float xs[14], ys[14];
#pragma unroll
            for (int k2 = 0; k2 < 14; ++k2) {
                xs[k2] = ax[r * APR_LD + c0 + k2];
                ys[k2] = ay[r * APR_LD + c0 + k2];
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float v[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int t = 0; t < 11; ++t) {
                    const float x = xs[j + t], y = ys[j + t];
                    v[0] = fmaf(g.w[t], x, v[0]);
                    v[1] = fmaf(g.w[t], y, v[1]);
                    v[2] = fmaf(g.w[t], x * x, v[2]);
                    v[3] = fmaf(g.w[t], y * y, v[3]);
                    v[4] = fmaf(g.w[t], x * y, v[4]);
                }
#pragma unroll
                for (int f = 0; f < 5; ++f) rowf[f][r * ROW_LD + c0 + j] = v[f];
            }
        }
        __syncthreads();
        // H pass: 4 rows of one column from a 14-high window, then this input channel's share of the three output channels
        float v[4][5];
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int f = 0; f < 5; ++f) v[j][f] = 0.f;
#pragma unroll
        for (int k2 = 0; k2 < 14; ++k2) {
#pragma unroll
            for (int f = 0; f < 5; ++f) {
                const float s = rowf[f][(py + k2) * ROW_LD + px];
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (k2 - j >= 0 && k2 - j < 11) v[j][f] = fmaf(g.w[k2 - j], s, v[j][f]);
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int co = 0; co < 3; ++co)
#pragma unroll
                for (int f = 0; f < 5; ++f) acc[j][co][f] = fmaf(mix.m[co][ci], v[j][f], acc[j][co][f]);
        __syncthreads();                                        // the next channel overwrites ax / ay / rowf
    }

    double s = 0.0;                                             // the SSIM map (:186-196) of this thread's pixels that lie inside the image
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (y0 + py + j < hc && x0 + px < wc) {
#pragma unroll
            for (int co = 0; co < 3; ++co) {
                const float mu1 = acc[j][co][0], mu2 = acc[j][co][1];
                const float mu1_sq = mu1 * mu1, mu2_sq = mu2 * mu2, mu12 = mu1 * mu2;
                const float s1 = acc[j][co][2] - mu1_sq, s2 = acc[j][co][3] - mu2_sq, s12 = acc[j][co][4] - mu12;
                s += (double)(((2.f * mu12 + C1) * (2.f * s12 + C2)) / ((mu1_sq + mu2_sq + C1) * (s1 + s2 + C2)));
            }
        }
    }
    double* o = part + ((long)blockIdx.y * gridDim.x + blockIdx.x) * 2;
#pragma unroll 1
    for (int q = 0; q < 2; ++q) {                               // the same tree for both sums
        red[tid] = q == 0 ? sse : s;
        __syncthreads();
        for (int st = 128; st > 0; st >>= 1) {
            if (tid < st) red[tid] += red[tid + st];
            __syncthreads();
        }
        if (tid == 0) o[q] = red[0];
        __syncthreads();
    }
}

// one workgroup per image: out2[b] = {sum of squared differences, mean of the SSIM map}, the tiles walked in a fixed order
__global__ __launch_bounds__(256) void pair_corrected_finish_kernel(const double* __restrict__ part, int tiles, double count,
                                                                    double* __restrict__ out2) {
    __shared__ double red[256];
    const int tid = threadIdx.x;
#pragma unroll 1
    for (int q = 0; q < 2; ++q) {
        double s = 0.0;
        for (int t = tid; t < tiles; t += 256) s += part[((long)blockIdx.x * tiles + t) * 2 + q];
        red[tid] = s;
        __syncthreads();
        for (int st = 128; st > 0; st >>= 1) {
            if (tid < st) red[tid] += red[tid + st];
            __syncthreads();
        }
        if (tid == 0) out2[(long)blockIdx.x * 2 + q] = q == 0 ? red[0] : red[0] / count;
        __syncthreads();
    }
}

// grid (pixel blocks, B): out [B][3][h][w]
__global__ __launch_bounds__(256) void pair_apply_u8_kernel(const unsigned char* __restrict__ rs, const double* __restrict__ coef, long n,
                                                            float* __restrict__ out) {
    const long p = (long)blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    const long b = blockIdx.y;
#pragma unroll
    for (int c = 0; c < 3; ++c) out[(b * 3 + c) * n + p] = corrected(rs[(b * n + p) * 3 + c], load_coef(coef, b, c));
}

static_assert(PARTS == 256, "one part per thread of the fold workgroup");

bool size_ok(int B, int h, int w) { return B > 0 && B <= 65535 && h > 0 && w > 0 && (long)h * w <= 0x7fffffffL; }
bool crop_ok(int h, int w, int crop) { return crop >= 0 && h > 2 * crop && w > 2 * crop; }

}  // namespace

extern "C" int fdn_correct_abi_version(void) { return FDN_CORRECT_ABI_VERSION; }

extern "C" int fdn_pair_moments_u8(const unsigned char* gt, const unsigned char* restored, int B, int h, int w, int crop, long* moments,
                                   fdn_stream_t stream) {
    FDN_CHECK_ARG(gt && restored && moments && size_ok(B, h, w) && crop_ok(h, w, crop));
    static_assert(sizeof(long) == sizeof(long long), "moments are 64-bit");
    hipLaunchKernelGGL(pair_moments_u8_kernel, dim3(PARTS, (unsigned)B), dim3(256), 0, static_cast<hipStream_t>(stream), gt, restored, h, w, crop,
                       reinterpret_cast<long long*>(moments));
    return fdn_launch_status();
}

extern "C" int fdn_pair_moments_fold(const long* moments, int B, long* folded, fdn_stream_t stream) {
    FDN_CHECK_ARG(moments && folded && B > 0 && B <= 65535);
    hipLaunchKernelGGL(pair_moments_fold_kernel, dim3((unsigned)B), dim3(256), 0, static_cast<hipStream_t>(stream),
                       reinterpret_cast<const long long*>(moments), reinterpret_cast<long long*>(folded));
    return fdn_launch_status();
}

extern "C" long fdn_pair_corrected_ws(int B, int h, int w, int crop) {
    if (!size_ok(B, h, w) || !crop_ok(h, w, crop)) return 0;
    return 2L * B * cdiv(h - 2 * crop, TILE) * cdiv(w - 2 * crop, TILE);
}

extern "C" int fdn_pair_corrected_u8(const unsigned char* gt, const unsigned char* restored, int B, int h, int w, int crop, const double* coef,
                                     const int* is255, const double* taps11, const double* chmix9, double* ws, double* out2,
                                     fdn_stream_t stream) {
    FDN_CHECK_ARG(gt && restored && coef && is255 && taps11 && chmix9 && ws && out2 && size_ok(B, h, w) && crop_ok(h, w, crop));
    G11 g;
    M33 mix;
    for (int i = 0; i < 11; ++i) g.w[i] = (float)taps11[i];
    for (int i = 0; i < 9; ++i) mix.m[i / 3][i % 3] = (float)chmix9[i];
    SsimC cc;                                              // python doubles, cast when they meet the fp32 maps (as fdn_pair_ssim3d_u8)
    cc.c1_unit = (float)((0.01 * 1.0) * (0.01 * 1.0));
    cc.c2_unit = (float)((0.03 * 1.0) * (0.03 * 1.0));
    cc.c1_255 = (float)((0.01 * 255.0) * (0.01 * 255.0));
    cc.c2_255 = (float)((0.03 * 255.0) * (0.03 * 255.0));
    const int hc = h - 2 * crop, wc = w - 2 * crop;
    const int tiles_x = cdiv(wc, TILE), tiles_y = cdiv(hc, TILE);
    const int tiles = tiles_x * tiles_y;                   // <= h * w <= 2^31 - 1
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(pair_corrected_u8_kernel, dim3((unsigned)tiles, (unsigned)B), dim3(256), 0, s, gt, restored, h, w, crop, tiles_x, coef, is255,
                       g, mix, cc, ws);
    hipLaunchKernelGGL(pair_corrected_finish_kernel, dim3((unsigned)B), dim3(256), 0, s, (const double*)ws, tiles, 3.0 * (double)hc * (double)wc,
                       out2);
    return fdn_launch_status();
}

extern "C" int fdn_pair_apply_u8(const unsigned char* restored, const double* coef, int B, int h, int w, float* out, fdn_stream_t stream) {
    FDN_CHECK_ARG(restored && coef && out && size_ok(B, h, w));
    const long n = (long)h * w;
    hipLaunchKernelGGL(pair_apply_u8_kernel, dim3((unsigned)cdiv(n, 256), (unsigned)B), dim3(256), 0, static_cast<hipStream_t>(stream), restored,
                       coef, n, out);
    return fdn_launch_status();
}
