// Paired validation metrics for batches of 8-bit images (ABI 20): the default branch of the reference's calculate_psnr (RGB, basicsr/metrics/
// psnr_ssim.py:47-62) and calculate_ssim (ssim3d=True, :149-200, :286-313) on uint8 [B][h][w][3] images as fdn_post_u8 writes and decoders
// give them, what the reference's validation scores (image_restoration_model.py:746-748, :844-848).
//   fdn_pair_sse_u8    : per image the sum of squared byte differences and the maximum of image 1, as FDN_PAIR_PARTS integer partials
//   fdn_pair_ssim3d_u8 : per image the mean of the 3-D SSIM map in ONE tiled launch on the bytes of the two images (no float copy of them
//                        in memory), then a per-image finish that folds all partials in a fixed order
// The 11x11x11 window is the outer product of three getGaussianKernel(11, 1.5).  Over three channels with replicate padding every tap of
// the channel pass lands on channel 0, 1 or 2, so that pass is a fixed 3 x 3 matrix: M[co][ci] = the sum of the taps t with
// clamp(co + t - 5, 0, 2) == ci.  Per 32 x 32 tile and input channel: the 42 x 42 apron (crop first, then replicate at the cropped
// image's border) goes to LDS as floats, the five fields x, y, x^2, y^2, xy are filtered along W into LDS and along H into registers
// (fp32, taps in ascending order as fdn_ssim3d's passes), and M adds the channel's share to the three output channels.  The apron is
// therefore loaded in three passes of byte loads three bytes apart, one per channel; the second and third hit in cache.
// No atomics: a tile's sum is a fixed tree over its 256 threads, an image's sum a fixed walk over its tiles, so a score has the same
// bits on every call and whatever else is in the batch.
// The float32 roundings of the reference's map (mu^2, E[x^2] - mu^2, the quotient) are part of what it computes, so contraction into
// FMAs is off in this file; the filter taps are explicit fmaf, as in fdn_ssim3d.
#include "common.hpp"

#pragma clang fp contract(off)

namespace {

constexpr int TILE = 32, RAD = 5, APR = TILE + 2 * RAD;     // 42
constexpr int APR_LD = APR + 1;                             // 43: the W pass reads 4 rows x 8 column groups of 4 per 32 lanes, conflict-free at an odd stride
constexpr int ROW_LD = TILE + 1;                            // 33: its writes (4 rows x 8 groups) land on 32 different banks
constexpr int PARTS = FDN_PAIR_PARTS;

struct G11 { float w[11]; };
struct M33 { float m[3][3]; };
struct SsimC { float c1_unit, c2_unit, c1_255, c2_255; };   // (0.01 L)^2, (0.03 L)^2 for L = 1 and L = 255 (:176-177)

__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// stats [B][PARTS][2]: part p of image b covers the cropped rows p, p + PARTS, ...; [0] = sum of (a - b)^2, [1] = max of a.
// Integers, so the sums are exact in any order.
__global__ __launch_bounds__(256) void pair_sse_u8_kernel(const unsigned char* __restrict__ a, const unsigned char* __restrict__ b, int h, int w,
                                                          int cb, long long* __restrict__ stats) {
    __shared__ unsigned long long reds[256];
    __shared__ unsigned redm[256];
    const int hc = h - 2 * cb, n = (w - 2 * cb) * 3, tid = threadIdx.x;
    const long img = (long)blockIdx.y * h * w * 3;
    unsigned long long s = 0;
    unsigned m = 0;
    for (int r = blockIdx.x; r < hc; r += PARTS) {
        const long row = img + ((long)(r + cb) * w + cb) * 3;
        for (int i = tid; i < n; i += 256) {
            const int x = a[row + i], d = x - (int)b[row + i];
            s += (unsigned)(d * d);
            m = x > (int)m ? (unsigned)x : m;
        }
    }
    reds[tid] = s;
    redm[tid] = m;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if (tid < st) {
            reds[tid] += reds[tid + st];
            redm[tid] = redm[tid] > redm[tid + st] ? redm[tid] : redm[tid + st];
        }
        __syncthreads();
    }
    if (tid == 0) {
        long long* o = stats + ((long)blockIdx.y * PARTS + blockIdx.x) * 2;
        o[0] = (long long)reds[0];
        o[1] = (long long)redm[0];
    }
}

// grid (tiles, B); part [B][tiles] = the tile's sum of the SSIM map over the three channels.  43.5 KB of LDS lets three workgroups share
// a CU; the bound keeps the registers to that too (167 VGPRs, no scratch)
__global__ __launch_bounds__(256, 3) void pair_ssim3d_u8_kernel(const unsigned char* __restrict__ a, const unsigned char* __restrict__ b, int h, int w,
                                                             int cb, int tiles_x, const long long* __restrict__ stats, G11 g, M33 mix, SsimC cc,
                                                             double* __restrict__ part) {
    __shared__ float ax[APR * APR_LD], ay[APR * APR_LD];        // one channel of the apron, both images
    __shared__ float rowf[5][APR * ROW_LD];                     // the five fields after the W pass
    __shared__ double red[256];
    const int tid = threadIdx.x;
    const int hc = h - 2 * cb, wc = w - 2 * cb;
    const long img = (long)blockIdx.y * h * w * 3;
    const int y0 = ((int)blockIdx.x / tiles_x) * TILE, x0 = ((int)blockIdx.x % tiles_x) * TILE;   // in the cropped image
    // max_value = 1 if img1.max() <= 1 else 255 (:311), from the partial maxima fdn_pair_sse_u8 left behind
    const int is255 = __syncthreads_or(stats[((long)blockIdx.y * PARTS + tid) * 2 + 1] > 1);
    const float C1 = is255 ? cc.c1_255 : cc.c1_unit, C2 = is255 ? cc.c2_255 : cc.c2_unit;
    const int px = tid & 31, py = (tid >> 5) * 4;               // H pass and map: column px, rows py .. py + 3 of the tile
    float acc[4][3][5];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int co = 0; co < 3; ++co)
#pragma unroll
            for (int f = 0; f < 5; ++f) acc[j][co][f] = 0.f;

#pragma unroll 1
    for (int ci = 0; ci < 3; ++ci) {
        for (int i = tid; i < APR * APR; i += 256) {
            const int r = i / APR, c = i - r * APR;
            const int yy = clampi(y0 + r - RAD, hc - 1) + cb, xx = clampi(x0 + c - RAD, wc - 1) + cb;   // padding_mode='replicate' (:158)
            const long off = img + ((long)yy * w + xx) * 3 + ci;
            ax[r * APR_LD + c] = (float)a[off];
            ay[r * APR_LD + c] = (float)b[off];
        }
        __syncthreads();
        // W pass: an item is 4 neighbouring columns of one apron row, from a 14-wide window
        for (int it = tid; it < APR * (TILE / 4); it += 256) {
            const int r = it >> 3, c0 = (it & 7) * 4;
            float xs[14], ys[14];
#pragma unroll
            for (int k = 0; k < 14; ++k) {
                xs[k] = ax[r * APR_LD + c0 + k];
                ys[k] = ay[r * APR_LD + c0 + k];
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
        for (int k = 0; k < 14; ++k) {
#pragma unroll
            for (int f = 0; f < 5; ++f) {
                const float s = rowf[f][(py + k) * ROW_LD + px];
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (k - j >= 0 && k - j < 11) v[j][f] = fmaf(g.w[k - j], s, v[j][f]);
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
    red[tid] = s;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if (tid < st) red[tid] += red[tid + st];
        __syncthreads();
    }
    if (tid == 0) part[(long)blockIdx.y * gridDim.x + blockIdx.x] = red[0];
}

// one workgroup per image: out[b] = {sum of squared differences, max of image 1, mean of the SSIM map}
__global__ __launch_bounds__(256) void pair_finish_kernel(const long long* __restrict__ stats, const double* __restrict__ part, int tiles,
                                                          double count, double* __restrict__ out) {
    __shared__ unsigned long long reds[256];
    __shared__ long long redm[256];
    __shared__ double red[256];
    const int tid = threadIdx.x;
    const long long* st2 = stats + ((long)blockIdx.x * PARTS + tid) * 2;
    double s = 0.0;
    for (int t = tid; t < tiles; t += 256) s += part[(long)blockIdx.x * tiles + t];
    reds[tid] = (unsigned long long)st2[0];
    redm[tid] = st2[1];
    red[tid] = s;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if (tid < st) {
            reds[tid] += reds[tid + st];
            redm[tid] = redm[tid] > redm[tid + st] ? redm[tid] : redm[tid + st];
            red[tid] += red[tid + st];
        }
        __syncthreads();
    }
    if (tid == 0) {
        double* o = out + (long)blockIdx.x * 3;
        o[0] = (double)reds[0];
        o[1] = (double)redm[0];
        o[2] = red[0] / count;
    }
}

static_assert(PARTS == 256, "one partial per thread of the SSIM and finish workgroups");

bool pair_args_ok(const void* a, const void* b, int B, int h, int w, int crop) {
    return a && b && B > 0 && B <= 65535 && h > 0 && w > 0 && crop >= 0 && h > 2 * crop && w > 2 * crop;
}

}  // namespace

extern "C" long fdn_pair_ssim3d_ws(int B, int h, int w, int crop) {
    if (B <= 0 || crop < 0 || h <= 2 * crop || w <= 2 * crop) return 0;
    return (long)B * cdiv(h - 2 * crop, TILE) * cdiv(w - 2 * crop, TILE);
}

extern "C" int fdn_pair_sse_u8(const unsigned char* a, const unsigned char* b, int B, int h, int w, int crop, long* stats,
                               fdn_stream_t stream) {
    FDN_CHECK_ARG(pair_args_ok(a, b, B, h, w, crop) && stats);
    static_assert(sizeof(long) == sizeof(long long), "stats are 64-bit");
    hipLaunchKernelGGL(pair_sse_u8_kernel, dim3(PARTS, (unsigned)B), dim3(256), 0, static_cast<hipStream_t>(stream), a, b, h, w, crop,
                       reinterpret_cast<long long*>(stats));
    return fdn_launch_status();
}

extern "C" int fdn_pair_ssim3d_u8(const unsigned char* a, const unsigned char* b, int B, int h, int w, int crop, const long* stats,
                                  const double* taps11, const double* chmix9, double* ws, double* out3, fdn_stream_t stream) {
    FDN_CHECK_ARG(pair_args_ok(a, b, B, h, w, crop) && stats && taps11 && chmix9 && ws && out3);
    G11 g;
    M33 mix;
    for (int i = 0; i < 11; ++i) g.w[i] = (float)taps11[i];
    for (int i = 0; i < 9; ++i) mix.m[i / 3][i % 3] = (float)chmix9[i];
    SsimC cc;                                              // python doubles, cast when they meet the fp32 maps (as fdn_ssim3d)
    cc.c1_unit = (float)((0.01 * 1.0) * (0.01 * 1.0));
    cc.c2_unit = (float)((0.03 * 1.0) * (0.03 * 1.0));
    cc.c1_255 = (float)((0.01 * 255.0) * (0.01 * 255.0));
    cc.c2_255 = (float)((0.03 * 255.0) * (0.03 * 255.0));
    const int hc = h - 2 * crop, wc = w - 2 * crop;
    const int tiles_x = cdiv(wc, TILE), tiles_y = cdiv(hc, TILE);
    FDN_CHECK_ARG((long)tiles_x * tiles_y <= 0x7fffffffL);
    const int tiles = tiles_x * tiles_y;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const long long* st = reinterpret_cast<const long long*>(stats);
    hipLaunchKernelGGL(pair_ssim3d_u8_kernel, dim3((unsigned)tiles, (unsigned)B), dim3(256), 0, s, a, b, h, w, crop, tiles_x, st, g, mix, cc, ws);
    hipLaunchKernelGGL(pair_finish_kernel, dim3((unsigned)B), dim3(256), 0, s, st, (const double*)ws, tiles, 3.0 * (double)hc * (double)wc, out3);
    return fdn_launch_status();
}
