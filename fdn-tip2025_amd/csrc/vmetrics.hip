// Video evaluation straight from codec samples (include/fdn_vmetrics.h): an enhanced stream of Y'CbCr 4:2:0 frames against a ground-truth
// stream, 8 or 10 bit, planar or semi-planar, never through 8-bit RGB.
//   fdn_yuv420_pair_stats : per frame pair the squared code differences summed over Y, Cb and Cr and the two luma sums.  Integers in 64
//                           bits, so exact in any order: per-thread sums, a tree per workgroup, one vector atomic per word
//   fdn_yuv420_ssim_y     : per frame pair the mean of the SSIM map of the luma planes, the reference's _ssim_cly (basicsr/metrics/
//                           psnr_ssim.py:202-240: 11 x 11 Gaussian, replicate border, no crop) on the codes, in float64, in ONE tiled
//                           launch over (tile, frame) and a per-frame fold
// Per 32 x 32 tile: the 42 x 42 apron of both frames' luma codes goes to LDS as 16-bit words (replicate addressing at the frame's edge,
// a 10-bit word above 1023 counts as 1023), the five fields a, b, a^2, b^2, ab are filtered along W into LDS (55 KB of doubles) and along
// H into registers, taps in ascending order; the map and every sum are float64.  No atomics on doubles: a tile's sum is a fixed tree over
// its 256 threads, a frame's sum a fixed walk over its tiles, so a score has the same bits on every call and in every slot of a batch.
// A frame starts at b * h * w * 3 / 2 samples, aligned to a sample only: every load here is a plain sample load.
// About 130 fp64 FMAs and 2 - 4 B per pixel; next to a 35 ms forward nothing here is worth more machinery.
#include "common.hpp"

#include "../../include/fdn_vmetrics.h"

#pragma clang fp contract(off)

namespace {

constexpr int TILE = 32, RAD = 5, APR = TILE + 2 * RAD;     // 42
constexpr int APR_LD = APR + 1;                             // 43
constexpr int ROW_LD = TILE + 1;                            // 33
constexpr int STATS_THREADS = 256, STATS_PER_THREAD = 8, STATS_MAX_BLOCKS = 2048;   // per frame

struct G11 { double w[11]; };

__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// Workgroup (x, b) walks samples x * 256 + tid, + gridDim.x * 256, ... of frame pair b: the luma plane, then (PAIR) the chroma samples,
// whose plane is found from the index alone.  s[0 .. 4] as the words of stats; one squared difference is at most 1023^2 and fits 32 bits,
// every sum is kept in 64.
template <typename T, bool PAIR>
__global__ __launch_bounds__(STATS_THREADS) void pair_stats_kernel(const T* __restrict__ a, const T* __restrict__ b,
                                                                   unsigned long long* __restrict__ stats, long n, int layout, unsigned top) {
    __shared__ unsigned long long red[5][STATS_THREADS];
    const int tid = threadIdx.x;
    const long frame = (long)blockIdx.y * (n + (n >> 1));
    const T* fa = a + frame;
    const long total = PAIR ? n + (n >> 1) : n, quarter = n >> 2;
    const long step = (long)gridDim.x * STATS_THREADS;
    unsigned long long s[5] = {0, 0, 0, 0, 0};
    for (long i = (long)blockIdx.x * STATS_THREADS + tid; i < total; i += step) {
        const unsigned x = min((unsigned)fa[i], top);
        if constexpr (PAIR) {
            const unsigned y = min((unsigned)b[frame + i], top);
            const int d = (int)x - (int)y;
            const unsigned dd = (unsigned)(d * d);
            if (i < n) {
                s[0] += dd;
                s[3] += x;
                s[4] += y;
            } else {
                const long j = i - n;
                const bool cr = layout ? (j & 1) : (j >= quarter);
                s[cr ? 2 : 1] += dd;
            }
        } else {
            s[3] += x;
        }
    }
#pragma unroll
    for (int k = 0; k < 5; ++k) red[k][tid] = s[k];
    __syncthreads();
    for (int st = STATS_THREADS / 2; st > 0; st >>= 1) {
        if (tid < st) {
#pragma unroll
            for (int k = 0; k < 5; ++k) red[k][tid] += red[k][tid + st];
        }
        __syncthreads();
    }
    if (tid < 5 && red[tid][0]) atomicAdd(&stats[(long)blockIdx.y * 5 + tid], red[tid][0]);
}

// grid (tiles, B); part [B][tiles] = the tile's sum of the SSIM map over its pixels inside the frame.  63 KB of LDS: two workgroups a CU.
template <typename T>
__global__ __launch_bounds__(256) void ssim_y_kernel(const T* __restrict__ a, const T* __restrict__ b, int h, int w, int tiles_x, unsigned top,
                                                     G11 g, double C1, double C2, double* __restrict__ part) {
    __shared__ unsigned short ax[APR * APR_LD], ay[APR * APR_LD];   // the apron of the two luma planes
    __shared__ double rowf[5][APR * ROW_LD];                        // the five fields after the W pass
    __shared__ double red[256];
    const int tid = threadIdx.x;
    const long n = (long)h * w;
    const long frame = (long)blockIdx.y * (n + (n >> 1));
    const int y0 = ((int)blockIdx.x / tiles_x) * TILE, x0 = ((int)blockIdx.x % tiles_x) * TILE;
    for (int i = tid; i < APR * APR; i += 256) {
        const int r = i / APR, c = i - r * APR;
        const int yy = clampi(y0 + r - RAD, h - 1), xx = clampi(x0 + c - RAD, w - 1);       // BORDER_REPLICATE
        const long off = frame + (long)yy * w + xx;
        ax[r * APR_LD + c] = (unsigned short)min((unsigned)a[off], top);
        ay[r * APR_LD + c] = (unsigned short)min((unsigned)b[off], top);
    }
    __syncthreads();
    // W pass: an item is 4 neighbouring columns of one apron row, from a 14-wide window
    for (int it = tid; it < APR * (TILE / 4); it += 256) {
        const int r = it >> 3, c0 = (it & 7) * 4;
        double xs[14], ys[14];
#pragma unroll
        for (int k = 0; k < 14; ++k) {
            xs[k] = (double)ax[r * APR_LD + c0 + k];
            ys[k] = (double)ay[r * APR_LD + c0 + k];
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            double v[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int t = 0; t < 11; ++t) {
                const double x = xs[j + t], y = ys[j + t];         // the products of two codes are exact
                v[0] = fma(g.w[t], x, v[0]);
                v[1] = fma(g.w[t], y, v[1]);
                v[2] = fma(g.w[t], x * x, v[2]);
                v[3] = fma(g.w[t], y * y, v[3]);
                v[4] = fma(g.w[t], x * y, v[4]);
            }
#pragma unroll
            for (int f = 0; f < 5; ++f) rowf[f][r * ROW_LD + c0 + j] = v[f];
        }
    }
    __syncthreads();
    // H pass: column px, rows py .. py + 3 of the tile from a 14-high window
    const int px = tid & 31, py = (tid >> 5) * 4;
    double v[4][5];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int f = 0; f < 5; ++f) v[j][f] = 0.0;
#pragma unroll
    for (int k = 0; k < 14; ++k) {
#pragma unroll
        for (int f = 0; f < 5; ++f) {
            const double s = rowf[f][(py + k) * ROW_LD + px];
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (k - j >= 0 && k - j < 11) v[j][f] = fma(g.w[k - j], s, v[j][f]);
        }
    }
    double s = 0.0;                                                 // the map (:226-238) at this thread's pixels inside the frame
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (y0 + py + j < h && x0 + px < w) {
            const double mu1 = v[j][0], mu2 = v[j][1];
            const double mu1_sq = mu1 * mu1, mu2_sq = mu2 * mu2, mu12 = mu1 * mu2;
            const double s1 = v[j][2] - mu1_sq, s2 = v[j][3] - mu2_sq, s12 = v[j][4] - mu12;
            s += ((2.0 * mu12 + C1) * (2.0 * s12 + C2)) / ((mu1_sq + mu2_sq + C1) * (s1 + s2 + C2));
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

// one workgroup per frame: out[b] = (the frame's partials, walked with stride 256 and folded by a tree) / (h w)
__global__ __launch_bounds__(256) void ssim_y_fold_kernel(const double* __restrict__ part, int tiles, double count, double* __restrict__ out) {
    __shared__ double red[256];
    const int tid = threadIdx.x;
    double s = 0.0;
    for (int t = tid; t < tiles; t += 256) s += part[(long)blockIdx.x * tiles + t];
    red[tid] = s;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if (tid < st) red[tid] += red[tid + st];
        __syncthreads();
    }
    if (tid == 0) out[blockIdx.x] = red[0] / count;
}

bool frames_ok(int B, int h, int w, int bits) {
    return B > 0 && B < 65536 && h >= 2 && w >= 2 && h % 2 == 0 && w % 2 == 0 && (bits == 8 || bits == 10) && (long)h * w < (1L << 30);
}

template <typename T>
void launch_stats(const void* a, const void* b, unsigned long long* stats, int B, long n, int layout, unsigned top, hipStream_t s) {
    const long total = b ? n + (n >> 1) : n;
    const dim3 grid(max(1, min(cdiv(total, (long)STATS_THREADS * STATS_PER_THREAD), STATS_MAX_BLOCKS)), B);
    if (b)
        hipLaunchKernelGGL((pair_stats_kernel<T, true>), grid, dim3(STATS_THREADS), 0, s, static_cast<const T*>(a), static_cast<const T*>(b), stats,
                           n, layout, top);
    else
        hipLaunchKernelGGL((pair_stats_kernel<T, false>), grid, dim3(STATS_THREADS), 0, s, static_cast<const T*>(a), static_cast<const T*>(nullptr),
                           stats, n, layout, top);
}

}  // namespace

extern "C" int fdn_vmetrics_abi_version(void) { return FDN_VMETRICS_ABI_VERSION; }

extern "C" int fdn_yuv420_pair_stats(const void* a, const void* b, long* stats, int B, int h, int w, int layout, int bits,
                                     fdn_stream_t stream) {
    FDN_CHECK_ARG(a && stats && frames_ok(B, h, w, bits) && (layout == 0 || layout == 1) && !(layout == 1 && bits == 10));
    static_assert(sizeof(long) == sizeof(unsigned long long), "stats are 64-bit");
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (hipMemsetAsync(stats, 0, (size_t)B * 5 * sizeof(long), s) != hipSuccess) return FDN_ERR_LAUNCH;
    unsigned long long* st = reinterpret_cast<unsigned long long*>(stats);
    const long n = (long)h * w;
    if (bits == 8)
        launch_stats<unsigned char>(a, b, st, B, n, layout, 255u, s);
    else
        launch_stats<unsigned short>(a, b, st, B, n, layout, 1023u, s);
    return fdn_launch_status();
}

extern "C" long fdn_yuv420_ssim_y_ws(int B, int h, int w) {
    if (!frames_ok(B, h, w, 8)) return 0;
    return (long)B * cdiv(h, TILE) * cdiv(w, TILE);
}

extern "C" int fdn_yuv420_ssim_y(const void* a, const void* b, double* out, double* ws, const double* taps11, int B, int h, int w, int bits,
                                 fdn_stream_t stream) {
    FDN_CHECK_ARG(a && b && out && ws && taps11 && frames_ok(B, h, w, bits));
    G11 g;
    for (int i = 0; i < 11; ++i) g.w[i] = taps11[i];
    const double L = (double)((1 << bits) - 1);
    const double C1 = (0.01 * L) * (0.01 * L), C2 = (0.03 * L) * (0.03 * L);
    const int tiles_x = cdiv(w, TILE), tiles = tiles_x * cdiv(h, TILE);      // < 2^20 + 2^16: h w < 2^30
    const dim3 grid((unsigned)tiles, (unsigned)B);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (bits == 8)
        hipLaunchKernelGGL(ssim_y_kernel<unsigned char>, grid, dim3(256), 0, s, static_cast<const unsigned char*>(a),
                           static_cast<const unsigned char*>(b), h, w, tiles_x, 255u, g, C1, C2, ws);
    else
        hipLaunchKernelGGL(ssim_y_kernel<unsigned short>, grid, dim3(256), 0, s, static_cast<const unsigned short*>(a),
                           static_cast<const unsigned short*>(b), h, w, tiles_x, 1023u, g, C1, C2, ws);
    hipLaunchKernelGGL(ssim_y_fold_kernel, dim3((unsigned)B), dim3(256), 0, s, (const double*)ws, tiles, (double)h * (double)w, out);
    return fdn_launch_status();
}
