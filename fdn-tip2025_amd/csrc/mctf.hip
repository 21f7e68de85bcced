// Motion-compensated temporal denoising (include/fdn_mctf.h, ABI 1; linked into libfdn_mctf.so, beside libfdn_hip.so).  The header has the
// definition, operation by operation.
//   fdn_mctf_blend : blend_kernel, one launch per frame (frame i reads what the launch of frame i - 1 wrote).  A workgroup of 256 threads
//                    walks tiles of 64 x 16 pixels; a wave is one row of 64 pixels, a thread owns four pixels of one column, 4 rows apart.
//                    Phase 1: every pixel of the tile and of its one-pixel ring that lies inside the frame gets its clamped value, its
//                    overlapped-block prediction (12 gathered loads: 4 vectors x 3 channels) and d, once: the tile's pixels by their
//                    owners, which keep c and pred in registers, the ring's 2 * 66 + 2 * 16 = 164 pixels by the first 164 threads, which
//                    keep nothing but d.  d goes to LDS, 18 x 66 floats.  Phase 2: the 3 x 3 sum of d is read from LDS at indices clamped to
//                    the frame (the replicated border), so a ring position outside the frame is neither computed nor read.
// One rounding per operation and a fixed order everywhere, so contraction into FMAs is off in this file.
#include "common.hpp"

#include <math.h>

#include "../../include/fdn_mctf.h"

#pragma clang fp contract(off)

namespace {

constexpr int BS = 16, TW = 64, TH = 16, LW = TW + 2, LH = TH + 2, RING = 2 * LW + 2 * TH;
constexpr int MAX_GRID = 65536;                                     // workgroups per launch; a frame of more tiles is walked in strides

static_assert(TW == 64 && TH * TW == 4 * 256 && RING <= 256, "a wave per row, four pixels per thread, one ring pixel per thread");

__device__ __forceinline__ float clamp01(float f) { return fminf(fmaxf(f, 0.f), 1.f); }
__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

struct Frame {
    const float* cur;                                               // [3][H][W]
    const float* P;                                                 // [3][h][w], the predecessor
    const short* mv;                                                // [nby][nbx][2]
    int h, w, nby, nbx;
    long plane, in_plane, W;
};

// (y, x) inside the frame -> c, pred; returns d
__device__ __forceinline__ float predict(const Frame& f, int y, int x, float (&c)[3], float (&pred)[3]) {
    const int b0y = (y - 8) >> 4, b0x = (x - 8) >> 4;               // floor: the shift of a negative int is arithmetic
    const int by[2] = {clampi(b0y, f.nby - 1), clampi(b0y + 1, f.nby - 1)}, bx[2] = {clampi(b0x, f.nbx - 1), clampi(b0x + 1, f.nbx - 1)};
    const float wy1 = (float)(2 * ((y + 8) & 15) + 1) * 0.03125f, wx1 = (float)(2 * ((x + 8) & 15) + 1) * 0.03125f;
    const float wy[2] = {1.0f - wy1, wy1}, wx[2] = {1.0f - wx1, wx1};
    pred[0] = pred[1] = pred[2] = 0.f;
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const short* m = f.mv + ((long)by[j] * f.nbx + bx[i]) * 2;
            const long at = (long)clampi(y + (int)m[0], f.h - 1) * f.w + clampi(x + (int)m[1], f.w - 1);
            const float wt = wy[j] * wx[i];
#pragma unroll
            for (int k = 0; k < 3; ++k) pred[k] = pred[k] + wt * f.P[k * f.plane + at];
        }
    const long at = (long)y * f.W + x;
#pragma unroll
    for (int k = 0; k < 3; ++k) c[k] = clamp01(f.cur[k * f.in_plane + at]);
    return fmaxf(fmaxf(fabsf(c[0] - pred[0]), fabsf(c[1] - pred[1])), fabsf(c[2] - pred[2]));
}

// grid (min(tiles of the frame, MAX_GRID)): one frame
__global__ __launch_bounds__(256) void blend_kernel(const float* __restrict__ cur, const float* __restrict__ P, const short* __restrict__ mv,
                                                    const long* __restrict__ stat, float* __restrict__ out, float* __restrict__ kmap, int h,
                                                    int w, int H, int W, int nby, int nbx, int tiles_x, int tiles, float strength,
                                                    float inv_threshold, long cut_limit) {
    __shared__ float s_d[LH * LW];
    const int tid = threadIdx.x, tx = tid & 63, ty = tid >> 6;
    const Frame f = {cur, P, mv, h, w, nby, nbx, (long)h * w, (long)H * W, (long)W};
    const bool bypass = P == nullptr || stat[0] > cut_limit;       // the same in every thread of the launch
    for (int t = blockIdx.x; t < tiles; t += gridDim.x) {
        const int y0 = (t / tiles_x) * TH, x0 = (t % tiles_x) * TW, x = x0 + tx;
        if (bypass) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int y = y0 + ty + 4 * j;
                if (x < w && y < h) {
                    const long at = (long)y * w + x;
#pragma unroll
                    for (int k = 0; k < 3; ++k) out[k * f.plane + at] = clamp01(cur[k * f.in_plane + (long)y * W + x]);
                    if (kmap) kmap[at] = 0.f;
                }
            }
            continue;
        }
        float c[4][3], p[4][3];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int y = y0 + ty + 4 * j;
            if (x < w && y < h) s_d[(ty + 4 * j + 1) * LW + tx + 1] = predict(f, y, x, c[j], p[j]);
        }
        if (tid < RING) {                                           // the ring: rows -1 and TH over LW columns, columns -1 and TW over TH rows
            const int side = tid < 2 * LW ? tid / LW : 2 + (tid - 2 * LW) / TH, k = tid < 2 * LW ? tid - side * LW : (tid - 2 * LW) % TH;
            const int ry = side == 0 ? -1 : (side == 1 ? TH : k), rx = side < 2 ? k - 1 : (side == 2 ? -1 : TW);
            const int y = y0 + ry, xr = x0 + rx;
            if (y >= 0 && y < h && xr >= 0 && xr < w) {
                float cr[3], pr[3];
                s_d[(ry + 1) * LW + rx + 1] = predict(f, y, xr, cr, pr);
            }
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int y = y0 + ty + 4 * j;
            if (x < w && y < h) {
                float s = 0.f;
#pragma unroll
                for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
                    for (int dx = -1; dx <= 1; ++dx)                // clamped to the frame: inside the tile or on a ring pixel that was computed
                        s = s + s_d[(clampi(y + dy, h - 1) - y0 + 1) * LW + clampi(x + dx, w - 1) - x0 + 1];
                const float D = s * (1.0f / 9.0f), tt = D * inv_threshold;
                const float k = strength * fmaxf(1.0f - tt * tt, 0.f);
                const long at = (long)y * w + x;
#pragma unroll
                for (int q = 0; q < 3; ++q) out[q * f.plane + at] = c[j][q] + k * (p[j][q] - c[j][q]);
                if (kmap) kmap[at] = k;
            }
        }
        __syncthreads();                                            // the next tile's phase 1 overwrites s_d
    }
}

}  // namespace

extern "C" int fdn_mctf_abi_version(void) { return FDN_MCTF_ABI_VERSION; }

extern "C" int fdn_mctf_blend(const float* cur, const float* prev, const short* mv, const long* stats, float* out, float* kmap, int B, int h,
                              int w, int H, int W, float strength, float inv_threshold, long cut_limit, fdn_stream_t stream) {
    FDN_CHECK_ARG(cur && mv && stats && out && B >= 1 && B < 65536 && h >= 1 && w >= 1 && H >= h && W >= w && (long)h * w < (1L << 30));
    FDN_CHECK_ARG(strength >= 0.f && strength <= 1.f && isfinite(inv_threshold) && inv_threshold > 0.f && cut_limit >= 0);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int nby = cdiv(h, BS), nbx = cdiv(w, BS), tiles_x = cdiv(w, TW), tiles = tiles_x * cdiv(h, TH);
    const long plane = (long)h * w, in_frame = 3L * H * W;
    for (int b = 0; b < B; ++b) {
        hipLaunchKernelGGL(blend_kernel, dim3((unsigned)(tiles < MAX_GRID ? tiles : MAX_GRID)), dim3(256), 0, s, cur + b * in_frame,
                           b ? out + (b - 1) * 3 * plane : prev, mv + (long)b * nby * nbx * 2, stats + (long)b * 4, out + b * 3 * plane,
                           kmap ? kmap + b * plane : nullptr, h, w, H, W, nby, nbx, tiles_x, tiles, strength, inv_threshold, cut_limit);
        const int rc = fdn_launch_status();
        if (rc != FDN_OK) return rc;
    }
    return FDN_OK;
}
