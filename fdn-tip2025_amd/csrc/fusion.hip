// Exposure fusion of K renderings of one frame (include/fdn_fusion.h, ABI 1; linked into libfdn_fusion.so, beside libfdn_hip.so).  The
// header has the definitions and the order of every operation.
//   fdn_fuse_weights : weights_kernel, one thread per pixel across all K: the K unnormalised weights wait in LDS (one column per thread,
//                      so no two lanes meet on a bank) while their sum forms, and are normalised from there; double throughout.
//   fdn_pyr_down     : pyr_down_kernel, one 32 x 32 tile of outputs per workgroup: the 67 x 67 source tile with its apron is staged in LDS
//                      (reflected at the frame's edge, clamped where the source is the renderings), filtered along x into a second LDS
//                      tile, then along y.  Global loads and stores walk x fastest.
//   fdn_pyr_up       : pyr_up_kernel, four samples of a row per thread.
//   fdn_fuse_pyramid : pyr_down_kernel per level for the 3 K image planes and the K weight planes, then blend_kernel per level from the
//                      coarsest up: a thread owns four samples of a row in the three channels, walks k itself, reads Gw_{k,l} once for
//                      the three channels, Gi_{k,l} as one 16-byte load where the address allows, and interpolates Gi_{k,l+1} and the
//                      collapsed level below from the few coarse samples its four need.  No Laplacian level is stored.
// No atomics, every sum in a fixed order.  The arithmetic is defined with one rounding per operation, so contraction into FMAs is off.
#include "common.hpp"

#include <math.h>

#include "../../include/fdn_fusion.h"

#pragma clang fp contract(off)

namespace {

constexpr int TD = FDN_FUSION_TILE, SA = 2 * TD + 3;          // 32 x 32 outputs from a 67 x 67 source tile
constexpr int SA_LD = SA + 1, TD_LD = TD + 1;
constexpr int MAXK = FDN_FUSION_MAX_K;

static_assert(TD * TD == 4 * 256, "four outputs per thread");

__device__ __forceinline__ float clamp01(float v) { return v < 0.f ? 0.f : (v > 1.f ? 1.f : v); }

// an index into an axis of length n, reflected without repeating the edge sample, until in range.  64 bits off the common path: an axis
// may be 2^31 - 1 long, and a tile that hangs over the edge asks for indices past twice that
__device__ __forceinline__ int reflect(long i, int n) {
    if (i >= 0 && i < n) return (int)i;
    if (n == 1) return 0;
    const long p = 2L * (n - 1);
    long r = i % p;
    if (r < 0) r += p;
    return (int)(r < n ? r : p - r);
}

__device__ __forceinline__ float tap5(float a0, float a1, float a2, float a3, float a4) {
    return (((a0 + a4) + 4.0f * (a1 + a3)) + 6.0f * a2) * 0.0625f;
}

__device__ __forceinline__ double factor(double v, double e, int mode) { return mode == 1 ? v : pow(v, e); }

// grid cdiv(w, 64) * cdiv(h, 4) blocks of 64 x 4 pixels.  mode_*: 0 = the factor is left out, 1 = as it is, 2 = pow
__global__ __launch_bounds__(256) void weights_kernel(const float* __restrict__ imgs, float* __restrict__ weights, int K, int h, int w, int H,
                                                      int W, int bx, double wc, double ws, double we, int mode_c, int mode_s, int mode_e) {
    __shared__ double Wl[MAXK][256];
    const int tid = threadIdx.x;
    const long xl0 = (long)(blockIdx.x % (unsigned)bx) * 64 + (tid & 63), yl0 = (long)(blockIdx.x / (unsigned)bx) * 4 + (tid >> 6);
    if (xl0 >= w || yl0 >= h) return;                         // no barrier below: a thread reads only its own column of Wl
    const int x = (int)xl0, y = (int)yl0;
    const long plane = (long)H * W;
    const int yu = reflect(y - 1L, h), yd = reflect(y + 1L, h), xl = reflect(x - 1L, w), xr = reflect(x + 1L, w);
    const long at[5] = {(long)y * W + x, (long)yu * W + x, (long)yd * W + x, (long)y * W + xl, (long)y * W + xr};
    double sum = 0.0;
#pragma unroll 1
    for (int k = 0; k < K; ++k) {
        const float* p = imgs + (long)k * 3 * plane;
        double g[5], R = 0.0, G = 0.0, B = 0.0;
#pragma unroll
        for (int n = 0; n < 5; ++n) {
            const double r = (double)clamp01(p[at[n]]), gg = (double)clamp01(p[plane + at[n]]), b = (double)clamp01(p[2 * plane + at[n]]);
            g[n] = 0.2989 * r + 0.587 * gg + 0.114 * b;
            if (n == 0) {
                R = r;
                G = gg;
                B = b;
            }
        }
        double v = 1.0;
        if (mode_c) v = v * factor(fabs(4.0 * g[0] - g[1] - g[2] - g[3] - g[4]), wc, mode_c);
        if (mode_s) {
            const double m = (R + G + B) / 3.0;
            const double dr = R - m, dg = G - m, db = B - m;
            v = v * factor(sqrt((dr * dr + dg * dg + db * db) / 3.0), ws, mode_s);
        }
        if (mode_e) {
            const double dr = R - 0.5, dg = G - 0.5, db = B - 0.5;
            v = v * factor(exp(-(dr * dr + dg * dg + db * db) / 0.08000000000000002), we, mode_e);
        }
        v = v + 1e-12;
        Wl[k][tid] = v;
        sum = sum + v;
    }
    const long o = (long)y * w + x, hw = (long)h * w;
#pragma unroll 1
    for (int k = 0; k < K; ++k) weights[k * hw + o] = (float)(Wl[k][tid] / sum);
}

// grid C * tiles; in [C][H][W] of which [:hs, :ws] is the source, out [C][hd][wd]
__global__ __launch_bounds__(256) void pyr_down_kernel(const float* __restrict__ in, float* __restrict__ out, int hs, int ws, int H, int W, int hd,
                                                   int wd, int tiles_x, int tiles, int clamp) {
    __shared__ float src[SA][SA_LD];
    __shared__ float tmp[SA][TD_LD];
    const int tid = threadIdx.x;
    const long c = blockIdx.x / (unsigned)tiles;
    const int tile = (int)(blockIdx.x - c * tiles);
    const int y0 = (tile / tiles_x) * TD, x0 = (tile % tiles_x) * TD;
    const float* p = in + c * H * (long)W;
    for (int i = tid; i < SA * SA; i += 256) {
        const int r = i / SA, cc = i - r * SA;
        const int sy = reflect(2L * y0 - 2 + r, hs), sx = reflect(2L * x0 - 2 + cc, ws);
        const float v = p[(long)sy * W + sx];
        src[r][cc] = clamp ? clamp01(v) : v;
    }
    __syncthreads();
    for (int i = tid; i < SA * TD; i += 256) {
        const int r = i / TD, j = i - r * TD;
        const float* s = &src[r][2 * j];
        tmp[r][j] = ws == 1 ? s[2] : tap5(s[0], s[1], s[2], s[3], s[4]);
    }
    __syncthreads();
    const int px = tid & 31;
#pragma unroll
    for (int n = 0; n < 4; ++n) {
        const int py = (tid >> 5) + 8 * n;
        const int oy = y0 + py, ox = x0 + px;
        if (oy < hd && ox < wd)
            out[(c * hd + oy) * (long)wd + ox] =
                hs == 1 ? tmp[2 * py + 2][px] : tap5(tmp[2 * py][px], tmp[2 * py + 1][px], tmp[2 * py + 2][px], tmp[2 * py + 3][px], tmp[2 * py + 4][px]);
    }
}

// u(r, x0 .. x0 + 3) of one coarse row, x0 a multiple of 4: the four coarse samples around j0 = x0 / 2, each read once
__device__ __forceinline__ void up_row4(const float* __restrict__ row, int wc, int j0, float (&u)[4]) {
    if (wc == 1) {
        u[0] = u[1] = u[2] = u[3] = row[0];
        return;
    }
    const float a = row[reflect(j0 - 1, wc)], b = row[reflect(j0, wc)], c = row[reflect(j0 + 1, wc)], d = row[reflect(j0 + 2, wc)];
    u[0] = ((a + c) + 6.0f * b) * 0.125f;
    u[1] = (b + c) * 0.5f;
    u[2] = ((b + d) + 6.0f * c) * 0.125f;
    u[3] = (c + d) * 0.5f;
}

// up(c)(y, x0 .. x0 + 3) of one coarse plane [hc][wc]; samples past the fine level's width come out as finite garbage and are not stored
__device__ __forceinline__ void up4(const float* __restrict__ c, int hc, int wc, int y, int x0, float (&v)[4]) {
    const int i = y >> 1, j0 = x0 >> 1;
    float u0[4];
    up_row4(c + (long)i * wc, wc, j0, u0);
    if (hc == 1) {
#pragma unroll
        for (int n = 0; n < 4; ++n) v[n] = u0[n];
        return;
    }
    float up[4];
    up_row4(c + (long)reflect(i + 1, hc) * wc, wc, j0, up);
    if (y & 1) {
#pragma unroll
        for (int n = 0; n < 4; ++n) v[n] = (u0[n] + up[n]) * 0.5f;
    } else {
        float um[4];
        up_row4(c + (long)reflect(i - 1, hc) * wc, wc, j0, um);
#pragma unroll
        for (int n = 0; n < 4; ++n) v[n] = ((um[n] + up[n]) + 6.0f * u0[n]) * 0.125f;
    }
}

// p[0 .. 3] where they lie below n, as one 16-byte access where the address allows; the rest is 0 / not written
__device__ __forceinline__ void load4(const float* __restrict__ p, int n, float (&v)[4]) {
    if (n >= 4 && (reinterpret_cast<uintptr_t>(p) & 15u) == 0) {
        const float4 f = *reinterpret_cast<const float4*>(p);
        v[0] = f.x;
        v[1] = f.y;
        v[2] = f.z;
        v[3] = f.w;
    } else {
#pragma unroll
        for (int t = 0; t < 4; ++t) v[t] = t < n ? p[t] : 0.f;
    }
}
__device__ __forceinline__ void store4(float* __restrict__ p, int n, const float (&v)[4]) {
    if (n >= 4 && (reinterpret_cast<uintptr_t>(p) & 15u) == 0) {
        *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int t = 0; t < 4; ++t)
            if (t < n) p[t] = v[t];
    }
}

// grid C planes (y) x groups of four samples (x); in [C][hc][wc] -> out [C][h][w]
__global__ __launch_bounds__(256) void pyr_up_kernel(const float* __restrict__ in, float* __restrict__ out, int h, int w, int hc, int wc, int gx) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)gx * h) return;
    const int y = (int)(idx / gx), x0 = (int)(idx - (long)y * gx) * 4;
    const long c = blockIdx.y;
    float v[4];
    up4(in + c * hc * (long)wc, hc, wc, y, x0, v);
    store4(out + (c * h + y) * (long)w + x0, w - x0, v);
}

// One level of the blend and of the collapse.  fine: Gi_{k,l}, [K][3] planes of [H][W] of which [:h, :w] is the level (the renderings
// themselves at l = 0, clamped); wgt: Gw_{k,l} [K][h][w]; coarse: Gi_{k,l+1} [K][3][hc][wc] and below: out_{l+1} [3][hc][wc], both NULL at
// the last level; out: out_l [3][h][w].  A thread owns four samples of a row.
__global__ __launch_bounds__(256) void blend_kernel(const float* __restrict__ fine, const float* __restrict__ wgt, const float* __restrict__ coarse,
                                                    const float* __restrict__ below, float* __restrict__ out, int K, int h, int w, int H, int W,
                                                    int hc, int wc, int gx, int clamp) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)gx * h) return;
    const int y = (int)(idx / gx), x0 = (int)(idx - (long)y * gx) * 4;
    const int n = w - x0;
    const long plane = (long)H * W, cplane = (long)hc * wc, hw = (long)h * w;
    float acc[3][4];
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[c][t] = 0.f;
#pragma unroll 1
    for (int k = 0; k < K; ++k) {
        float wv[4];
        load4(wgt + k * hw + (long)y * w + x0, n, wv);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float f[4];
            load4(fine + ((long)k * 3 + c) * plane + (long)y * W + x0, n, f);
            if (clamp) {
#pragma unroll
                for (int t = 0; t < 4; ++t) f[t] = clamp01(f[t]);
            }
            if (coarse) {
                float u[4];
                up4(coarse + ((long)k * 3 + c) * cplane, hc, wc, y, x0, u);
#pragma unroll
                for (int t = 0; t < 4; ++t) f[t] = f[t] - u[t];
            }
#pragma unroll
            for (int t = 0; t < 4; ++t) acc[c][t] = acc[c][t] + wv[t] * f[t];
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        if (below) {
            float u[4];
            up4(below + c * cplane, hc, wc, y, x0, u);
#pragma unroll
            for (int t = 0; t < 4; ++t) acc[c][t] = acc[c][t] + u[t];
        }
        store4(out + c * hw + (long)y * w + x0, n, acc[c]);
    }
}

bool size_ok(int h, int w) { return h >= 1 && w >= 1 && (long)h * w <= 0x7FFFFFFFL; }
bool k_ok(int K) { return K >= 1 && K <= MAXK; }
bool exponent_ok(double e) { return e >= 0.0 && e <= 1.7976931348623157e308; }     // false for a NaN
int exponent_mode(double e) { return e == 0.0 ? 0 : (e == 1.0 ? 1 : 2); }

int levels_of(int h, int w) {
    int m = h < w ? h : w, L = 0;
    while (m >= 2) {
        m >>= 1;
        ++L;
    }
    return L < FDN_FUSION_MAX_LEVELS ? L : FDN_FUSION_MAX_LEVELS;
}

int launch_down(const float* in, float* out, int C, int h, int w, int H, int W, int clamp, hipStream_t s) {
    const int hd = (h + 1) / 2, wd = (w + 1) / 2;
    const long tiles = (long)cdiv(hd, TD) * cdiv(wd, TD);
    if (C * tiles > 0x7FFFFFFFL) return FDN_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(pyr_down_kernel, dim3((unsigned)(C * tiles)), dim3(256), 0, s, in, out, h, w, H, W, hd, wd, cdiv(wd, TD), (int)tiles, clamp);
    return FDN_OK;
}

}  // namespace

extern "C" int fdn_fusion_abi_version(void) { return FDN_FUSION_ABI_VERSION; }

extern "C" int fdn_fusion_dims(int h, int w, int* levels) {
    FDN_CHECK_ARG(levels && size_ok(h, w));
    *levels = levels_of(h, w);
    return FDN_OK;
}

extern "C" long fdn_fusion_ws(int K, int h, int w) {
    if (!k_ok(K) || !size_ok(h, w)) return -1;
    long samples = 0;
    for (int l = 0, L = levels_of(h, w); l < L; ++l) {
        h = (h + 1) / 2;
        w = (w + 1) / 2;
        samples += (long)h * w;
    }
    return samples * (4L * K + 3) * (long)sizeof(float);
}

extern "C" int fdn_fuse_weights(const float* imgs, float* weights, int K, int h, int w, int H, int W, double wc, double ws, double we,
                                fdn_stream_t stream) {
    FDN_CHECK_ARG(imgs && weights && k_ok(K) && size_ok(h, w) && H >= h && W >= w && exponent_ok(wc) && exponent_ok(ws) && exponent_ok(we));
    const int bx = cdiv(w, 64);
    hipLaunchKernelGGL(weights_kernel, dim3((unsigned)((long)bx * cdiv(h, 4))), dim3(256), 0, static_cast<hipStream_t>(stream), imgs, weights, K, h,
                       w, H, W, bx, wc, ws, we, exponent_mode(wc), exponent_mode(ws), exponent_mode(we));
    return fdn_launch_status();
}

extern "C" int fdn_pyr_down(const float* in, float* out, int C, int h, int w, int H, int W, int clamp01, fdn_stream_t stream) {
    FDN_CHECK_ARG(in && out && C >= 1 && size_ok(h, w) && H >= h && W >= w);
    const int rc = launch_down(in, out, C, h, w, H, W, clamp01 != 0 ? 1 : 0, static_cast<hipStream_t>(stream));
    return rc != FDN_OK ? rc : fdn_launch_status();
}

extern "C" int fdn_pyr_up(const float* in, float* out, int C, int h, int w, fdn_stream_t stream) {
    FDN_CHECK_ARG(in && out && C >= 1 && size_ok(h, w));
    if (C > 65535) return FDN_ERR_UNSUPPORTED;
    const int gx = cdiv(w, 4);
    hipLaunchKernelGGL(pyr_up_kernel, dim3((unsigned)cdiv((long)gx * h, 256), (unsigned)C), dim3(256), 0, static_cast<hipStream_t>(stream), in, out, h, w,
                       (h + 1) / 2, (w + 1) / 2, gx);
    return fdn_launch_status();
}

extern "C" int fdn_fuse_pyramid(const float* imgs, const float* weights, float* out, float* work, int K, int h, int w, int H, int W,
                                fdn_stream_t stream) {
    FDN_CHECK_ARG(imgs && weights && out && k_ok(K) && size_ok(h, w) && H >= h && W >= w);
    const int L = levels_of(h, w);
    FDN_CHECK_ARG(L == 0 || (work && (reinterpret_cast<uintptr_t>(work) & 15u) == 0));
    hipStream_t s = static_cast<hipStream_t>(stream);
    // level l >= 1 of the workspace: Gi [K][3][hl][wl], Gw [K][hl][wl], out [3][hl][wl]
    const float* gi[FDN_FUSION_MAX_LEVELS + 1];
    const float* gw[FDN_FUSION_MAX_LEVELS + 1];
    float* ol[FDN_FUSION_MAX_LEVELS + 1];
    int hl[FDN_FUSION_MAX_LEVELS + 1], wl[FDN_FUSION_MAX_LEVELS + 1], Hl[FDN_FUSION_MAX_LEVELS + 1], Wl[FDN_FUSION_MAX_LEVELS + 1];
    gi[0] = imgs, gw[0] = weights, ol[0] = out, hl[0] = h, wl[0] = w, Hl[0] = H, Wl[0] = W;
    float* at = work;
    for (int l = 1; l <= L; ++l) {
        hl[l] = Hl[l] = (hl[l - 1] + 1) / 2;
        wl[l] = Wl[l] = (wl[l - 1] + 1) / 2;
        const long n = (long)hl[l] * wl[l];
        float* i_l = at;
        float* w_l = at + 3L * K * n;
        ol[l] = at + 4L * K * n;
        at += (4L * K + 3) * n;
        int rc = launch_down(gi[l - 1], i_l, 3 * K, hl[l - 1], wl[l - 1], Hl[l - 1], Wl[l - 1], l == 1, s);
        if (rc == FDN_OK) rc = launch_down(gw[l - 1], w_l, K, hl[l - 1], wl[l - 1], hl[l - 1], wl[l - 1], 0, s);
        if (rc != FDN_OK) return rc;
        gi[l] = i_l, gw[l] = w_l;
    }
    for (int l = L; l >= 0; --l) {
        const bool last = l == L;
        const int gx = cdiv(wl[l], 4);
        hipLaunchKernelGGL(blend_kernel, dim3((unsigned)cdiv((long)gx * hl[l], 256)), dim3(256), 0, s, gi[l], gw[l], last ? nullptr : gi[l + 1],
                           last ? nullptr : (const float*)ol[l + 1], ol[l], K, hl[l], wl[l], Hl[l], Wl[l], last ? 1 : hl[l + 1], last ? 1 : wl[l + 1],
                           gx, l == 0);
    }
    return fdn_launch_status();
}
