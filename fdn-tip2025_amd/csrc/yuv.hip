// Video frames either side of the LPNet -> FDN forward (include/fdn_video.h; no reference counterpart, the reference reads PNGs):
//   fdn_pre_yuv420  : Y'CbCr 4:2:0 frames, 8 or 10 bit, planar or semi-planar -> fp32 R'G'B' planes, reflect-padded like fdn_pre_u8
//   fdn_post_yuv420 : fp32 R'G'B' planes -> crop -> Y'CbCr 4:2:0 frames of the same layout
// straight between the codec's samples and fp32, so a frame is rounded once on the way out and never passes through 8-bit RGB.
// HBM-bound reshuffles like harness.hip's pair: about 12 B of fp32 per pixel against 1.5 - 3 B of samples.  Both kernels run with FMA
// contraction off, so every operation rounds once and the bounds of tests/test_gpu_yuv.py can be derived.
#include "common.hpp"

#include "../../include/fdn_video.h"

namespace {

// where the chroma samples lie, relative to the first sample after the luma plane: U at [i * cstep], V at [voff + i * cstep]
struct yuv_layout {
    long voff;
    int cstep;
    int center;             // chroma_loc
};

struct yuv_pre {
    yuv_layout l;
    int maxcode;            // 2^bits - 1: a 10-bit word above it counts as it
    int y_off, c_off16;     // 16 s | 0;  16 x (128 s | 2^(bits - 1))
    float y_div, c_div16;   // 219 s | 2^bits - 1;  16 x (224 s | 2^bits - 1)
    float r_cr, g_cb, g_cr, b_cb;
};

struct yuv_post {
    yuv_layout l;
    float kr, kg, kb, cb_div, cr_div;
    float y_scale, y_add, c_scale, c_add, top;
};

__device__ __forceinline__ float clamp01(float f) { return fminf(fmaxf(f, 0.f), 1.f); }

// One thread per output pixel: one luma read, eight chroma reads that neighbouring threads share (cache), three coalesced plane stores.
template <typename T>
__global__ __launch_bounds__(256) void pre_yuv420_kernel(const T* __restrict__ frames, float* __restrict__ out, int h, int w, int H, int W,
                                                         yuv_pre p) {
#pragma clang fp contract(off)
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y, b = blockIdx.z;
    if (x >= W) return;
    const int sy = y < h ? y : 2 * (h - 1) - y;                    // as pre_u8_kernel: F.pad(mode='reflect')
    const int sx = x < w ? x : 2 * (w - 1) - x;
    const int ch = h >> 1, cw = w >> 1;
    const long luma = (long)h * w;
    const T* f = frames + (long)b * (luma + (luma >> 1));
    const T* c = f + luma;
    // chroma row j sits on luma row 2 j + 0.5: 3/4 of row sy / 2, 1/4 of the row on the other side of sy; indices clamped to the frame
    const int j = sy >> 1, k = sx >> 1;
    const int j2 = (sy & 1) ? min(j + 1, ch - 1) : max(j - 1, 0);
    int k2, wa;                                                    // weights wa, 4 - wa (quarters) on columns k, k2
    if (p.l.center) {
        k2 = (sx & 1) ? min(k + 1, cw - 1) : max(k - 1, 0);
        wa = 3;
    } else {
        k2 = min(k + 1, cw - 1);
        wa = (sx & 1) ? 2 : 4;
    }
    const int wb = 4 - wa;
    const long a1 = ((long)j * cw + k) * p.l.cstep, b1 = ((long)j * cw + k2) * p.l.cstep;
    const long a2 = ((long)j2 * cw + k) * p.l.cstep, b2 = ((long)j2 * cw + k2) * p.l.cstep;
    int cs[2];                                                     // 16 x the interpolated code: an exact integer
#pragma unroll
    for (int v = 0; v < 2; ++v) {
        const T* q = c + (v ? p.l.voff : 0);
        cs[v] = 3 * (wa * min((int)q[a1], p.maxcode) + wb * min((int)q[b1], p.maxcode)) +
                (wa * min((int)q[a2], p.maxcode) + wb * min((int)q[b2], p.maxcode));
    }
    const float Y = (float)(min((int)f[(long)sy * w + sx], p.maxcode) - p.y_off) / p.y_div;
    const float Cb = (float)(cs[0] - p.c_off16) / p.c_div16, Cr = (float)(cs[1] - p.c_off16) / p.c_div16;
    const float R = Y + p.r_cr * Cr;
    const float G = (Y - p.g_cb * Cb) - p.g_cr * Cr;
    const float Bl = Y + p.b_cb * Cb;
    float* o = out + (long)b * 3 * H * W + (long)y * W + x;
    const long hw = (long)H * W;
    o[0] = clamp01(R);                                             // out of gamut would be NaN in FDN's 1 - pow(1 - x, .)
    o[hw] = clamp01(G);
    o[2 * hw] = clamp01(Bl);
}

// One thread per 2 x 2 luma quad: its four pixels (and, for chroma_loc left, the column to their left) -> four Y and one Cb / Cr pair.
template <typename T>
__global__ __launch_bounds__(256) void post_yuv420_kernel(const float* __restrict__ res, T* __restrict__ frames, int h, int w, int H, int W,
                                                          yuv_post p) {
#pragma clang fp contract(off)
    const int k = blockIdx.x * 256 + threadIdx.x, j = blockIdx.y, b = blockIdx.z;
    const int cw = w >> 1;
    if (k >= cw) return;
    const long hw = (long)H * W, luma = (long)h * w;
    const float* r = res + (long)b * 3 * hw;
    T* f = frames + (long)b * (luma + (luma >> 1));
    const int x0 = 2 * k, y0 = 2 * j;
    float cb[3], cr[3], Y[2][2];                                   // columns x0, x0 + 1 and (left) max(x0 - 1, 0): the mean of the two rows
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        if (c == 2 && p.l.center) break;
        const int x = c == 2 ? max(x0 - 1, 0) : x0 + c;           // x0 + 1 <= w - 1: w is even; the padding is never read
        float vb[2], vr[2];
#pragma unroll
        for (int dy = 0; dy < 2; ++dy) {
            const float* q = r + (long)(y0 + dy) * W + x;
            const float R = clamp01(q[0]), G = clamp01(q[hw]), Bl = clamp01(q[2 * hw]);
            const float yy = (p.kr * R + p.kg * G) + p.kb * Bl;
            vb[dy] = (Bl - yy) / p.cb_div;
            vr[dy] = (R - yy) / p.cr_div;
            if (c < 2) Y[dy][c] = yy;
        }
        cb[c] = (vb[0] + vb[1]) * 0.5f;
        cr[c] = (vr[0] + vr[1]) * 0.5f;
    }
    float Cb, Cr;
    if (p.l.center) {
        Cb = (cb[0] + cb[1]) * 0.5f;
        Cr = (cr[0] + cr[1]) * 0.5f;
    } else {
        Cb = ((cb[2] + 2.0f * cb[0]) + cb[1]) * 0.25f;
        Cr = ((cr[2] + 2.0f * cr[0]) + cr[1]) * 0.25f;
    }
#pragma unroll
    for (int dy = 0; dy < 2; ++dy)
#pragma unroll
        for (int c = 0; c < 2; ++c)
            f[(long)(y0 + dy) * w + x0 + c] = (T)fminf(fmaxf(rintf(Y[dy][c] * p.y_scale + p.y_add), 0.f), p.top);   // rintf: half to even
    T* q = f + luma + ((long)j * cw + k) * p.l.cstep;
    q[0] = (T)fminf(fmaxf(rintf(Cb * p.c_scale + p.c_add), 0.f), p.top);
    q[p.l.voff] = (T)fminf(fmaxf(rintf(Cr * p.c_scale + p.c_add), 0.f), p.top);
}

bool yuv_args_ok(const void* a, const void* b, int B, int h, int w, int H, int W, int layout, int bits, int matrix, int full_range,
                 int chroma_loc) {
    const auto flag = [](int v) { return v == 0 || v == 1; };
    return a && b && B > 0 && B < 65536 && h >= 2 && w >= 2 && h % 2 == 0 && w % 2 == 0 && H >= h && W >= w && (bits == 8 || bits == 10) &&
           flag(layout) && !(layout == 1 && bits == 10) && flag(matrix) && flag(full_range) && flag(chroma_loc);
}

yuv_layout yuv_layout_of(int h, int w, int layout, int chroma_loc) {
    return layout == 1 ? yuv_layout{1, 2, chroma_loc} : yuv_layout{(long)(h / 2) * (w / 2), 1, chroma_loc};
}

void yuv_matrix(int matrix, double& kr, double& kg, double& kb) {
    kr = matrix == 1 ? 0.2126 : 0.299;
    kb = matrix == 1 ? 0.0722 : 0.114;
    kg = 1.0 - kr - kb;
}

}  // namespace

extern "C" int fdn_video_abi_version(void) { return FDN_VIDEO_ABI_VERSION; }

extern "C" int fdn_pre_yuv420(const void* frames, float* out, int B, int h, int w, int H, int W, int layout, int bits, int matrix,
                              int full_range, int chroma_loc, fdn_stream_t stream) {
    FDN_CHECK_ARG(yuv_args_ok(frames, out, B, h, w, H, W, layout, bits, matrix, full_range, chroma_loc) && H < 65536);
    FDN_CHECK_ARG(H - h < h && W - w < w);                          // reflect padding needs pad < size
    double kr, kg, kb;
    yuv_matrix(matrix, kr, kg, kb);
    const int s = 1 << (bits - 8), top = (1 << bits) - 1;
    yuv_pre p;
    p.l = yuv_layout_of(h, w, layout, chroma_loc);
    p.maxcode = top;
    p.y_off = full_range ? 0 : 16 * s;
    p.y_div = full_range ? (float)top : (float)(219 * s);
    p.c_off16 = 16 * 128 * s;
    p.c_div16 = full_range ? (float)(16 * top) : (float)(16 * 224 * s);
    p.r_cr = (float)(2.0 * (1.0 - kr));
    p.b_cb = (float)(2.0 * (1.0 - kb));
    p.g_cb = (float)(2.0 * kb * (1.0 - kb) / kg);
    p.g_cr = (float)(2.0 * kr * (1.0 - kr) / kg);
    const dim3 grid(cdiv(W, 256), H, B);
    if (bits == 8)
        hipLaunchKernelGGL(pre_yuv420_kernel<unsigned char>, grid, dim3(256), 0, static_cast<hipStream_t>(stream),
                           static_cast<const unsigned char*>(frames), out, h, w, H, W, p);
    else
        hipLaunchKernelGGL(pre_yuv420_kernel<unsigned short>, grid, dim3(256), 0, static_cast<hipStream_t>(stream),
                           static_cast<const unsigned short*>(frames), out, h, w, H, W, p);
    return fdn_launch_status();
}

extern "C" int fdn_post_yuv420(const float* res, void* frames, int B, int h, int w, int H, int W, int layout, int bits, int matrix,
                               int full_range, int chroma_loc, fdn_stream_t stream) {
    FDN_CHECK_ARG(yuv_args_ok(res, frames, B, h, w, H, W, layout, bits, matrix, full_range, chroma_loc) && h < 65536);
    double kr, kg, kb;
    yuv_matrix(matrix, kr, kg, kb);
    const int s = 1 << (bits - 8), top = (1 << bits) - 1;
    yuv_post p;
    p.l = yuv_layout_of(h, w, layout, chroma_loc);
    p.kr = (float)kr;
    p.kg = (float)kg;
    p.kb = (float)kb;
    p.cb_div = (float)(2.0 * (1.0 - kb));
    p.cr_div = (float)(2.0 * (1.0 - kr));
    p.y_scale = full_range ? (float)top : (float)(219 * s);
    p.y_add = full_range ? 0.f : (float)(16 * s);
    p.c_scale = full_range ? (float)top : (float)(224 * s);
    p.c_add = (float)(128 * s);
    p.top = (float)top;
    const dim3 grid(cdiv(w / 2, 256), h / 2, B);
    if (bits == 8)
        hipLaunchKernelGGL(post_yuv420_kernel<unsigned char>, grid, dim3(256), 0, static_cast<hipStream_t>(stream), res,
                           static_cast<unsigned char*>(frames), h, w, H, W, p);
    else
        hipLaunchKernelGGL(post_yuv420_kernel<unsigned short>, grid, dim3(256), 0, static_cast<hipStream_t>(stream), res,
                           static_cast<unsigned short*>(frames), h, w, H, W, p);
    return fdn_launch_status();
}
