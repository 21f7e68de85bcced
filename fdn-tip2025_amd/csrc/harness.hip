// The step either side of the LPNet -> FDN forward, on the GPU:
//   fdn_pre_u8  : uint8 HWC image(s) -> /255 fp32 -> RGB CHW -> reflect-pad bottom/right to the x32 grid
//                 (inference_fdn_lolblur.py:47-62, basicsr/utils/img_util.py:9-33)
//   fdn_post_u8 : crop -> clamp(0,1) -> *255 -> round half-to-even -> uint8 HWC, RGB -> BGR
//                 (inference_fdn_lolblur.py:72-75, basicsr/utils/img_util.py:36-98)
//   fdn_tiles_gather_u8 / fdn_tiles_merge_u8 : the tiled path's pair between a uint8 frame and fp32 tiles (ABI 21)
//   fdn_tiles_merge_w / fdn_tiles_merge_w_u8 : the merge with per-tile weights (feathered seams) instead of the uniform average
// Pure byte <-> float reshuffles, HBM-bound: a thread owns one pixel (3 bytes in, 3 coalesced plane
// stores out, or the reverse).
#include "common.hpp"

namespace {

__global__ __launch_bounds__(256) void pre_u8_kernel(const unsigned char* __restrict__ img, float* __restrict__ out, int h, int w,
                                                     int H, int W, int swap_rb) {
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y, b = blockIdx.z;
    if (x >= W) return;
    const int sy = y < h ? y : 2 * (h - 1) - y;                    // F.pad(mode='reflect'): no edge repeat
    const int sx = x < w ? x : 2 * (w - 1) - x;
    const unsigned char* p = img + (((long)b * h + sy) * w + sx) * 3;
    const float c0 = (float)p[0] / 255.0f, c1 = (float)p[1] / 255.0f, c2 = (float)p[2] / 255.0f;   // true division, as numpy's
    float* o = out + (long)b * 3 * H * W + (long)y * W + x;
    const long hw = (long)H * W;
    o[0] = swap_rb ? c2 : c0;
    o[hw] = c1;
    o[2 * hw] = swap_rb ? c0 : c2;
}

__global__ __launch_bounds__(256) void post_u8_kernel(const float* __restrict__ res, unsigned char* __restrict__ out, int h, int w,
                                                      int H, int W, int swap_rb) {
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y, b = blockIdx.z;
    if (x >= w) return;
    const float* r = res + (long)b * 3 * H * W + (long)y * W + x;
    const long hw = (long)H * W;
    unsigned char v[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float f = r[c * hw];
        f = f < 0.f ? 0.f : (f > 1.f ? 1.f : f);                    // clamp_(0, 1)
        v[c] = (unsigned char)rintf(f * 255.0f);                    // numpy .round(): half to even
    }
    unsigned char* o = out + (((long)b * h + y) * w + x) * 3;
    o[0] = swap_rb ? v[2] : v[0];
    o[1] = v[1];
    o[2] = swap_rb ? v[0] : v[2];
}

// Tiled inference (ImageRestorationModel.grids / grids_inverse, image_restoration_model.py:261-339, scale 1):
// gather: tile t = x[:, i_t : i_t + ch, j_t : j_t + cw]; merge: every output pixel adds the tiles covering it in tile
// order (the order of the reference's accumulation loop, so the fp32 sum is the same) and divides by their count.
__global__ __launch_bounds__(256) void tiles_gather_kernel(const float* __restrict__ x, float* __restrict__ tiles,
                                                           const int* __restrict__ ij, int C, int H, int W, int ch, int cw) {
    const int px = blockIdx.x * 256 + threadIdx.x, c = blockIdx.y, t = blockIdx.z;
    if (px >= ch * cw) return;
    const int y = px / cw, xx = px - y * cw;
    const int i = ij[2 * t], j = ij[2 * t + 1];
    tiles[(((long)t * C + c) * ch + y) * cw + xx] = x[((long)c * H + i + y) * W + j + xx];
}

__global__ __launch_bounds__(256) void tiles_merge_kernel(const float* __restrict__ tiles, float* __restrict__ out,
                                                          const int* __restrict__ ij, int T, int C, int H, int W, int ch, int cw) {
    const int px = blockIdx.x * 256 + threadIdx.x, c = blockIdx.y;
    if (px >= H * W) return;
    const int y = px / W, xx = px - y * W;
    float acc = 0.f, cnt = 0.f;
    for (int t = 0; t < T; ++t) {
        const int dy = y - ij[2 * t], dx = xx - ij[2 * t + 1];
        if (dy >= 0 && dy < ch && dx >= 0 && dx < cw) {
            acc += tiles[(((long)t * C + c) * ch + dy) * cw + dx];
            cnt += 1.0f;
        }
    }
    out[(long)c * H * W + px] = acc / cnt;
}

// The same pair between a uint8 HWC frame and fp32 tiles, without the frame-sized fp32 image in between: gather = pre_u8_kernel's
// /255 and channel order (no padding: tiles are cut from the frame itself) + tiles_gather_kernel's indexing; merge =
// tiles_merge_kernel's ordered sum and division + post_u8_kernel's clamp and rounding.  Same operations on the same values in the
// same order, so both equal the two-launch compositions bit for bit.  A thread owns one pixel and its three channels.
__global__ __launch_bounds__(256) void tiles_gather_u8_kernel(const unsigned char* __restrict__ img, float* __restrict__ tiles,
                                                              const int* __restrict__ ij, int h, int w, int ch, int cw, int swap_rb) {
    const long px = (long)blockIdx.x * 256 + threadIdx.x, plane = (long)ch * cw;
    const int t = blockIdx.z;
    if (px >= plane) return;
    const int y = (int)(px / cw), xx = (int)(px - (long)y * cw);
    const int i = ij[2 * t], j = ij[2 * t + 1];
    if (i < 0 || j < 0 || i > h - ch || j > w - cw) return;        // an origin outside the frame: nothing is read
    const unsigned char* p = img + ((long)(i + y) * w + j + xx) * 3;
    const float c0 = (float)p[0] / 255.0f, c1 = (float)p[1] / 255.0f, c2 = (float)p[2] / 255.0f;   // true division, as pre_u8_kernel
    float* o = tiles + (long)t * 3 * plane + px;
    o[0] = swap_rb ? c2 : c0;
    o[plane] = c1;
    o[2 * plane] = swap_rb ? c0 : c2;
}

__global__ __launch_bounds__(256) void tiles_merge_u8_kernel(const float* __restrict__ tiles, unsigned char* __restrict__ out,
                                                             const int* __restrict__ ij, int T, int h, int w, int ch, int cw, int swap_rb) {
    const long px = (long)blockIdx.x * 256 + threadIdx.x;
    if (px >= (long)h * w) return;
    const int y = (int)(px / w), xx = (int)(px - (long)y * w);
    const long plane = (long)ch * cw;
    float acc[3] = {0.f, 0.f, 0.f}, cnt = 0.f;
    for (int t = 0; t < T; ++t) {
        const int dy = y - ij[2 * t], dx = xx - ij[2 * t + 1];
        if (dy >= 0 && dy < ch && dx >= 0 && dx < cw) {
            const float* s = tiles + (long)t * 3 * plane + (long)dy * cw + dx;
#pragma unroll
            for (int c = 0; c < 3; ++c) acc[c] += s[c * plane];
            cnt += 1.0f;
        }
    }
    unsigned char v[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float f = acc[c] / cnt;
        f = f < 0.f ? 0.f : (f > 1.f ? 1.f : f);                    // clamp_(0, 1)
        v[c] = (unsigned char)rintf(f * 255.0f);                    // numpy .round(): half to even
    }
    unsigned char* o = out + px * 3;
    o[0] = swap_rb ? v[2] : v[0];
    o[1] = v[1];
    o[2] = swap_rb ? v[0] : v[2];
}

// The feathered merge (no reference counterpart): tile t weighs its pixel (dy, dx) with wy[t][dy] * wx[t][dx] - ramps across the overlap
// with its neighbours, 1 elsewhere (fdn_hip.tiling.feather_weights) - and the pixel is sum(w x) / sum(w) over the tiles covering it, in
// tile order.  One accumulate routine for both forms, NC channels of one pixel at a time, with contraction off: every product and every
// add rounds once, whatever the compiler would make of either instantiation, so the u8 form equals the fp32 form + post_u8_kernel bit for
// bit.  s: the first of the pixel's NC planes in tile 0.
template <int NC>
__device__ __forceinline__ float merge_w_accumulate(const float* __restrict__ s, const int* __restrict__ ij, const float* __restrict__ wy,
                                                    const float* __restrict__ wx, int T, long tile_stride, long plane, int ch, int cw, int y,
                                                    int xx, float (&acc)[NC]) {
#pragma clang fp contract(off)
    float wsum = 0.f;
#pragma unroll
    for (int c = 0; c < NC; ++c) acc[c] = 0.f;
    for (int t = 0; t < T; ++t) {
        const int dy = y - ij[2 * t], dx = xx - ij[2 * t + 1];
        if (dy >= 0 && dy < ch && dx >= 0 && dx < cw) {
            const float wgt = wy[(long)t * ch + dy] * wx[(long)t * cw + dx];
            const float* p = s + t * tile_stride + (long)dy * cw + dx;
#pragma unroll
            for (int c = 0; c < NC; ++c) acc[c] = acc[c] + wgt * p[c * plane];
            wsum = wsum + wgt;
        }
    }
    return wsum;
}

__global__ __launch_bounds__(256) void tiles_merge_w_kernel(const float* __restrict__ tiles, float* __restrict__ out,
                                                            const int* __restrict__ ij, const float* __restrict__ wy,
                                                            const float* __restrict__ wx, int T, int C, int H, int W, int ch, int cw) {
    const long px = (long)blockIdx.x * 256 + threadIdx.x;
    const int c = blockIdx.y;
    if (px >= (long)H * W) return;
    const int y = (int)(px / W), xx = (int)(px - (long)y * W);
    const long plane = (long)ch * cw;
    float acc[1];
    const float wsum = merge_w_accumulate<1>(tiles + c * plane, ij, wy, wx, T, C * plane, plane, ch, cw, y, xx, acc);
    out[(long)c * H * W + px] = acc[0] / wsum;
}

__global__ __launch_bounds__(256) void tiles_merge_w_u8_kernel(const float* __restrict__ tiles, unsigned char* __restrict__ out,
                                                               const int* __restrict__ ij, const float* __restrict__ wy,
                                                               const float* __restrict__ wx, int T, int h, int w, int ch, int cw,
                                                               int swap_rb) {
    const long px = (long)blockIdx.x * 256 + threadIdx.x;
    if (px >= (long)h * w) return;
    const int y = (int)(px / w), xx = (int)(px - (long)y * w);
    const long plane = (long)ch * cw;
    float acc[3];
    const float wsum = merge_w_accumulate<3>(tiles, ij, wy, wx, T, 3 * plane, plane, ch, cw, y, xx, acc);
    unsigned char v[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float f = acc[c] / wsum;
        f = f < 0.f ? 0.f : (f > 1.f ? 1.f : f);                    // clamp_(0, 1)
        v[c] = (unsigned char)rintf(f * 255.0f);                    // numpy .round(): half to even
    }
    unsigned char* o = out + px * 3;
    o[0] = swap_rb ? v[2] : v[0];
    o[1] = v[1];
    o[2] = swap_rb ? v[0] : v[2];
}

}  // namespace

extern "C" int fdn_tiles_gather(const float* x, float* tiles, const int* ij, int T, int C, int H, int W, int ch, int cw,
                                fdn_stream_t stream) {
    FDN_CHECK_ARG(x && tiles && ij && T > 0 && C > 0 && H > 0 && W > 0 && ch > 0 && cw > 0 && ch <= H && cw <= W && C < 65536 && T < 65536);
    hipLaunchKernelGGL(tiles_gather_kernel, dim3(cdiv((long)ch * cw, 256), C, T), dim3(256), 0, static_cast<hipStream_t>(stream), x,
                       tiles, ij, C, H, W, ch, cw);
    return fdn_launch_status();
}

extern "C" int fdn_tiles_merge(const float* tiles, float* out, const int* ij, int T, int C, int H, int W, int ch, int cw,
                               fdn_stream_t stream) {
    FDN_CHECK_ARG(tiles && out && ij && T > 0 && C > 0 && H > 0 && W > 0 && ch > 0 && cw > 0 && ch <= H && cw <= W && C < 65536);
    hipLaunchKernelGGL(tiles_merge_kernel, dim3(cdiv((long)H * W, 256), C), dim3(256), 0, static_cast<hipStream_t>(stream), tiles, out,
                       ij, T, C, H, W, ch, cw);
    return fdn_launch_status();
}

extern "C" int fdn_tiles_gather_u8(const unsigned char* img, float* tiles, const int* ij, int T, int h, int w, int ch, int cw,
                                   int swap_rb, fdn_stream_t stream) {
    FDN_CHECK_ARG(img && tiles && ij && T > 0 && h > 0 && w > 0 && ch > 0 && cw > 0 && ch <= h && cw <= w && T < 65536);
    hipLaunchKernelGGL(tiles_gather_u8_kernel, dim3(cdiv((long)ch * cw, 256), 1, T), dim3(256), 0, static_cast<hipStream_t>(stream), img,
                       tiles, ij, h, w, ch, cw, swap_rb);
    return fdn_launch_status();
}

extern "C" int fdn_tiles_merge_u8(const float* tiles, unsigned char* out, const int* ij, int T, int h, int w, int ch, int cw,
                                  int swap_rb, fdn_stream_t stream) {
    FDN_CHECK_ARG(tiles && out && ij && T > 0 && h > 0 && w > 0 && ch > 0 && cw > 0 && ch <= h && cw <= w && T < 65536);
    hipLaunchKernelGGL(tiles_merge_u8_kernel, dim3(cdiv((long)h * w, 256)), dim3(256), 0, static_cast<hipStream_t>(stream), tiles, out,
                       ij, T, h, w, ch, cw, swap_rb);
    return fdn_launch_status();
}

extern "C" int fdn_tiles_merge_w(const float* tiles, float* out, const int* ij, const float* wy, const float* wx, int T, int C, int H,
                                 int W, int ch, int cw, fdn_stream_t stream) {
    FDN_CHECK_ARG(tiles && out && ij && wy && wx && T > 0 && C > 0 && H > 0 && W > 0 && ch > 0 && cw > 0 && ch <= H && cw <= W && C < 65536 &&
                  T < 65536);
    hipLaunchKernelGGL(tiles_merge_w_kernel, dim3(cdiv((long)H * W, 256), C), dim3(256), 0, static_cast<hipStream_t>(stream), tiles, out,
                       ij, wy, wx, T, C, H, W, ch, cw);
    return fdn_launch_status();
}

extern "C" int fdn_tiles_merge_w_u8(const float* tiles, unsigned char* out, const int* ij, const float* wy, const float* wx, int T, int h,
                                    int w, int ch, int cw, int swap_rb, fdn_stream_t stream) {
    FDN_CHECK_ARG(tiles && out && ij && wy && wx && T > 0 && h > 0 && w > 0 && ch > 0 && cw > 0 && ch <= h && cw <= w && T < 65536);
    hipLaunchKernelGGL(tiles_merge_w_u8_kernel, dim3(cdiv((long)h * w, 256)), dim3(256), 0, static_cast<hipStream_t>(stream), tiles, out,
                       ij, wy, wx, T, h, w, ch, cw, swap_rb);
    return fdn_launch_status();
}

extern "C" int fdn_pre_u8(const unsigned char* img, float* out, int B, int h, int w, int H, int W, int swap_rb,
                          fdn_stream_t stream) {
    FDN_CHECK_ARG(img && out && B > 0 && h > 0 && w > 0 && H >= h && W >= w && B < 65536 && H < 65536);
    FDN_CHECK_ARG(H - h < h && W - w < w);                          // reflect padding needs pad < size
    hipLaunchKernelGGL(pre_u8_kernel, dim3(cdiv(W, 256), H, B), dim3(256), 0, static_cast<hipStream_t>(stream), img, out, h, w, H,
                       W, swap_rb);
    return fdn_launch_status();
}

extern "C" int fdn_post_u8(const float* res, unsigned char* out, int B, int h, int w, int H, int W, int swap_rb,
                           fdn_stream_t stream) {
    FDN_CHECK_ARG(res && out && B > 0 && h > 0 && w > 0 && H >= h && W >= w && B < 65536 && h < 65536);
    hipLaunchKernelGGL(post_u8_kernel, dim3(cdiv(w, 256), h, B), dim3(256), 0, static_cast<hipStream_t>(stream), res, out, h, w, H,
                       W, swap_rb);
    return fdn_launch_status();
}
