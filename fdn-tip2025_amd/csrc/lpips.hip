// LPIPS v0.1 (Zhang et al. 2018; the `lpips` package's LPIPS(net='vgg' | 'alex', version='0.1') in eval mode) around the backbone
// convs, which run on fdn_conv2d with FDN_ACT_RELU:
//   fdn_lpips_prep_u8  : 8-bit HWC images (B, G, R or R, G, B) -> the scaling layer's output [B][3][h][w], in the float32 op order of
//                        the reference's scripts/metrics/calculate_lpips.py: / 255, normalize(mean = std = .5), (x - shift) / scale
//   fdn_lpips_prep_f32 : the same from float planes in [0, 1] (lpips' normalize=True: 2 x - 1) or already in [-1, 1]
//   fdn_maxpool2d      : nn.MaxPool2d(k, s) without padding, floor mode, over planes
//   fdn_lpips_layer    : one tap for B pairs: the two channel norms, the weighted squared difference of the normalised vectors, the
//                        spatial mean - fp64 sums, fixed-order partials and a fixed-order final sum (no atomics): the result does not
//                        depend on the batch, on the order of a pair or on the run
// The float32 roundings of the reference are part of what it computes, and a contracted a * ra - b * rb would not be symmetric in
// the pair, so contraction into FMAs is off in this file.
#include "common.hpp"

#pragma clang fp contract(off)

namespace {

__device__ __forceinline__ float lpips_scale(float v, int c) {
    // ScalingLayer: torch.Tensor([-.030, -.088, -.188]) and ([.458, .448, .450]), float32 roundings of the double literals
    const float shift = c == 0 ? (float)-.030 : (c == 1 ? (float)-.088 : (float)-.188);
    const float scale = c == 0 ? (float).458 : (c == 1 ? (float).448 : (float).450);
    return (v - shift) / scale;
}

__global__ __launch_bounds__(256) void lpips_prep_u8_kernel(const unsigned char* __restrict__ src, float* __restrict__ out, long hw, int bgr) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= hw) return;
    const int b = blockIdx.y;
    const unsigned char* p = src + ((long)b * hw + i) * 3;
    float* o = out + (long)b * 3 * hw + i;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float v = (float)p[bgr ? 2 - c : c] / 255.0f;
        v = (v - 0.5f) / 0.5f;                                     // torchvision normalize: sub_(mean).div_(std)
        o[c * hw] = lpips_scale(v, c);
    }
}

__global__ __launch_bounds__(256) void lpips_prep_f32_kernel(const float* __restrict__ x, float* __restrict__ out, long hw, int from01) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= hw) return;
    const long base = (long)blockIdx.y * 3 * hw + i;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float v = x[base + c * hw];
        if (from01) v = 2.0f * v - 1.0f;
        out[base + c * hw] = lpips_scale(v, c);
    }
}

// one output element per thread; NaN propagates as in torch's max_pool2d (a NaN in the window wins)
__global__ __launch_bounds__(256) void maxpool2d_kernel(const float* __restrict__ x, float* __restrict__ out, long total, int H, int W, int OH,
                                                        int OW, int k, int s) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const long ohw = (long)OH * OW;
    const long pl = i / ohw;
    const int r = (int)(i - pl * ohw);
    const int oy = r / OW, ox = r - oy * OW;
    const float* p = x + pl * H * W + (long)(oy * s) * W + ox * s;
    float m = -INFINITY;
    for (int ky = 0; ky < k; ++ky)
        for (int kx = 0; kx < k; ++kx) {
            const float v = p[(long)ky * W + kx];
            if (v > m || isnan(v)) m = v;
        }
    out[i] = m;
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// workgroup `blockIdx.x` of pair b walks pixels blockIdx.x * 256 + tid + k * nparts * 256 in order; its sum lands in part[b][blockIdx.x].
// nparts depends on P alone, so every sum is formed in the same order whatever the batch.
__global__ __launch_bounds__(256) void lpips_layer_kernel(const float* __restrict__ f, const float* __restrict__ w, double* __restrict__ part,
                                                          int B, int C, long P, int nparts) {
    __shared__ double wsum[4];
    const int b = blockIdx.y, tid = threadIdx.x;
    const float* f0 = f + (long)b * C * P;
    const float* f1 = f + (long)(B + b) * C * P;
    double acc = 0.0;
    for (long p = (long)blockIdx.x * 256 + tid; p < P; p += (long)nparts * 256) {
        double s0 = 0.0, s1 = 0.0;
        for (int c = 0; c < C; ++c) {
            const double a = f0[c * P + p], q = f1[c * P + p];
            s0 += a * a;
            s1 += q * q;
        }
        const double ra = 1.0 / (sqrt(s0) + 1e-10), rb = 1.0 / (sqrt(s1) + 1e-10);      // normalize_tensor(eps=1e-10)
        double d = 0.0;
        for (int c = 0; c < C; ++c) {
            const double x = (double)f0[c * P + p] * ra - (double)f1[c * P + p] * rb;
            d += (double)w[c] * x * x;
        }
        acc += d;
    }
    acc = wave_sum(acc);
    if ((tid & 63) == 0) wsum[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0) part[(long)b * nparts + blockIdx.x] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
}

// one workgroup per pair: the nparts partials in a fixed order, then the mean over the P pixels
__global__ __launch_bounds__(256) void lpips_finish_kernel(const double* __restrict__ part, double* __restrict__ out, int nparts, long P,
                                                           int accumulate) {
    __shared__ double wsum[4];
    const int b = blockIdx.x, tid = threadIdx.x;
    double acc = 0.0;
    for (int i = tid; i < nparts; i += 256) acc += part[(long)b * nparts + i];
    acc = wave_sum(acc);
    if ((tid & 63) == 0) wsum[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0) {
        const double mean = (((wsum[0] + wsum[1]) + wsum[2]) + wsum[3]) / (double)P;
        out[b] = accumulate ? out[b] + mean : mean;
    }
}

}  // namespace

extern "C" int fdn_lpips_prep_u8(const unsigned char* src, float* out, int B, int H, int W, int bgr, fdn_stream_t stream) {
    FDN_CHECK_ARG(src && out && B > 0 && B <= 65535 && H > 0 && W > 0 && (bgr == 0 || bgr == 1));
    const long hw = (long)H * W;
    hipLaunchKernelGGL(lpips_prep_u8_kernel, dim3((unsigned)cdiv(hw, 256L), (unsigned)B), dim3(256), 0, static_cast<hipStream_t>(stream),
                       src, out, hw, bgr);
    return fdn_launch_status();
}

extern "C" int fdn_lpips_prep_f32(const float* x, float* out, int B, int H, int W, int from01, fdn_stream_t stream) {
    FDN_CHECK_ARG(x && out && B > 0 && B <= 65535 && H > 0 && W > 0 && (from01 == 0 || from01 == 1));
    const long hw = (long)H * W;
    hipLaunchKernelGGL(lpips_prep_f32_kernel, dim3((unsigned)cdiv(hw, 256L), (unsigned)B), dim3(256), 0, static_cast<hipStream_t>(stream),
                       x, out, hw, from01);
    return fdn_launch_status();
}

extern "C" int fdn_maxpool2d(const float* x, float* out, long planes, int H, int W, int k, int s, fdn_stream_t stream) {
    FDN_CHECK_ARG(x && out && planes > 0 && H > 0 && W > 0 && k > 0 && s > 0 && H >= k && W >= k);
    const int OH = (H - k) / s + 1, OW = (W - k) / s + 1;
    const long total = planes * OH * OW;
    FDN_CHECK_ARG(total <= 0xFFFFFF00L);                           // grid.x * 256 threads within 32 bits
    hipLaunchKernelGGL(maxpool2d_kernel, dim3((unsigned)cdiv(total, 256L)), dim3(256), 0, static_cast<hipStream_t>(stream), x, out, total, H,
                       W, OH, OW, k, s);
    return fdn_launch_status();
}

extern "C" int fdn_lpips_layer(const float* f, const float* w, double* out, int B, int C, int H, int W, int accumulate, double* ws,
                               fdn_stream_t stream) {
    FDN_CHECK_ARG(f && w && out && ws && B > 0 && B <= 65535 && C > 0 && H > 0 && W > 0 && (accumulate == 0 || accumulate == 1));
    const long P = (long)H * W;
    const int nparts = (int)(cdiv(P, 256L) < FDN_LPIPS_PARTS ? cdiv(P, 256L) : FDN_LPIPS_PARTS);
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(lpips_layer_kernel, dim3((unsigned)nparts, (unsigned)B), dim3(256), 0, s, f, w, ws, B, C, P, nparts);
    hipLaunchKernelGGL(lpips_finish_kernel, dim3((unsigned)B), dim3(256), 0, s, ws, out, nparts, P, accumulate);
    return fdn_launch_status();
}
