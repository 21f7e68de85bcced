// NIQE, the reference's no-reference quality metric (basicsr/metrics/niqe.py:67-205), on the GPU up to the per-block features; the
// 36x36 MVG fit at the end (:141-153) stays on the host.  Three steps, each one launch for a whole batch:
//   fdn_niqe_luma     : the plane NIQE scores - to_y_channel (:197), cv2.cvtColor BGR2GRAY (:199) or the image as it is (input_order
//                       'HW') - cut to the crop_border and to whole 96x96 blocks from the top-left (:203, :104-107)
//   fdn_niqe_mscn     : the mean-subtracted, contrast-normalised plane of one scale (:111-117): 7x7 `convolve(.., mode='nearest')` of
//                       the plane and of its square in fp64, rounded to fp32 where scipy stores them; scale 2 takes the scale-1 plane
//                       through the 2x2 mean its cv2.resize(.., 1/2) is (:134-138) in the tile loader
//   fdn_niqe_features : one workgroup per (image, block): the block in LDS, the five AGGD fits of compute_feature (:40-64) as fp64
//                       sums, the table search of estimate_aggd_param (:21-37) and the 18 features
// The float32 roundings the reference makes are part of what it computes, so contraction into FMAs is off in this file.
#include "common.hpp"

#pragma clang fp contract(off)

namespace {

constexpr int kTile = 16;                 // MSCN: 16x16 outputs per workgroup
constexpr int kApron = 3;                 // 7x7 window
constexpr int kSpan = kTile + 2 * kApron;
constexpr int kMaxBlock = 96;             // features: the largest block (scale 1), 36 KiB of fp32 in LDS

struct Win49 { double w[49]; };

// the plane NIQE scores, one pixel: mode 0 = to_y_channel (3 channels: Y of BT.601; 1 channel: (x / 255) * 255 in float32, what
// metric_util.py:43-47 does to an image that is not 3-channel), 1 = cv2.cvtColor(img / 255., COLOR_BGR2GRAY) * 255. in float32
// (0.114 B + 0.587 G + 0.299 R, summed in that order), 2 = the image as it is (input_order 'HW')
__global__ __launch_bounds__(256) void niqe_luma_kernel(const float* __restrict__ src, float* __restrict__ out, int C, int Hs, int Ws, int top,
                                                        int left, int H, int W, int mode) {
    const long hw = (long)H * W;
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= hw) return;
    const int b = blockIdx.y;
    const int y = (int)(i / W), x = (int)(i % W);
    const long plane = (long)Hs * Ws;
    const float* p = src + (long)b * C * plane + (long)(top + y) * Ws + (left + x);
    float v;
    if (mode == 2) {
        v = p[0];
    } else if (C == 1) {
        v = (p[0] / 255.0f) * 255.0f;
    } else if (mode == 0) {
        v = fdn_bgr_to_y(p[0], p[plane], p[2 * plane]);
    } else {
        const float bb = p[0] / 255.0f, gg = p[plane] / 255.0f, rr = p[2 * plane] / 255.0f;
        v = ((bb * 0.114f + gg * 0.587f) + rr * 0.299f) * 255.0f;
    }
    out[(long)b * hw + i] = v;
}

// MSCN of one 16x16 tile.  src is [B][H][W] (half = 0) or the scale-1 plane [B][2H][2W] (half = 1: float32 img / 255, the 2x2 mean
// ((a + b) + c) + d) * 0.25 with a, b the upper pair, * 255).  The border replicates at the edge of the plane the window runs over.
__global__ __launch_bounds__(256) void niqe_mscn_kernel(const float* __restrict__ src, float* __restrict__ out, int H, int W, int half, Win49 win) {
    __shared__ float img[kSpan][kSpan];
    __shared__ float sq[kSpan][kSpan];
    const int b = blockIdx.z;
    const int oy0 = blockIdx.y * kTile, ox0 = blockIdx.x * kTile;
    const long hw = (long)H * W;
    const float* s = src + (long)b * (half ? 4 * hw : hw);
    for (int t = threadIdx.x; t < kSpan * kSpan; t += 256) {
        const int ty = t / kSpan, tx = t % kSpan;
        const int y = min(max(oy0 + ty - kApron, 0), H - 1), x = min(max(ox0 + tx - kApron, 0), W - 1);   // mode='nearest'
        float v;
        if (half) {
            const float* q = s + (long)(2 * y) * (2 * W) + 2 * x;
            const float a = q[0] / 255.0f, bb = q[1] / 255.0f, c = q[2 * W] / 255.0f, d = q[2 * W + 1] / 255.0f;
            v = ((((a + bb) + c) + d) * 0.25f) * 255.0f;
        } else {
            v = s[(long)y * W + x];
        }
        img[ty][tx] = v;
        sq[ty][tx] = v * v;                                       // np.square(img), float32
    }
    __syncthreads();
    const int ly = threadIdx.x / kTile, lx = threadIdx.x % kTile;
    const int oy = oy0 + ly, ox = ox0 + lx;
    if (oy >= H || ox >= W) return;
    // scipy.ndimage.convolve = correlate with the flipped window, taps in row-major order of the flipped window, float64 sum of
    // float64(input) * weight, stored as float32
    double m = 0.0, q2 = 0.0;
#pragma unroll
    for (int a = 0; a < 7; ++a) {
#pragma unroll
        for (int c = 0; c < 7; ++c) {
            const double w = win.w[(6 - a) * 7 + (6 - c)];
            m = m + (double)img[ly + a][lx + c] * w;
            q2 = q2 + (double)sq[ly + a][lx + c] * w;
        }
    }
    const float mu = (float)m, ex2 = (float)q2;
    const float sigma = sqrtf(fabsf(ex2 - mu * mu));
    out[(long)b * hw + (long)oy * W + ox] = (img[ly + kApron][lx + kApron] - mu) / (sigma + 1.0f);
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// argmin((r_gam - r)^2) over an increasing r_gam: the nearest entry, ties to the lower index; NaN or an infinite r makes every
// squared difference NaN or inf and np.argmin then returns 0 (the reference's alpha = 0.2 quirk)
__device__ int table_index(const double* __restrict__ r_gam, int n, double r) {
    if (!isfinite(r)) return 0;
    int lo = 0, hi = n;                                           // first index with r_gam >= r
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (r_gam[mid] < r) lo = mid + 1; else hi = mid;
    }
    if (lo == 0) return 0;
    if (lo == n) return n - 1;
    const double d0 = r_gam[lo - 1] - r, d1 = r_gam[lo] - r;
    return d1 * d1 < d0 * d0 ? lo : lo - 1;
}

// one workgroup per (block, image).  Block (idx_h, idx_w) of the plane [H][W] at bs = 96 / scale, workgroup index idx_w * nbh + idx_h
// (niqe.py:120-128).  Fit 0 is the block, fits 1..4 block * np.roll(block, s) for s = (0,1), (1,0), (1,1), (1,-1), circular within the
// block, the product in float32.  Per fit: count and sum of x^2 of the negatives and of the positives, sum |x|, sum x^2, in fp64.
// tables [4][ntab]: gam, r_gam, sqrt(G(1/a) / G(3/a)), G(2/a) / G(1/a) (float64, built on the host).  feats [B][nblocks][18].
__global__ __launch_bounds__(256) void niqe_features_kernel(const float* __restrict__ mscn, double* __restrict__ feats, int H, int W, int bs,
                                                            const double* __restrict__ tables, int ntab) {
    __shared__ float blk[kMaxBlock * kMaxBlock];
    __shared__ double part[4][5][6];
    const int nbh = H / bs;
    const int idx = blockIdx.x, b = blockIdx.y;
    const int bw = idx / nbh, bh = idx % nbh;
    const float* p = mscn + (long)b * H * W + (long)(bh * bs) * W + bw * bs;
    const int n = bs * bs;
    for (int t = threadIdx.x; t < n; t += 256) blk[t] = p[(long)(t / bs) * W + t % bs];
    __syncthreads();
    constexpr int sy[5] = {0, 0, 1, 1, 1}, sx[5] = {0, 1, 0, 1, -1};
    double acc[5][6];
#pragma unroll
    for (int f = 0; f < 5; ++f)
#pragma unroll
        for (int k = 0; k < 6; ++k) acc[f][k] = 0.0;
    for (int t = threadIdx.x; t < n; t += 256) {
        const int r = t / bs, c = t % bs;
        const float v = blk[t];
#pragma unroll
        for (int f = 0; f < 5; ++f) {
            float x = v;
            if (f) {
                const int rr = r - sy[f] < 0 ? r - sy[f] + bs : r - sy[f];
                int cc = c - sx[f];
                cc = cc < 0 ? cc + bs : (cc >= bs ? cc - bs : cc);
                x = v * blk[rr * bs + cc];
            }
            const double xd = (double)x, x2 = xd * xd;
            if (x < 0.f) { acc[f][0] += 1.0; acc[f][1] += x2; }
            if (x > 0.f) { acc[f][2] += 1.0; acc[f][3] += x2; }
            acc[f][4] += fabs(xd);
            acc[f][5] += x2;
        }
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int f = 0; f < 5; ++f)
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            const double s = wave_sum(acc[f][k]);
            if (lane == 0) part[wave][f][k] = s;
        }
    __syncthreads();
    const int f = threadIdx.x;
    if (f >= 5) return;
    double S[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) S[k] = ((part[0][f][k] + part[1][f][k]) + part[2][f][k]) + part[3][f][k];
    const double N = (double)n;
    const double left_std = sqrt(S[1] / S[0]), right_std = sqrt(S[3] / S[2]);   // 0 / 0 = NaN: the empty mean of the reference
    const double gh = left_std / right_std;
    const double ma = S[4] / N;
    const double rhat = (ma * ma) / (S[5] / N);
    const double g2p1 = gh * gh + 1.0;
    const double rhatnorm = (rhat * (gh * gh * gh + 1.0) * (gh + 1.0)) / (g2p1 * g2p1);
    const int j = table_index(tables + ntab, ntab, rhatnorm);
    const double alpha = tables[j], ratio = tables[2 * ntab + j];
    const double beta_l = left_std * ratio, beta_r = right_std * ratio;
    double* o = feats + ((long)b * gridDim.x + idx) * 18;
    if (f == 0) {
        o[0] = alpha;
        o[1] = (beta_l + beta_r) / 2.0;
    } else {
        double* q = o + 2 + 4 * (f - 1);
        q[0] = alpha;
        q[1] = (beta_r - beta_l) * tables[3 * ntab + j];          // Eq. 8
        q[2] = beta_l;
        q[3] = beta_r;
    }
}

}  // namespace

extern "C" int fdn_niqe_luma(const float* src, float* out, int B, int C, int Hs, int Ws, int top, int left, int H, int W, int mode,
                             fdn_stream_t stream) {
    FDN_CHECK_ARG(src && out && B > 0 && H > 0 && W > 0 && top >= 0 && left >= 0 && top + H <= Hs && left + W <= Ws);
    FDN_CHECK_ARG((mode == 0 && (C == 1 || C == 3)) || (mode == 1 && C == 3) || (mode == 2 && C == 1));
    const long hw = (long)H * W;
    hipLaunchKernelGGL(niqe_luma_kernel, dim3((unsigned)cdiv(hw, 256L), (unsigned)B), dim3(256), 0, static_cast<hipStream_t>(stream), src,
                       out, C, Hs, Ws, top, left, H, W, mode);
    return fdn_launch_status();
}

extern "C" int fdn_niqe_mscn(const float* src, float* mscn, int B, int H, int W, int half, const double* window49, fdn_stream_t stream) {
    FDN_CHECK_ARG(src && mscn && window49 && B > 0 && H > 0 && W > 0 && (half == 0 || half == 1));
    Win49 win;
    for (int i = 0; i < 49; ++i) win.w[i] = window49[i];
    hipLaunchKernelGGL(niqe_mscn_kernel, dim3((unsigned)cdiv(W, kTile), (unsigned)cdiv(H, kTile), (unsigned)B), dim3(256), 0,
                       static_cast<hipStream_t>(stream), src, mscn, H, W, half, win);
    return fdn_launch_status();
}

extern "C" int fdn_niqe_features(const float* mscn, double* feats, int B, int H, int W, int block, const double* tables, int ntab,
                                 fdn_stream_t stream) {
    FDN_CHECK_ARG(mscn && feats && tables && B > 0 && block > 0 && block <= kMaxBlock && ntab >= 2);
    FDN_CHECK_ARG(H >= block && W >= block && H % block == 0 && W % block == 0);
    const int nblocks = (H / block) * (W / block);
    hipLaunchKernelGGL(niqe_features_kernel, dim3((unsigned)nblocks, (unsigned)B), dim3(256), 0, static_cast<hipStream_t>(stream), mscn,
                       feats, H, W, block, tables, ntab);
    return fdn_launch_status();
}
