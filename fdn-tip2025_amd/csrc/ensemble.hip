// Geometric self-ensemble around the forward (include/fdn_ensemble.h; no reference counterpart): the eight flips and transpositions of a
// frame, made on the way into the network, and the network's results on them folded back into one frame on the way out.
//   fdn_d4_pre_u8  : uint8 HWC frames -> K transformed, reflect-padded fp32 CHW copies (fdn_pre_u8 of each transformed frame)
//   fdn_d4_apply   : the same movement for fp32 CHW input (the tiles of the tiled route)
//   fdn_d4_mean    : K results -> each mapped back, summed in ascending k, divided once by K
//   fdn_d4_post_u8 : the same, then fdn_post_u8's clamp and rounding into uint8 HWC
// Pure movement plus a short ordered sum, HBM-bound.  The four codes without a transposition read and write along rows: a thread owns one
// pixel, as in harness.hip.  The four with one would read columns - a wave fetching 64 cache lines for 192 or 256 bytes - so those go
// through a square LDS tile: rows read coalesced from the source, rows written coalesced to the destination, the tile's pitch odd so
// that the column-wise LDS access in between touches every bank once.
#include "common.hpp"

#include "../../include/fdn_ensemble.h"

namespace {

constexpr int TP = 64;                                              // tile of the transposing copy kernel: one 32-bit word per pixel
constexpr int TM = 32;                                              // tile of the transposing mean kernel: three words per pixel

__device__ __forceinline__ int reflect(int i, int n) { return i < n ? i : 2 * (n - 1) - i; }   // F.pad(mode='reflect'): no edge repeat

// one pixel of the source as three words, and the three floats of such words: uint8 HWC is divided by 255 (true division, as
// pre_u8_kernel's) after the tile, so that a pixel is one word in LDS; fp32 CHW is moved as it is
struct px3 {
    unsigned c[3];
};
__device__ __forceinline__ px3 load_px(const unsigned char* __restrict__ img, long b, int sy, int sx, int h, int w) {
    const unsigned char* p = img + ((b * h + sy) * w + sx) * 3;
    return px3{{p[0], p[1], p[2]}};
}
__device__ __forceinline__ px3 load_px(const float* __restrict__ x, long b, int sy, int sx, int h, int w) {
    const long hw = (long)h * w;
    const float* p = x + b * 3 * hw + (long)sy * w + sx;
    return px3{{__float_as_uint(p[0]), __float_as_uint(p[hw]), __float_as_uint(p[2 * hw])}};
}
template <typename T>
__device__ __forceinline__ float px_value(unsigned word) {
    if constexpr (sizeof(T) == 1) return (float)word / 255.0f;
    else return __uint_as_float(word);
}

template <typename T>
__device__ __forceinline__ void store_px(float* __restrict__ out, long copy, int y, int x, int H, int W, const px3& p, int swap_rb) {
    const long hw = (long)H * W;
    float* o = out + copy * 3 * hw + (long)y * W + x;
    const float c0 = px_value<T>(p.c[0]), c1 = px_value<T>(p.c[1]), c2 = px_value<T>(p.c[2]);
    o[0] = swap_rb ? c2 : c0;
    o[hw] = c1;
    o[2 * hw] = swap_rb ? c0 : c2;
}

// codes without a transposition: block (kk * nbx + i, y, b) owns pixels i * 256 .. of row y of copy kk; both sides run along rows
template <typename T>
__global__ __launch_bounds__(256) void d4_copy_kernel(const T* __restrict__ src, float* __restrict__ out, int h, int w, int H, int W,
                                                      int codes, int nbx, int swap_rb) {
    const int kk = blockIdx.x / nbx, x = (blockIdx.x - kk * nbx) * 256 + threadIdx.x, y = blockIdx.y, b = blockIdx.z;
    if (x >= W) return;
    const int k = (codes >> (3 * kk)) & 7;
    const int u = reflect(y, h), v = reflect(x, w);
    const px3 p = load_px(src, b, k & 2 ? h - 1 - u : u, k & 1 ? w - 1 - v : v, h, w);
    store_px<T>(out, (long)kk * gridDim.z + b, y, x, H, W, p, swap_rb);
}

// The source indices that the outputs i0 .. i1 of one axis (reflected within n) read: a run lo .. hi of at most i1 - i0 + 1 indices,
// whether the outputs lie inside n, in the padding (a descending run) or across the edge (the reflected part folds back over the rest).
__device__ __forceinline__ void reflected_run(int i0, int i1, int n, int& lo, int& hi) {
    const int a = reflect(i0, n), b = reflect(i1, n);
    lo = min(a, b);
    hi = (i0 < n && i1 >= n) ? n - 1 : max(a, b);
}

// codes with a transposition: block (kk * ntx + i, j, b) owns the TP x TP output tile (j, i) of copy kk.  Output (y, x) reads the
// mirrored source at (row u, column v) = (reflect(x), reflect(y)): the tile's rows u come from its x range and its columns v from its y
// range, both runs of at most TP (reflected_run).  Phase 1 walks those source rows along v (coalesced; a mirror only turns the
// direction) into tile[u][v]; phase 2 walks the output rows along x and reads tile[u(x)][v(y)] - down a column of the tile, which the
// pitch TP + 1 spreads over all banks.
template <typename T>
__global__ __launch_bounds__(256) void d4_copy_tr_kernel(const T* __restrict__ src, float* __restrict__ out, int h, int w, int H, int W,
                                                         int codes, int ntx, int swap_rb) {
    constexpr int NW = sizeof(T) == 1 ? 1 : 3;                      // words per pixel in LDS: a uint8 pixel packs into one
    __shared__ unsigned tile[NW][TP][TP + 1];
    const int kk = blockIdx.x / ntx, x0 = (blockIdx.x - kk * ntx) * TP, y0 = blockIdx.y * TP, b = blockIdx.z;
    const int k = (codes >> (3 * kk)) & 7;
    int ulo, uhi, vlo, vhi;
    reflected_run(x0, min(x0 + TP, W) - 1, h, ulo, uhi);            // h' x w' = w x h: x runs over the source's rows
    reflected_run(y0, min(y0 + TP, H) - 1, w, vlo, vhi);
    const int nu = uhi - ulo + 1, nv = vhi - vlo + 1;
    for (int i = threadIdx.x; i < TP * TP; i += 256) {
        const int du = i / TP, dv = i % TP;
        if (du < nu && dv < nv) {
            const int u = ulo + du, v = vlo + dv;
            const px3 p = load_px(src, b, k & 2 ? h - 1 - u : u, k & 1 ? w - 1 - v : v, h, w);
            if constexpr (NW == 1) {
                tile[0][du][dv] = p.c[0] | (p.c[1] << 8) | (p.c[2] << 16);
            } else {
#pragma unroll
                for (int c = 0; c < 3; ++c) tile[c][du][dv] = p.c[c];
            }
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < TP * TP; i += 256) {
        const int y = y0 + i / TP, x = x0 + i % TP;
        if (y < H && x < W) {
            const int du = reflect(x, h) - ulo, dv = reflect(y, w) - vlo;
            px3 p;
            if constexpr (NW == 1) {
                const unsigned q = tile[0][du][dv];
                p = px3{{q & 0xFFu, (q >> 8) & 0xFFu, q >> 16}};
            } else {
#pragma unroll
                for (int c = 0; c < 3; ++c) p.c[c] = tile[c][du][dv];
            }
            store_px<T>(out, (long)kk * gridDim.z + b, y, x, H, W, p, swap_rb);
        }
    }
}

// ---- the way back -----------------------------------------------------------------------------------------------------------------
struct mean_args {
    const float* res_a;
    const float* res_b;
    int B, h, w, Ha, Wa, Hb, Wb, codes_a, Ka, codes_b, Kb;
};

// The end of both mean kernels for one pixel: the division by K, then either the three plane stores or post_u8_kernel's clamp, scale,
// rounding and channel order.  Contraction is off in the accumulation and here, so every add and the division round once in both forms.
template <bool U8>
__device__ __forceinline__ void mean_finish(const float (&acc)[3], float K, void* __restrict__ out, long b, int y, int x, int h, int w,
                                            int swap_rb) {
#pragma clang fp contract(off)
    if constexpr (U8) {
        unsigned char v[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float f = acc[c] / K;
            f = f < 0.f ? 0.f : (f > 1.f ? 1.f : f);                // clamp_(0, 1)
            v[c] = (unsigned char)rintf(f * 255.0f);                // numpy .round(): half to even
        }
        unsigned char* o = static_cast<unsigned char*>(out) + ((b * h + y) * w + x) * 3;
        o[0] = swap_rb ? v[2] : v[0];
        o[1] = v[1];
        o[2] = swap_rb ? v[0] : v[2];
    } else {
        const long hw = (long)h * w;
        float* o = static_cast<float*>(out) + b * 3 * hw + (long)y * w + x;
#pragma unroll
        for (int c = 0; c < 3; ++c) o[c * hw] = acc[c] / K;
    }
}

// the terms of the codes without a transposition for output pixel (y, x): read along rows straight from res_a, in ascending k
__device__ __forceinline__ void mean_rows(const mean_args& a, long b, int y, int x, float (&acc)[3]) {
#pragma clang fp contract(off)
    const long plane = (long)a.Ha * a.Wa;
    for (int kk = 0; kk < a.Ka; ++kk) {
        const int k = (a.codes_a >> (3 * kk)) & 7;
        const float* p = a.res_a + ((long)kk * a.B + b) * 3 * plane + (long)(k & 2 ? a.h - 1 - y : y) * a.Wa + (k & 1 ? a.w - 1 - x : x);
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[c] = kk == 0 ? p[c * plane] : acc[c] + p[c * plane];
    }
}

// Block (i, j, b) owns the TM x TM tile (j, i) of frame b's output; thread t its pixels (t / TM + 8 r, t % TM), r = 0 .. 3, with three
// channels each.  The codes of res_a are summed first (mean_rows), then those of res_b one at a time through LDS: output (y, x) takes
// res_b at (row v, column u) with u = mirror(y), v = mirror(x), so the tile's rows v come from its x range and its columns u from its y
// range; phase 1 walks res_b's rows along u (coalesced) into tile[v][u], phase 2 reads tile[v(x)][u(y)] with x along the lanes - down a
// column of the tile, pitch TM + 1.
template <bool U8>
__global__ __launch_bounds__(256) void d4_mean_kernel(mean_args a, void* __restrict__ out, int swap_rb) {
#pragma clang fp contract(off)
    __shared__ float tile[3][TM][TM + 1];
    const int x0 = blockIdx.x * TM, y0 = blockIdx.y * TM, dx = threadIdx.x % TM, dy0 = threadIdx.x / TM;
    const long b = blockIdx.z;
    const int x = x0 + dx, nx = min(TM, a.w - x0), ny = min(TM, a.h - y0);
    float acc[TM / 8][3];
#pragma unroll
    for (int r = 0; r < TM / 8; ++r) {
        const int y = y0 + dy0 + 8 * r;
        if (x < a.w && y < a.h) mean_rows(a, b, y, x, acc[r]);
    }
    const long plane = (long)a.Hb * a.Wb;
    for (int kk = 0; kk < a.Kb; ++kk) {
        const int k = (a.codes_b >> (3 * kk)) & 7;
        const int ulo = k & 2 ? a.h - y0 - ny : y0, vlo = k & 1 ? a.w - x0 - nx : x0;   // a mirrored run is a run again
        const float* res = a.res_b + ((long)kk * a.B + b) * 3 * plane;
        if (kk) __syncthreads();                                    // the tile of the code before has been read
#pragma unroll
        for (int r = 0; r < TM / 8; ++r) {
            const int dv = dy0 + 8 * r, du = dx;
            if (dv < nx && du < ny) {
                const float* p = res + (long)(vlo + dv) * a.Wb + ulo + du;
#pragma unroll
                for (int c = 0; c < 3; ++c) tile[c][dv][du] = p[c * plane];
            }
        }
        __syncthreads();
        const bool first = a.Ka == 0 && kk == 0;
#pragma unroll
        for (int r = 0; r < TM / 8; ++r) {
            const int y = y0 + dy0 + 8 * r;
            if (x < a.w && y < a.h) {
                const int du = (k & 2 ? a.h - 1 - y : y) - ulo, dv = (k & 1 ? a.w - 1 - x : x) - vlo;
#pragma unroll
                for (int c = 0; c < 3; ++c) acc[r][c] = first ? tile[c][dv][du] : acc[r][c] + tile[c][dv][du];
            }
        }
    }
    const float K = (float)(a.Ka + a.Kb);
#pragma unroll
    for (int r = 0; r < TM / 8; ++r) {
        const int y = y0 + dy0 + 8 * r;
        if (x < a.w && y < a.h) mean_finish<U8>(acc[r], K, out, b, y, x, a.h, a.w, swap_rb);
    }
}

// the codes of the set bits of m, ascending, three bits each -> (codes, count)
inline int pack_codes(int m, int* count) {
    int codes = 0, n = 0;
    for (int k = 0; k < 8; ++k)
        if (m >> k & 1) codes |= k << (3 * n++);
    *count = n;
    return codes;
}

template <typename T>
int d4_copy(const T* src, float* out, int B, int h, int w, int H, int W, int mask, int swap_rb, fdn_stream_t stream) {
    FDN_CHECK_ARG(src && out && B > 0 && B < 65536 && h > 0 && w > 0 && mask >= 1 && mask <= 255);
    FDN_CHECK_ARG(!(mask & 0x0F) || !(mask & 0xF0));                // one call makes one output shape
    const bool tr = mask & 0xF0;
    const int hp = tr ? w : h, wp = tr ? h : w;
    FDN_CHECK_ARG(H >= hp && W >= wp && H < 65536);
    FDN_CHECK_ARG(H - hp < hp && W - wp < wp);                      // reflect padding needs pad < size
    int K;
    const int codes = pack_codes(mask, &K);
    if (tr) {
        const int ntx = cdiv(W, TP);
        hipLaunchKernelGGL(d4_copy_tr_kernel<T>, dim3(K * ntx, cdiv(H, TP), B), dim3(256), 0, static_cast<hipStream_t>(stream), src, out, h,
                           w, H, W, codes, ntx, swap_rb);
    } else {
        const int nbx = cdiv(W, 256);
        hipLaunchKernelGGL(d4_copy_kernel<T>, dim3(K * nbx, H, B), dim3(256), 0, static_cast<hipStream_t>(stream), src, out, h, w, H, W,
                           codes, nbx, swap_rb);
    }
    return fdn_launch_status();
}

template <bool U8>
int d4_mean(const float* res_a, const float* res_b, void* out, int B, int h, int w, int Ha, int Wa, int Hb, int Wb, int mask, int swap_rb,
            fdn_stream_t stream) {
    FDN_CHECK_ARG(out && B > 0 && B < 65536 && h > 0 && w > 0 && h < 65536 && mask >= 1 && mask <= 255);
    FDN_CHECK_ARG(!res_a == !(mask & 0x0F) && !res_b == !(mask & 0xF0));
    FDN_CHECK_ARG(!res_a || (Ha >= h && Wa >= w));
    FDN_CHECK_ARG(!res_b || (Hb >= w && Wb >= h));
    mean_args a{res_a, res_b, B, h, w, Ha, Wa, Hb, Wb, 0, 0, 0, 0};
    a.codes_a = pack_codes(mask & 0x0F, &a.Ka);
    a.codes_b = pack_codes(mask >> 4, &a.Kb);                       // bits 1 and 2 of a code are all the kernel reads
    hipLaunchKernelGGL(d4_mean_kernel<U8>, dim3(cdiv(w, TM), cdiv(h, TM), B), dim3(256), 0, static_cast<hipStream_t>(stream), a, out,
                       swap_rb);
    return fdn_launch_status();
}

}  // namespace

extern "C" int fdn_ensemble_abi_version(void) { return FDN_ENSEMBLE_ABI_VERSION; }

extern "C" int fdn_d4_pre_u8(const unsigned char* img, float* out, int B, int h, int w, int H, int W, int mask, int swap_rb,
                             fdn_stream_t stream) {
    return d4_copy(img, out, B, h, w, H, W, mask, swap_rb, stream);
}

extern "C" int fdn_d4_apply(const float* x, float* out, int N, int h, int w, int H, int W, int mask, fdn_stream_t stream) {
    return d4_copy(x, out, N, h, w, H, W, mask, 0, stream);
}

extern "C" int fdn_d4_mean(const float* res_a, const float* res_b, float* out, int B, int h, int w, int Ha, int Wa, int Hb, int Wb,
                           int mask, fdn_stream_t stream) {
    return d4_mean<false>(res_a, res_b, out, B, h, w, Ha, Wa, Hb, Wb, mask, 0, stream);
}

extern "C" int fdn_d4_post_u8(const float* res_a, const float* res_b, unsigned char* out, int B, int h, int w, int Ha, int Wa, int Hb,
                              int Wb, int mask, int swap_rb, fdn_stream_t stream) {
    return d4_mean<true>(res_a, res_b, out, B, h, w, Ha, Wa, Hb, Wb, mask, swap_rb, stream);
}
