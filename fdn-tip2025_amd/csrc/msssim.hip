// Multi-scale SSIM of batches of 8-bit image pairs and of video luma planes (include/fdn_msssim.h, ABI 1; linked into libfdn_msssim.so,
// beside libfdn_hip.so).  The header has the definitions.
//   pyramid_kernel : one thread per sample of level s + 1, the integer sum of the 2 x 2 block of level s with the last row / column taken
//                    twice where the size is odd.  Level 0 is never materialised: where s = 0 the block is formed from the bytes or codes
//                    (the channel, the gray sum, the 10-bit clamp), as the window kernel forms its tile.
//   window_kernel  : one 16 x 32 tile of map positions per workgroup.  The tile of A and B with its 10-sample apron sits in LDS as int32
//                    (2 x 26 x 42 words), the row pass of the five moments goes into LDS as doubles (5 x 26 x 32), the column pass out of
//                    it, then cs, l, ss, the optional maps and the tile's two partial sums.
//   fold_kernel    : one workgroup per plane and level adds the tiles' partial sums in a fixed order.
// Batch, planes and both images ride in the grid: one call is four pyramid launches, five window launches and one fold.  No atomics: a
// tile's sums are fixed trees over its 256 threads, a plane's sums a fixed walk over its tiles.  Every moment is defined with one rounding
// per operation, so contraction into FMAs is off in this file.
#include "common.hpp"

#include "../../include/fdn_msssim.h"

#pragma clang fp contract(off)

namespace {

constexpr int NL = FDN_MSSSIM_LEVELS, MIN_SIDE = FDN_MSSSIM_MIN_SIDE;
constexpr int TH = FDN_MSSSIM_TILE_H, TW = FDN_MSSSIM_TILE_W, AP = 10, AH = TH + AP, AW = TW + AP, AW_LD = AW + 1;
static_assert(TW == 32 && TH * TW == 2 * 256, "two map positions per thread, a row of the tile per 32 threads");
static_assert(2 * AH * AW_LD * 4 + 5 * AH * TW * 8 + 256 * 8 <= 64 * 1024, "static LDS of the window kernel");

enum { K_CH = 0, K_GRAY = 1, K_Y8 = 2, K_Y10 = 3, K_I32 = 4 };   // where the samples of a level come from

struct G11 { double w[11]; };

// the two sources of a level: bytes / codes for level 0, an int32 level [P][h][w] for the others
struct Src {
    const void* p[2];
    int kind;
    int bgr;       // K_CH, K_GRAY: the bytes of a pixel are B, G, R
    long stride;   // K_Y8, K_Y10: samples between frames
};

struct Fold {
    long off[NL];   // where the level's partials start in the workspace, in doubles
    int tiles[NL];
};

// sample (y, x) of plane `plane` of an h x w level; y < h and x < w
__device__ __forceinline__ int sample(const Src& s, int which, long plane, int y, int x, int h, int w) {
    const void* base = s.p[which];
    switch (s.kind) {
    case K_CH: {
        const long image = plane / 3;
        const int k = (int)(plane - 3 * image);
        return static_cast<const unsigned char*>(base)[((image * h + y) * (long)w + x) * 3 + (s.bgr ? 2 - k : k)];
    }
    case K_GRAY: {
        const unsigned char* p = static_cast<const unsigned char*>(base) + ((plane * h + y) * (long)w + x) * 3;
        return 299 * p[s.bgr ? 2 : 0] + 587 * p[1] + 114 * p[s.bgr ? 0 : 2];
    }
    case K_Y8:
        return static_cast<const unsigned char*>(base)[plane * s.stride + (long)y * w + x];
    case K_Y10: {
        const int v = static_cast<const unsigned short*>(base)[plane * s.stride + (long)y * w + x];
        return v > 1023 ? 1023 : v;
    }
    default:
        return static_cast<const int*>(base)[(plane * h + y) * (long)w + x];
    }
}

// the sum of v over the workgroup's 256 threads, the same tree on every call
__device__ __forceinline__ double block_sum(double v, double* red, int tid) {
    red[tid] = v;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if (tid < st) red[tid] += red[tid + st];
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
}

// grid 2 * P * blocks, blocks = cdiv(hn * wn, 256): dst[which] [P][hn][wn] = the 2 x 2 block sums of the h x w level `src`
__global__ __launch_bounds__(256) void pyramid_kernel(Src src, long P, int h, int w, int hn, int wn, int blocks, int* __restrict__ dst_a,
                                                      int* __restrict__ dst_b) {
    const long pw = blockIdx.x / blocks;                          // which * P + plane
    const int which = (int)(pw / P);
    const long plane = pw - which * P;
    const long at = (long)(blockIdx.x - pw * blocks) * 256 + threadIdx.x;
    if (at >= (long)hn * wn) return;
    const int i = (int)(at / wn), j = (int)(at - (long)i * wn);
    const int y0 = 2 * i, y1 = 2 * i + 1 < h ? 2 * i + 1 : h - 1, x0 = 2 * j, x1 = 2 * j + 1 < w ? 2 * j + 1 : w - 1;
    const int v = sample(src, which, plane, y0, x0, h, w) + sample(src, which, plane, y0, x1, h, w) + sample(src, which, plane, y1, x0, h, w) +
                  sample(src, which, plane, y1, x1, h, w);
    (which ? dst_b : dst_a)[plane * hn * (long)wn + at] = v;
}

// grid P * tiles; part [plane][tile][2] = the tile's sums of cs and of ss; cs_map, ss_map: NULL or [P][mh][mw] of this level
__global__ __launch_bounds__(256) void window_kernel(Src src, G11 g, int h, int w, int tiles_x, int tiles, double c1, double c2,
                                                     double* __restrict__ cs_map, double* __restrict__ ss_map, double* __restrict__ part) {
    __shared__ int smp[2][AH][AW_LD];
    __shared__ double row[5][AH][TW];
    __shared__ double red[256];
    const int tid = threadIdx.x;
    const long plane = blockIdx.x / tiles;
    const int tile = (int)(blockIdx.x - plane * tiles);
    const int y0 = (tile / tiles_x) * TH, x0 = (tile % tiles_x) * TW;
    const int mh = h - AP, mw = w - AP;
    for (int i = tid; i < 2 * AH * AW; i += 256) {
        const int which = i / (AH * AW), rem = i - which * (AH * AW);
        const int r = rem / AW, c = rem - r * AW;
        const int y = y0 + r, x = x0 + c;
        smp[which][r][c] = y < h && x < w ? sample(src, which, plane, y, x, h, w) : 0;     // outside the level: met by no map position
    }
    __syncthreads();
    for (int i = tid; i < AH * TW; i += 256) {
        const int r = i / TW, c = i - r * TW;
        double ra = 0.0, rb = 0.0, raa = 0.0, rbb = 0.0, rab = 0.0;
#pragma unroll
        for (int t = 0; t < 11; ++t) {
            const double a = (double)smp[0][r][c + t], b = (double)smp[1][r][c + t];
            ra = ra + g.w[t] * a;
            rb = rb + g.w[t] * b;
            raa = raa + g.w[t] * (a * a);
            rbb = rbb + g.w[t] * (b * b);
            rab = rab + g.w[t] * (a * b);
        }
        row[0][r][c] = ra;
        row[1][r][c] = rb;
        row[2][r][c] = raa;
        row[3][r][c] = rbb;
        row[4][r][c] = rab;
    }
    __syncthreads();
    const int px = tid & (TW - 1), py = tid / TW;
    double sum_cs = 0.0, sum_ss = 0.0;
#pragma unroll 1
    for (int j = 0; j < 2; ++j) {
        const int r = py + j * (TH / 2);
        const int y = y0 + r, x = x0 + px;
        if (y >= mh || x >= mw) continue;
        double m[5];
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            double v = 0.0;
#pragma unroll
            for (int t = 0; t < 11; ++t) v = v + g.w[t] * row[k][r + t][px];
            m[k] = v;
        }
        const double va = m[2] - m[0] * m[0], vb = m[3] - m[1] * m[1], vab = m[4] - m[0] * m[1];
        const double cs = (2.0 * vab + c2) / (va + vb + c2);
        const double l = (2.0 * (m[0] * m[1]) + c1) / (m[0] * m[0] + m[1] * m[1] + c1);
        const double ss = l * cs;
        const long at = (plane * mh + y) * (long)mw + x;
        if (cs_map) cs_map[at] = cs;
        if (ss_map) ss_map[at] = ss;
        sum_cs += cs;
        sum_ss += ss;
    }
    const double t0 = block_sum(sum_cs, red, tid), t1 = block_sum(sum_ss, red, tid);
    if (tid == 0) {
        part[2 * (long)blockIdx.x] = t0;
        part[2 * (long)blockIdx.x + 1] = t1;
    }
}

// grid P * 5: out [plane][level][2] = the sums of the level's part [plane][tile][2] over the tiles, thread t walking tiles t, t + 256, ...
// in order, then the tree
__global__ __launch_bounds__(256) void fold_kernel(const double* __restrict__ ws, Fold f, double* __restrict__ out) {
    __shared__ double red[256];
    const int tid = threadIdx.x;
    const long plane = blockIdx.x / NL;
    const int level = (int)(blockIdx.x - plane * NL);
    const int tiles = f.tiles[level];
    const double* p = ws + f.off[level] + 2 * plane * tiles;
#pragma unroll 1
    for (int v = 0; v < 2; ++v) {
        double sum = 0.0;
        for (int t = tid; t < tiles; t += 256) sum += p[2 * (long)t + v];
        const double total = block_sum(sum, red, tid);
        if (tid == 0) out[2 * (long)blockIdx.x + v] = total;
    }
}

bool aligned8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7u) == 0; }
bool size_ok(int B, int planes, int h, int w) {
    return B >= 1 && (planes == 1 || planes == 3) && h >= MIN_SIDE && w >= MIN_SIDE && (long)h * w <= 0x7FFFFFFFL;
}

struct Dims {
    int lh[NL], lw[NL];
    long n[NL];       // samples of a level of one plane
    long tiles[NL];   // tiles of a level's map
    long part_off[NL], parts;   // doubles: where a level's partials start, and all of them
    long pyr_off[NL], pyr;      // int32 words: where level s >= 1 starts in a pyramid of P planes, and the whole pyramid
    long map_off[NL];           // doubles: where level s starts in a map output of P planes
};

Dims dims_of(long P, int h, int w) {
    Dims d;
    d.parts = d.pyr = 0;
    long maps = 0;
    for (int s = 0; s < NL; ++s) {
        d.lh[s] = s ? (d.lh[s - 1] + 1) / 2 : h;
        d.lw[s] = s ? (d.lw[s - 1] + 1) / 2 : w;
        d.n[s] = (long)d.lh[s] * d.lw[s];
        d.tiles[s] = (long)cdiv(d.lh[s] - AP, TH) * cdiv(d.lw[s] - AP, TW);
        d.part_off[s] = d.parts;
        d.parts += 2 * P * d.tiles[s];
        d.pyr_off[s] = d.pyr;
        if (s) d.pyr += P * d.n[s];
        d.map_off[s] = maps;
        maps += P * (long)(d.lh[s] - AP) * (d.lw[s] - AP);
    }
    return d;
}

// the launches of one call; level 0 comes from `src0`, a pyramid the caller does not want lives behind the partials in ws
int score(Src src0, long P, int h, int w, double q0, double L, const double* taps11, int* pyr_a, int* pyr_b, double* cs_map, double* ss_map,
          double* ws, double* out, fdn_stream_t stream) {
    const Dims d = dims_of(P, h, w);
    for (int s = 0; s < NL; ++s) {
        if (P * d.tiles[s] > 0x7FFFFFFFL) return FDN_ERR_UNSUPPORTED;
        if (s && 2 * P * (long)cdiv(d.n[s], 256) > 0x7FFFFFFFL) return FDN_ERR_UNSUPPORTED;
    }
    if (P * NL > 0x7FFFFFFFL) return FDN_ERR_UNSUPPORTED;
    G11 g;
    for (int i = 0; i < 11; ++i) g.w[i] = taps11[i];
    int* own = reinterpret_cast<int*>(ws + d.parts);
    int* pa = pyr_a ? pyr_a : own;
    int* pb = pyr_b ? pyr_b : own + d.pyr;
    hipStream_t st = static_cast<hipStream_t>(stream);
    Src src = src0;
    Fold f;
    double q = q0;
    const double k1 = 0.01 * L, k2 = 0.03 * L;
    for (int s = 0; s < NL; ++s) {
        if (s) {
            const int blocks = cdiv(d.n[s], 256);
            hipLaunchKernelGGL(pyramid_kernel, dim3((unsigned)(2 * P * blocks)), dim3(256), 0, st, src, P, d.lh[s - 1], d.lw[s - 1], d.lh[s], d.lw[s],
                               blocks, pa + d.pyr_off[s], pb + d.pyr_off[s]);
            src.p[0] = pa + d.pyr_off[s];
            src.p[1] = pb + d.pyr_off[s];
            src.kind = K_I32;
            q = q * 4.0;
        }
        const double c1 = k1 * k1 * q * q, c2 = k2 * k2 * q * q;
        hipLaunchKernelGGL(window_kernel, dim3((unsigned)(P * d.tiles[s])), dim3(256), 0, st, src, g, d.lh[s], d.lw[s], cdiv(d.lw[s] - AP, TW),
                           (int)d.tiles[s], c1, c2, cs_map ? cs_map + d.map_off[s] : nullptr, ss_map ? ss_map + d.map_off[s] : nullptr,
                           ws + d.part_off[s]);
        f.off[s] = d.part_off[s];
        f.tiles[s] = (int)d.tiles[s];
    }
    hipLaunchKernelGGL(fold_kernel, dim3((unsigned)(P * NL)), dim3(256), 0, st, (const double*)ws, f, out);
    return fdn_launch_status();
}

}  // namespace

extern "C" int fdn_msssim_abi_version(void) { return FDN_MSSSIM_ABI_VERSION; }

extern "C" int fdn_msssim_dims(int h, int w, int* lh, int* lw, int* mh, int* mw) {
    FDN_CHECK_ARG(lh && lw && mh && mw && size_ok(1, 1, h, w));
    const Dims d = dims_of(1, h, w);
    for (int s = 0; s < NL; ++s) {
        lh[s] = d.lh[s];
        lw[s] = d.lw[s];
        mh[s] = d.lh[s] - AP;
        mw[s] = d.lw[s] - AP;
    }
    return FDN_OK;
}

extern "C" long fdn_msssim_ws(int B, int planes, int h, int w) {
    if (!size_ok(B, planes, h, w)) return 0;
    const Dims d = dims_of((long)B * planes, h, w);
    return d.parts + (2 * d.pyr + 1) / 2;                         // two int32 pyramids in doubles
}

extern "C" int fdn_msssim_u8(const unsigned char* a, const unsigned char* b, int B, int h, int w, int mode, int bgr, const double* taps11,
                             int* pyr_a, int* pyr_b, double* cs_map, double* ss_map, double* ws, double* out, fdn_stream_t stream) {
    FDN_CHECK_ARG(a && b && taps11 && ws && out && aligned8(ws) && (mode == FDN_MSSSIM_RGB || mode == FDN_MSSSIM_GRAY) && size_ok(B, 1, h, w));
    const bool rgb = mode == FDN_MSSSIM_RGB;
    Src src;
    src.p[0] = a;
    src.p[1] = b;
    src.kind = rgb ? K_CH : K_GRAY;
    src.bgr = bgr != 0 ? 1 : 0;
    src.stride = 0;
    return score(src, (long)B * (rgb ? 3 : 1), h, w, rgb ? 1.0 : 1000.0, 255.0, taps11, pyr_a, pyr_b, cs_map, ss_map, ws, out, stream);
}

extern "C" int fdn_msssim_luma(const void* a, const void* b, int B, int h, int w, int bits, long stride, const double* taps11, int* pyr_a,
                               int* pyr_b, double* cs_map, double* ss_map, double* ws, double* out, fdn_stream_t stream) {
    FDN_CHECK_ARG(a && b && taps11 && ws && out && aligned8(ws) && (bits == 8 || bits == 10) && size_ok(B, 1, h, w) && stride >= (long)h * w);
    Src src;
    src.p[0] = a;
    src.p[1] = b;
    src.kind = bits == 8 ? K_Y8 : K_Y10;
    src.bgr = 0;
    src.stride = stride;
    return score(src, B, h, w, 1.0, bits == 8 ? 255.0 : 1023.0, taps11, pyr_a, pyr_b, cs_map, ss_map, ws, out, stream);
}
