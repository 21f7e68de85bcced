// PIQE, the no-reference block-wise image quality score, of batches of 8-bit images and of video luma planes (include/fdn_piqe.h, ABI 1;
// linked into libfdn_piqe.so, beside libfdn_hip.so).  The header has the definition, every order of summation included.
//   piqe_tile_kernel : one 32 x 64 tile (2 x 4 blocks of 16 x 16) per workgroup.  The tile's codes with their 3-sample apron sit in LDS as
//                      uint16 (38 x 70), formed from the bytes once (the gray code, the 10-bit clamp, the replicate padding); the row pass of
//                      I and I * I goes into LDS as doubles (2 x 38 x 64), the column pass out of it with a sliding window of 14 rows per
//                      thread, and the MSCN values take the row pass's place (32 rows of 65: a block's 16 rows fall on 16 bank pairs).
//                      The block statistics run on 16 lanes per block, lane r owning row r: waves 0 and 1 take the variance and the 44
//                      segment tests (three per lane, joined by a ballot), waves 2 and 3 the centre and the surround; the row sums cross
//                      lanes through LDS and every lane adds them top to bottom itself.  One partial {D, count} per tile.
//   piqe_fold_kernel : one workgroup per plane adds the tiles' partials in the header's order.
// The batch rides in the grid: one call is two launches.  No atomics.  Every value is defined with one rounding per operation, so
// contraction into FMAs is off in this file.
#include "common.hpp"

#include "../../include/fdn_piqe.h"

#pragma clang fp contract(off)

namespace {

constexpr int BS = FDN_PIQE_BLOCK, TH = FDN_PIQE_TILE_H, TW = FDN_PIQE_TILE_W, AP = 3, AH = TH + 2 * AP, AW = TW + 2 * AP, AW_LD = AW + 1;
constexpr int NLD = TW + 1;                  // leading dimension of the MSCN tile, in doubles
constexpr int NBX = TW / BS, NB = (TH / BS) * NBX, ROWS = TH / 4;
static_assert(BS == 16 && TW == 64 && TH == 32 && NB == 8, "8 blocks of 16 lanes for each half of the 256 threads; a row of the tile per wave");
static_assert(TH * NLD <= 2 * AH * TW, "the MSCN tile fits where the row pass was");
static_assert(AH * AW_LD * 2 + 2 * AH * TW * 8 + 4 * NB * 16 * 8 + 3 * NB * 8 <= 64 * 1024, "static LDS");

enum { K_GRAY = 0, K_Y8 = 1, K_Y10 = 2 };

struct G7 { double w[7]; };

struct Src {
    const void* p;
    int kind;
    int bgr;       // K_GRAY: the bytes of a pixel are B, G, R
    long stride;   // K_Y8, K_Y10: samples between frames
};

// code (y, x) of plane `plane`; 0 <= y < h and 0 <= x < w
__device__ __forceinline__ int sample(const Src& s, long plane, int y, int x, int h, int w) {
    switch (s.kind) {
    case K_GRAY: {
        const unsigned char* p = static_cast<const unsigned char*>(s.p) + ((plane * h + y) * (long)w + x) * 3;
        return (299 * p[s.bgr ? 2 : 0] + 587 * p[1] + 114 * p[s.bgr ? 0 : 2] + 500) / 1000;
    }
    case K_Y8:
        return static_cast<const unsigned char*>(s.p)[plane * s.stride + (long)y * w + x];
    default: {
        const int v = static_cast<const unsigned short*>(s.p)[plane * s.stride + (long)y * w + x];
        return v > 1023 ? 1023 : v;
    }
    }
}

__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : v > hi ? hi : v; }

// grid P * tiles; part [plane][tile][2] = {the tile's sum of d, its number of active blocks}; mscn, var, cls: NULL or as the header lays them
__global__ __launch_bounds__(256) void piqe_tile_kernel(Src src, G7 g, double rq, int h, int w, int H, int W, int tiles_x, int tiles,
                                                        double* __restrict__ mscn, double* __restrict__ var, unsigned char* __restrict__ cls,
                                                        double* __restrict__ part) {
    __shared__ unsigned short smp[AH][AW_LD];   // codes are at most 1023
    __shared__ double buf[2 * AH * TW];       // the row pass of I and of I * I as [2][AH][TW]; then the MSCN tile as [TH][NLD]
    __shared__ double ex[2][2][NB][16];       // [waves 0, 1 | waves 2, 3][sums | squared deviations][block][row]
    __shared__ double csd_s[NB], d_s[NB];
    __shared__ int act_s[NB];
    const int tid = threadIdx.x;
    const long plane = blockIdx.x / tiles;
    const int tile = (int)(blockIdx.x - plane * tiles);
    const int y0 = (tile / tiles_x) * TH, x0 = (tile % tiles_x) * TW;

    for (int i = tid; i < AH * AW; i += 256) {
        const int r = i / AW, c = i - r * AW;
        smp[r][c] = (unsigned short)sample(src, plane, clampi(y0 - AP + r, h - 1), clampi(x0 - AP + c, w - 1), h, w);
    }
    __syncthreads();

    for (int i = tid; i < AH * TW; i += 256) {
        const int r = i / TW, c = i - r * TW;
        double r0 = 0.0, r1 = 0.0;
#pragma unroll
        for (int t = 0; t < 7; ++t) {
            const double x = (double)smp[r][c + t] * rq;                             // rq = 1 / q, a power of two: exact, as the division is
            r0 = r0 + g.w[t] * x;
            r1 = r1 + g.w[t] * (x * x);
        }
        buf[r * TW + c] = r0;
        buf[AH * TW + r * TW + c] = r1;
    }
    __syncthreads();

    {
        const int px = tid & (TW - 1), r0 = (tid / TW) * ROWS;                         // ROWS rows of one column per thread
        double a0[ROWS + 2 * AP], a1[ROWS + 2 * AP], n[ROWS];
#pragma unroll
        for (int k = 0; k < ROWS + 2 * AP; ++k) {
            a0[k] = buf[(r0 + k) * TW + px];
            a1[k] = buf[AH * TW + (r0 + k) * TW + px];
        }
#pragma unroll
        for (int j = 0; j < ROWS; ++j) {
            double mu = 0.0, m2 = 0.0;
#pragma unroll
            for (int t = 0; t < 7; ++t) {
                mu = mu + g.w[t] * a0[j + t];
                m2 = m2 + g.w[t] * a1[j + t];
            }
            const double x = (double)smp[r0 + j + AP][px + AP] * rq;
            const double sd = sqrt(fabs(m2 - mu * mu));
            n[j] = (x - mu) / (sd + 1.0);
            const int y = y0 + r0 + j, xx = x0 + px;
            if (mscn && y < H && xx < W) mscn[(plane * H + y) * (long)W + xx] = n[j];
        }
        __syncthreads();                                                               // every thread has read its part of the row pass
#pragma unroll
        for (int j = 0; j < ROWS; ++j) buf[(r0 + j) * NLD + px] = n[j];
    }
    __syncthreads();

    const int k = (tid >> 4) & (NB - 1), r = tid & 15, grp = tid >> 7;                // block of the tile, row of the block, which half
    const int bty = k / NBX, btx = k - bty * NBX;
    const double* b = buf + bty * BS * NLD + btx * BS;                                 // b[i * NLD + j]
    double x[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) x[j] = b[r * NLD + j];
    {
        double s = 0.0;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            if (grp && (j == 7 || j == 8)) continue;
            s = s + x[j];
        }
        ex[grp][0][k][r] = s;
    }
    __syncthreads();

    double cstd = 0.0;
    bool low = false;
    {
        double tot = 0.0;
#pragma unroll
        for (int i = 0; i < 16; ++i) tot = tot + ex[grp][0][k][i];
        const double mean = tot / (grp ? 224.0 : 256.0);
        double s = 0.0;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            if (grp && (j == 7 || j == 8)) continue;
            const double dv = x[j] - mean;
            s = s + dv * dv;
        }
        ex[grp][1][k][r] = s;
    }
    if (grp) {                                                                         // wave-uniform: the centre, by every lane alike
        double cs = 0.0;
#pragma unroll 1
        for (int c = 7; c < 9; ++c)
#pragma unroll
            for (int i = 0; i < 16; ++i) cs = cs + b[i * NLD + c];
        const double cm = cs / 32.0;
        double cd = 0.0;
#pragma unroll 1
        for (int c = 7; c < 9; ++c)
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const double dv = b[i * NLD + c] - cm;
                cd = cd + dv * dv;
            }
        cstd = sqrt(cd / 31.0);
    } else {                                                                           // the 44 segments: lane r takes r, r + 16, r + 32
#pragma unroll 1
        for (int sid = r; sid < 44; sid += 16) {
            const int e = sid / 11, s = sid - e * 11;
            const int at = e == 0 ? s : e == 1 ? s * NLD + 15 : e == 2 ? 15 * NLD + s : s * NLD, step = (e & 1) ? NLD : 1;
            double v[6], sum = 0.0;
#pragma unroll
            for (int i = 0; i < 6; ++i) {
                v[i] = b[at + i * step];
                sum = sum + v[i];
            }
            const double mean = sum / 6.0;
            double dev = 0.0;
#pragma unroll
            for (int i = 0; i < 6; ++i) {
                const double dv = v[i] - mean;
                dev = dev + dv * dv;
            }
            low = low || sqrt(dev / 5.0) < 0.1;
        }
    }
    const unsigned long long lows = __ballot(low);                                     // all 64 lanes of every wave are here
    const bool wndc = ((lows >> (tid & 48)) & 0xFFFFull) != 0;
    __syncthreads();

    double v = 0.0;
    {
        double tot = 0.0;
#pragma unroll
        for (int i = 0; i < 16; ++i) tot = tot + ex[grp][1][k][i];
        if (grp) {
            double csd = cstd / sqrt(tot / 223.0);
            if (csd != csd) csd = 0.0;
            if (r == 0) csd_s[k] = csd;
        } else {
            v = tot / 255.0;
        }
    }
    __syncthreads();

    if (!grp && r == 0) {
        const int by = y0 / BS + bty, bx = x0 / BS + btx, nby = H / BS, nbx = W / BS;
        const bool inside = by < nby && bx < nbx, active = v > 0.1;
        const double sigma = sqrt(v), csd = csd_s[k];
        const double beta = fabs(sigma - csd) / fmax(sigma, csd);
        const bool wnc = sigma > 2.0 * beta;
        const double d = (wndc ? 1.0 - v : 0.0) + (wnc ? v : 0.0);
        if (inside) {
            const long at = (plane * nby + by) * (long)nbx + bx;
            if (var) var[at] = v;
            if (cls) cls[at] = active ? (unsigned char)(FDN_PIQE_ACTIVE | (wndc ? FDN_PIQE_WNDC : 0) | (wnc ? FDN_PIQE_WNC : 0)) : (unsigned char)0;
        }
        d_s[k] = d;
        act_s[k] = inside && active ? 1 : 0;
    }
    __syncthreads();
    if (tid == 0) {
        double D = 0.0;
        int cnt = 0;
#pragma unroll
        for (int i = 0; i < NB; ++i)
            if (act_s[i]) {
                D = D + d_s[i];
                ++cnt;
            }
        part[2 * (long)blockIdx.x] = D;
        part[2 * (long)blockIdx.x + 1] = (double)cnt;
    }
}

// grid P: out [plane][2] = the sums of part [plane][tile][2] over the tiles, slot t walking tiles t, t + 256, ... in order, then the tree
__global__ __launch_bounds__(256) void piqe_fold_kernel(const double* __restrict__ ws, int tiles, double* __restrict__ out) {
    __shared__ double red[256];
    const int tid = threadIdx.x;
    const double* p = ws + 2 * (long)blockIdx.x * tiles;
#pragma unroll 1
    for (int v = 0; v < 2; ++v) {
        double sum = 0.0;
        for (int t = tid; t < tiles; t += 256) sum = sum + p[2 * (long)t + v];
        red[tid] = sum;
        __syncthreads();
        for (int st = 128; st > 0; st >>= 1) {
            if (tid < st) red[tid] = red[tid] + red[tid + st];
            __syncthreads();
        }
        if (tid == 0) out[2 * (long)blockIdx.x + v] = red[0];
        __syncthreads();
    }
}

bool aligned8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7u) == 0; }

struct Dims {
    long H, W, tiles_y, tiles_x;
};

Dims dims_of(int h, int w) {
    Dims d;
    d.H = ((long)h + BS - 1) / BS * BS;
    d.W = ((long)w + BS - 1) / BS * BS;
    d.tiles_y = (d.H + TH - 1) / TH;
    d.tiles_x = (d.W + TW - 1) / TW;
    return d;
}

bool size_ok(int B, int h, int w) {
    if (B < 1 || h < 1 || w < 1) return false;
    const Dims d = dims_of(h, w);
    return d.H * d.W <= 0x7FFFFFFFL;
}

int score(Src src, long P, int h, int w, double q, const double* taps7, double* mscn, double* var, unsigned char* cls, double* ws, double* out,
          fdn_stream_t stream) {
    const Dims d = dims_of(h, w);
    const long tiles = d.tiles_y * d.tiles_x;
    if (P * tiles * 256 > 0xFFFFFFFFL) return FDN_ERR_UNSUPPORTED;                  // HIP holds grid x block to 2^32 - 1 threads
    G7 g;
    for (int i = 0; i < 7; ++i) g.w[i] = taps7[i];
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(piqe_tile_kernel, dim3((unsigned)(P * tiles)), dim3(256), 0, st, src, g, 1.0 / q, h, w, (int)d.H, (int)d.W, (int)d.tiles_x,
                       (int)tiles, mscn, var, cls, ws);
    hipLaunchKernelGGL(piqe_fold_kernel, dim3((unsigned)P), dim3(256), 0, st, (const double*)ws, (int)tiles, out);
    return fdn_launch_status();
}

}  // namespace

extern "C" int fdn_piqe_abi_version(void) { return FDN_PIQE_ABI_VERSION; }

extern "C" int fdn_piqe_dims(int h, int w, int* dims) {
    FDN_CHECK_ARG(dims && size_ok(1, h, w));
    const Dims d = dims_of(h, w);
    dims[0] = (int)d.H;
    dims[1] = (int)d.W;
    dims[2] = (int)(d.H / BS);
    dims[3] = (int)(d.W / BS);
    dims[4] = (int)d.tiles_y;
    dims[5] = (int)d.tiles_x;
    return FDN_OK;
}

extern "C" long fdn_piqe_ws(int B, int h, int w) {
    if (!size_ok(B, h, w)) return 0;
    const Dims d = dims_of(h, w);
    return 2 * (long)B * d.tiles_y * d.tiles_x;
}

extern "C" int fdn_piqe_u8(const unsigned char* img, int B, int h, int w, int bgr, const double* taps7, double* mscn, double* var,
                           unsigned char* cls, double* ws, double* out, fdn_stream_t stream) {
    FDN_CHECK_ARG(img && taps7 && ws && out && aligned8(ws) && size_ok(B, h, w));
    Src src;
    src.p = img;
    src.kind = K_GRAY;
    src.bgr = bgr != 0 ? 1 : 0;
    src.stride = 0;
    return score(src, B, h, w, 1.0, taps7, mscn, var, cls, ws, out, stream);
}

extern "C" int fdn_piqe_luma(const void* frames, int B, int h, int w, int bits, long stride, const double* taps7, double* mscn, double* var,
                             unsigned char* cls, double* ws, double* out, fdn_stream_t stream) {
    FDN_CHECK_ARG(frames && taps7 && ws && out && aligned8(ws) && (bits == 8 || bits == 10) && size_ok(B, h, w) && stride >= (long)h * w);
    Src src;
    src.p = frames;
    src.kind = bits == 8 ? K_Y8 : K_Y10;
    src.bgr = 0;
    src.stride = stride;
    return score(src, B, h, w, bits == 8 ? 1.0 : 4.0, taps7, mscn, var, cls, ws, out, stream);
}
