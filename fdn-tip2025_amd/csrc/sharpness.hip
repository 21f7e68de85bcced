// Deblurring evaluation of batches of 8-bit image pairs (include/fdn_sharpness.h, ABI 1; linked into libfdn_sharpness.so, beside
// libfdn_hip.so).  The header has the definitions; a = ground truth, b = restored.
//   fdn_edge_u8 : edge_kernel, one 32 x 32 tile of pixels per workgroup.  The rows of the tile and its 4-pixel apron are staged in LDS as
//                 the aligned dwords that cover their interleaved bytes (a dword that would reach outside the two buffers is put together
//                 from guarded byte loads), d = a - b is unpacked from there with replicate padding, F is formed at the even-even points
//                 only (a quarter of the points), and the second 5 x 5 pass of a pixel collapses onto the at most 3 x 3 even-even points
//                 its clamped window meets: per axis the weights 1 8 1 or 5 5 away from the borders, by the parity of the pixel, and
//                 whatever the clamping piles up at them.  Integers up to the square root.
//   fdn_gmsd_u8 : gmsd_kernel, one 32 x 32 tile of grid points per workgroup: the block sums s of the tile and a 1-point apron in LDS,
//                 read from the 2 x 2 byte blocks directly, Prewitt in integers, q and m in double.
//   fold_kernel : one workgroup per image adds the tiles' partial sums in a fixed order.
// No atomics: a tile's sums are fixed trees over its 256 threads, an image's sums a fixed walk over its tiles.  q is defined with one
// rounding per operation, so contraction into FMAs is off in this file.
#include "common.hpp"

#include "../../include/fdn_sharpness.h"

#pragma clang fp contract(off)

namespace {

constexpr int ET = FDN_EDGE_TILE, EAP = 4, EA = ET + 2 * EAP;   // 40 x 40 apron of d
constexpr int RAW_DW = (EA * 3 + 3 + 3) / 4;                  // 31: dwords that cover a row's 120 bytes at any alignment
constexpr int RAW_LD = 32;
constexpr int FD = ET / 2 + 3;                                // even points y0 - 2, y0, ..., y0 + ET, and one zero slot behind them
constexpr int GT = FDN_GMSD_TILE, GA = GT + 2, GA_LD = GA + 1;
constexpr long long GMSD_T = 24480000000LL;                   // 170 * 144e6

static_assert(ET % 2 == 0, "a tile starts at an even coordinate: the parity of a pixel is that of its place in the tile");
static_assert(RAW_DW <= RAW_LD, "a staged row");
static_assert(ET * ET == 4 * 256 && GT * GT == 4 * 256, "four outputs per thread");

__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

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

// the aligned dword at address q of a buffer [lo, hi): one load where it lies inside, else its bytes inside, zero for the rest
__device__ __forceinline__ unsigned load_dword(uintptr_t q, uintptr_t lo, uintptr_t hi) {
    if (q >= lo && q + 4 <= hi) return *reinterpret_cast<const unsigned*>(q);
    unsigned v = 0;
#pragma unroll
    for (int t = 0; t < 4; ++t)
        if (q + t >= lo && q + t < hi) v |= (unsigned)*reinterpret_cast<const unsigned char*>(q + t) << (8 * t);
    return v;
}

// the weights the clamped 5-tap window of coordinate p (in [0, n)) leaves on the even coordinates e, e + 2, e + 4, e = p - 2 + (p & 1)
__device__ __forceinline__ void even_weights(int p, int n, int (&wt)[3]) {
    const int k[5] = {1, 5, 8, 5, 1};
    const int e = p - 2 + (p & 1);
    wt[0] = wt[1] = wt[2] = 0;
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        const int c = clampi(p + i - 2, n - 1);
        if (!(c & 1)) {
            const int s = (c - e) >> 1;                          // 0 .. 2: c >= max(p - 2, 0) >= e, c <= p + 2 <= e + 4
            wt[0] += s == 0 ? k[i] : 0;
            wt[1] += s == 1 ? k[i] : 0;
            wt[2] += s == 2 ? k[i] : 0;
        }
    }
}

// grid B * tiles; part [image][tile] = the tile's sum of e.  nbytes: the bytes of a and of b, 3 B h w.
__global__ __launch_bounds__(256) void edge_kernel(const unsigned char* __restrict__ a, const unsigned char* __restrict__ b, int h, int w,
                                                   int tiles_x, int tiles, long nbytes, int* __restrict__ resid, double* __restrict__ part) {
    __shared__ unsigned raw[2][EA][RAW_LD];                     // the staged rows of a and of b
    __shared__ int d[3][EA][EA + 1];                            // a - b per channel, replicate-padded
    __shared__ int F[3][FD][FD];
    __shared__ double red[256];
    const int tid = threadIdx.x;
    const long image = blockIdx.x / tiles;
    const int tile = (int)(blockIdx.x - image * tiles);
    const int y0 = (tile / tiles_x) * ET, x0 = (tile % tiles_x) * ET;
    const int xlo = x0 - EAP < 0 ? 0 : x0 - EAP, xhi = x0 + ET + EAP - 1 > w - 1 ? w - 1 : x0 + ET + EAP - 1;
    const int row_bytes = (xhi - xlo + 1) * 3;
    const uintptr_t lo[2] = {reinterpret_cast<uintptr_t>(a), reinterpret_cast<uintptr_t>(b)};

    for (int i = tid; i < 2 * EA * RAW_DW; i += 256) {
        const int which = i / (EA * RAW_DW), rem = i - which * (EA * RAW_DW);
        const int r = rem / RAW_DW, k = rem - r * RAW_DW;
        const int yy = clampi(y0 - EAP + r, h - 1);
        const uintptr_t p = lo[which] + ((image * h + yy) * (long)w + xlo) * 3;
        const unsigned sh = (unsigned)(p & 3);
        if (4 * k < (int)sh + row_bytes) raw[which][r][k] = load_dword(p - sh + 4 * (uintptr_t)k, lo[which], lo[which] + (uintptr_t)nbytes);
    }
    __syncthreads();
    for (int i = tid; i < EA * EA; i += 256) {
        const int r = i / EA, c = i - r * EA;
        const int yy = clampi(y0 - EAP + r, h - 1), xx = clampi(x0 - EAP + c, w - 1);     // replicate padding
        const long row = ((image * h + yy) * (long)w + xlo) * 3;
        const int oa = (int)((lo[0] + row) & 3) + (xx - xlo) * 3, ob = (int)((lo[1] + row) & 3) + (xx - xlo) * 3;
        const unsigned char* ra = reinterpret_cast<const unsigned char*>(raw[0][r]);
        const unsigned char* rb = reinterpret_cast<const unsigned char*>(raw[1][r]);
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) d[ch][r][c] = (int)ra[oa + ch] - (int)rb[ob + ch];
    }
    __syncthreads();
    // F at the even points (y0 - 2 + 2 fy, x0 - 2 + 2 fx) that lie in the image; the others are never met with a weight, and are zero
    for (int i = tid; i < 3 * FD * FD; i += 256) {
        const int ch = i / (FD * FD), rem = i - ch * (FD * FD);
        const int fy = rem / FD, fx = rem - fy * FD;
        const int qy = y0 - 2 + 2 * fy, qx = x0 - 2 + 2 * fx;
        int v = 0;
        if (fy < FD - 1 && fx < FD - 1 && qy >= 0 && qy < h && qx >= 0 && qx < w) {
            const int k[5] = {1, 5, 8, 5, 1};
#pragma unroll
            for (int iy = 0; iy < 5; ++iy) {
                int rs = 0;
#pragma unroll
                for (int ix = 0; ix < 5; ++ix) rs += k[ix] * d[ch][2 * fy + iy][2 * fx + ix];     // apron row of qy + iy - 2 is 2 fy + iy
                v += k[iy] * rs;
            }
        }
        F[ch][fy][fx] = v;
    }
    __syncthreads();
    const int px = tid & 31, py = (tid >> 5) * 4;
    double sum = 0.0;
    int wx[3];
    const bool xin = x0 + px < w;
    if (xin) even_weights(x0 + px, w, wx);
    const int fx0 = (px + (px & 1)) >> 1;                       // (x - 2 + (x & 1) - (x0 - 2)) / 2
#pragma unroll 1
    for (int j = 0; j < 4; ++j) {
        const int y = y0 + py + j;
        if (!xin || y >= h) continue;
        int wy[3];
        even_weights(y, h, wy);
        const int fy0 = (py + j + ((py + j) & 1)) >> 1;
        const long at = ((image * h + y) * (long)w + x0 + px) * 3;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            int acc = 0;
#pragma unroll
            for (int s = 0; s < 3; ++s)
#pragma unroll
                for (int t = 0; t < 3; ++t) acc += wy[s] * wx[t] * F[ch][fy0 + s][fx0 + t];
            const int N = 160000 * d[ch][py + j + EAP][px + EAP] - 4 * acc;
            if (resid) resid[at + ch] = N;
            const double r = (double)N / 40800000.0;
            sum += sqrt(r * r + 1e-6);
        }
    }
    const double total = block_sum(sum, red, tid);
    if (tid == 0) part[blockIdx.x] = total;
}

// grid B * tiles; part [image][tile][4] = the tile's sums of q, q^2, m of a, m of b
__global__ __launch_bounds__(256) void gmsd_kernel(const unsigned char* __restrict__ a, const unsigned char* __restrict__ b, int h, int w, int hd,
                                                   int wd, int bgr, int tiles_x, int tiles, long long* __restrict__ grad2,
                                                   float* __restrict__ map, double* __restrict__ part) {
    __shared__ int s[2][GA][GA_LD];
    __shared__ double red[256];
    const int tid = threadIdx.x;
    const long image = blockIdx.x / tiles;
    const int tile = (int)(blockIdx.x - image * tiles);
    const int i0 = (tile / tiles_x) * GT, j0 = (tile % tiles_x) * GT;
    const int ir = bgr ? 2 : 0, ib = bgr ? 0 : 2;
    for (int it = tid; it < 2 * GA * GA; it += 256) {
        const int which = it / (GA * GA), rem = it - which * (GA * GA);
        const int r = rem / GA, c = rem - r * GA;
        const int gi = i0 - 1 + r, gj = j0 - 1 + c;
        int v = 0;
        if (gi >= 0 && gi < hd && gj >= 0 && gj < wd) {
            const unsigned char* img = (which ? b : a) + image * h * (long)w * 3;
#pragma unroll
            for (int dy = 0; dy < 2; ++dy)
#pragma unroll
                for (int dx = 0; dx < 2; ++dx) {
                    const int y = 2 * gi + dy, x = 2 * gj + dx;
                    if (y < h && x < w) {
                        const unsigned char* p = img + ((long)y * w + x) * 3;
                        v += 299 * p[ir] + 587 * p[1] + 114 * p[ib];
                    }
                }
        }
        s[which][r][c] = v;
    }
    __syncthreads();
    const int px = tid & 31, py = (tid >> 5) * 4;
    double sq = 0.0, sq2 = 0.0, sma = 0.0, smb = 0.0;
#pragma unroll 1
    for (int j = 0; j < 4; ++j) {
        const int gi = i0 + py + j, gj = j0 + px;
        if (gi >= hd || gj >= wd) continue;
        const int r = py + j + 1, c = px + 1;
        long long A[2];
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            int gx = 0, gy = 0;
#pragma unroll
            for (int t = -1; t <= 1; ++t) {
                gx += s[k][r + t][c + 1] - s[k][r + t][c - 1];
                gy += s[k][r + 1][c + t] - s[k][r - 1][c + t];
            }
            A[k] = (long long)gx * gx + (long long)gy * gy;
            if (grad2) grad2[((image * 2 + k) * hd + gi) * (long)wd + gj] = A[k];
        }
        const double da = (double)A[0], db = (double)A[1];
        const double q = (2.0 * sqrt(da * db) + (double)GMSD_T) / (double)(A[0] + A[1] + GMSD_T);
        if (map) map[(image * hd + gi) * (long)wd + gj] = (float)q;
        sq += q;
        sq2 += q * q;
        sma += sqrt(da) / 12000.0;
        smb += sqrt(db) / 12000.0;
    }
    double* o = part + 4 * (long)blockIdx.x;
    const double t0 = block_sum(sq, red, tid), t1 = block_sum(sq2, red, tid), t2 = block_sum(sma, red, tid), t3 = block_sum(smb, red, tid);
    if (tid == 0) {
        o[0] = t0;
        o[1] = t1;
        o[2] = t2;
        o[3] = t3;
    }
}

// grid B: out [image][nv] = the sums of part [image][tile][nv] over the tiles, thread t walking tiles t, t + 256, ... in order, then the tree
__global__ __launch_bounds__(256) void fold_kernel(const double* __restrict__ part, int tiles, int nv, double* __restrict__ out) {
    __shared__ double red[256];
    const int tid = threadIdx.x;
    const double* p = part + (long)blockIdx.x * tiles * nv;
#pragma unroll 1
    for (int v = 0; v < nv; ++v) {
        double sum = 0.0;
        for (int t = tid; t < tiles; t += 256) sum += p[(long)t * nv + v];
        const double total = block_sum(sum, red, tid);
        if (tid == 0) out[(long)blockIdx.x * nv + v] = total;
    }
}

bool size_ok(int B, int h, int w) { return B >= 1 && h >= 1 && w >= 1 && (long)h * w <= 0x7FFFFFFFL; }
bool aligned8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7u) == 0; }
long edge_tiles(int h, int w) { return (long)cdiv(h, ET) * cdiv(w, ET); }
long gmsd_tiles(int h, int w) { return (long)cdiv((h + 1) / 2, GT) * cdiv((w + 1) / 2, GT); }
bool gmsd_ok(int B, int h, int w) { return size_ok(B, h, w) && (long)((h + 1) / 2) * ((w + 1) / 2) >= 2; }

}  // namespace

extern "C" int fdn_sharpness_abi_version(void) { return FDN_SHARPNESS_ABI_VERSION; }

extern "C" long fdn_edge_ws(int B, int h, int w) { return size_ok(B, h, w) ? B * edge_tiles(h, w) : 0; }

extern "C" int fdn_edge_u8(const unsigned char* a, const unsigned char* b, int B, int h, int w, int* resid, double* ws, double* out,
                           fdn_stream_t stream) {
    FDN_CHECK_ARG(a && b && ws && out && aligned8(ws) && size_ok(B, h, w));
    const long tiles = edge_tiles(h, w);
    if (B * tiles > 0x7FFFFFFFL) return FDN_ERR_UNSUPPORTED;
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(edge_kernel, dim3((unsigned)(B * tiles)), dim3(256), 0, s, a, b, h, w, cdiv(w, ET), (int)tiles, 3L * B * h * w, resid, ws);
    hipLaunchKernelGGL(fold_kernel, dim3((unsigned)B), dim3(256), 0, s, (const double*)ws, (int)tiles, 1, out);
    return fdn_launch_status();
}

extern "C" int fdn_gmsd_dims(int h, int w, int* hd, int* wd) {
    FDN_CHECK_ARG(hd && wd && size_ok(1, h, w));
    *hd = (h + 1) / 2;
    *wd = (w + 1) / 2;
    return FDN_OK;
}

extern "C" long fdn_gmsd_ws(int B, int h, int w) { return gmsd_ok(B, h, w) ? 4L * B * gmsd_tiles(h, w) : 0; }

extern "C" int fdn_gmsd_u8(const unsigned char* a, const unsigned char* b, int B, int h, int w, int bgr, long* grad2, float* map, double* ws,
                           double* out, fdn_stream_t stream) {
    FDN_CHECK_ARG(a && b && ws && out && aligned8(ws) && gmsd_ok(B, h, w));
    static_assert(sizeof(long) == sizeof(long long), "grad2 is 64-bit");
    const long tiles = gmsd_tiles(h, w);
    if (B * tiles > 0x7FFFFFFFL) return FDN_ERR_UNSUPPORTED;
    const int hd = (h + 1) / 2, wd = (w + 1) / 2;
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(gmsd_kernel, dim3((unsigned)(B * tiles)), dim3(256), 0, s, a, b, h, w, hd, wd, bgr != 0 ? 1 : 0, cdiv(wd, GT), (int)tiles,
                       reinterpret_cast<long long*>(grad2), map, ws);
    hipLaunchKernelGGL(fold_kernel, dim3((unsigned)B), dim3(256), 0, s, (const double*)ws, (int)tiles, 4, out);
    return fdn_launch_status();
}
