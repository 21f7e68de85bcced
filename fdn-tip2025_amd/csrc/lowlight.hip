// Low-light evaluation (include/fdn_lowlight.h): the lightness order error of an input against its enhanced version, and the CIEDE2000
// colour difference of a restored image against its ground truth, both from 8-bit images [B][h][w][3].
//   fdn_loe_u8      : LOE from the 256 x 256 joint histogram J of (La, Lb), L = max(R, G, B) - no pair of pixels is compared:
//                     loe_zero_kernel    J = 0 (a launch zeroes what it accumulates into)
//                     loe_hist_kernel    a workgroup counts up to CHUNK samples in a private histogram in LDS, then adds the bins it
//                                        touched to J with integer atomics (whose result does not depend on order)
//                     loe_tables_kernel  one workgroup per image: C = the inclusive 2-D prefix sum of J, R[x] = C[x][255],
//                                        K[y] = C[255][y], numerator = sum J (R + K - 2 C) in 64-bit integers
//   fdn_loe_map_u8  : loe_map_kernel, RD = R[La] + K[Lb] - 2 C[La][Lb] per sample, from the tables fdn_loe_u8 left in the workspace
//   fdn_deltae00_u8 : deltae_kernel, float64 per pixel from the bytes, per tile of TILE pixels {sum, max} in the workspace, and
//                     deltae_fold_kernel, one fixed fold per image.  No floating-point atomic.
// The private histogram: 65536 bins of uint32 are 256 KB and do not fit the 160 KB of LDS, but a workgroup that counts at most
// CHUNK <= 65535 samples needs 16 bits per bin, 128 KB: two bins share a 32-bit word, a sample adds 1 or 1 << 16 to it with an LDS atomic,
// and the low half cannot carry into the high one.  Low-light inputs crowd a few lightness values, so the same bin is hit over and over;
// in LDS that costs a few cycles per hit, and J in L2 sees one atomic per touched bin and workgroup instead of one per sample.
#include "common.hpp"

#include "../../include/fdn_lowlight.h"

#pragma clang fp contract(off)

namespace {

constexpr int BINS = 256 * 256;
constexpr long LOE_WORDS = (2L * BINS + 512) * 4 / 8;              // 8-byte words per image: J, C, R, K as uint32
constexpr int HT = 1024;                                           // threads of the LOE workgroups
constexpr int CHUNK = 32768;                                       // samples per histogram workgroup
constexpr size_t HIST_LDS = (size_t)BINS / 2 * sizeof(unsigned);   // 128 KB: two 16-bit bins per word
static_assert(CHUNK <= 65535, "a 16-bit bin must hold a whole chunk");

struct loe_tables {
    unsigned *J, *C, *R, *K;
};
__device__ __forceinline__ loe_tables tables_of(void* ws, long image) {
    unsigned* p = reinterpret_cast<unsigned*>(reinterpret_cast<unsigned long long*>(ws) + image * LOE_WORDS);
    return {p, p + BINS, p + 2 * BINS, p + 2 * BINS + 256};
}

// the sample grid of include/fdn_lowlight.h; false = bad arguments
bool sample_dims(int h, int w, int size, int* md, int* nd) {
    if (h < 1 || w < 1 || size < 0 || (long)h * w > 0x7FFFFFFFL) return false;
    const long s = h < w ? h : w;
    if (size == 0 || s <= size) {
        *md = h;
        *nd = w;
    } else {
        *md = (int)((2L * h * size + s) / (2 * s));
        *nd = (int)((2L * w * size + s) / (2 * s));
    }
    return true;
}

// lightness pair of sample s of an image: (La << 8) | Lb
__device__ __forceinline__ unsigned sample_key(const unsigned char* __restrict__ a, const unsigned char* __restrict__ b, long s, int h, int w,
                                               int Md, int Nd, bool full) {
    long pix = s;
    if (!full) {
        const long i = s / Nd, j = s - i * Nd;
        pix = (((2 * i + 1) * h) / (2L * Md)) * w + ((2 * j + 1) * w) / (2L * Nd);
    }
    const unsigned char *pa = a + pix * 3, *pb = b + pix * 3;
    const unsigned la = max(max((unsigned)pa[0], (unsigned)pa[1]), (unsigned)pa[2]);
    const unsigned lb = max(max((unsigned)pb[0], (unsigned)pb[1]), (unsigned)pb[2]);
    return (la << 8) | lb;
}

// grid B * 16: J of every image = 0
__global__ __launch_bounds__(HT) void loe_zero_kernel(void* ws) {
    const loe_tables t = tables_of(ws, blockIdx.x >> 4);
    reinterpret_cast<uint4*>(t.J)[(blockIdx.x & 15) * HT + threadIdx.x] = make_uint4(0u, 0u, 0u, 0u);
}

// grid B * chunks, HIST_LDS bytes of dynamic LDS
__global__ __launch_bounds__(HT) void loe_hist_kernel(const unsigned char* __restrict__ a, const unsigned char* __restrict__ b, int h, int w,
                                                      int Md, int Nd, int full, int chunks, void* ws) {
    extern __shared__ unsigned hist[];                              // [BINS / 2]: bin 2 i in the low half of word i, bin 2 i + 1 in the high
    const int tid = threadIdx.x;
    const long image = blockIdx.x / chunks;
    const int chunk = (int)(blockIdx.x - image * chunks);
    for (int i = tid; i < BINS / 2; i += HT) hist[i] = 0u;
    __syncthreads();
    const long m = (long)Md * Nd, s0 = (long)chunk * CHUNK, s1 = s0 + CHUNK < m ? s0 + CHUNK : m;
    const long base = image * h * w * 3;
    for (long s = s0 + tid; s < s1; s += HT) {
        const unsigned key = sample_key(a + base, b + base, s, h, w, Md, Nd, full != 0);
        atomicAdd(&hist[key >> 1], (key & 1u) ? 0x10000u : 1u);
    }
    __syncthreads();
    const loe_tables t = tables_of(ws, image);
    for (int i = tid; i < BINS / 2; i += HT) {
        const unsigned v = hist[i];
        if (v & 0xFFFFu) atomicAdd(&t.J[2 * i], v & 0xFFFFu);
        if (v >> 16) atomicAdd(&t.J[2 * i + 1], v >> 16);
    }
}

// grid B: the tables C, R, K of one image from its J, and out[image] = {numerator, m}
__global__ __launch_bounds__(HT) void loe_tables_kernel(void* ws, long m, long* __restrict__ out) {
    __shared__ unsigned segtot[4][256], sR[256];
    __shared__ __align__(16) unsigned sK[256];
    __shared__ unsigned long long wsum[HT / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const loe_tables t = tables_of(ws, blockIdx.x);
    {   // along x: thread = (segment of 64 rows, column y); requests run along y
        const int y = tid & 255, seg = tid >> 8;
        const unsigned* j = t.J + seg * 64 * 256 + y;
        unsigned tot = 0u;
#pragma unroll 16
        for (int k = 0; k < 64; ++k) tot += j[k * 256];
        segtot[seg][y] = tot;
        __syncthreads();
        unsigned run = 0u;                                          // the segments above this one, then J once more (it sits in L2)
        for (int s = 0; s < seg; ++s) run += segtot[s][y];
        unsigned* c = t.C + seg * 64 * 256 + y;
#pragma unroll 16
        for (int k = 0; k < 64; ++k) {
            run += j[k * 256];
            c[k * 256] = run;
        }
    }
    __threadfence();
    __syncthreads();
    // along y: a wave per row, a lane holds four consecutive y
    for (int r = 0; r < 256 / (HT / 64); ++r) {
        const int x = wave * (256 / (HT / 64)) + r;
        uint4 c = reinterpret_cast<const uint4*>(t.C)[x * 64 + lane];
        c.y += c.x;
        c.z += c.y;
        c.w += c.z;
        unsigned run = c.w;                                         // inclusive scan of the lanes' totals
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const unsigned up = __shfl_up(run, d);
            if (lane >= d) run += up;
        }
        const unsigned before = run - c.w;
        c.x += before;
        c.y += before;
        c.z += before;
        c.w += before;
        reinterpret_cast<uint4*>(t.C)[x * 64 + lane] = c;
        if (lane == 63) {
            sR[x] = c.w;
            t.R[x] = c.w;
        }
        if (x == 255) {
            reinterpret_cast<uint4*>(sK)[lane] = c;
            reinterpret_cast<uint4*>(t.K)[lane] = c;
        }
    }
    __threadfence();
    __syncthreads();
    unsigned long long acc = 0ull;
    for (int i = tid; i < BINS; i += HT) {
        const unsigned long long j = t.J[i];
        acc += j * ((unsigned long long)sR[i >> 8] + sK[i & 255] - 2ull * t.C[i]);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off);
    if (lane == 0) wsum[wave] = acc;
    __syncthreads();
    if (tid == 0) {
        unsigned long long s = 0ull;
        for (int k = 0; k < HT / 64; ++k) s += wsum[k];
        out[2 * blockIdx.x] = (long)s;
        out[2 * blockIdx.x + 1] = m;
    }
}

// grid (blocks, B): rd[image][s] of every sample
__global__ __launch_bounds__(256) void loe_map_kernel(const unsigned char* __restrict__ a, const unsigned char* __restrict__ b, int h, int w,
                                                      int Md, int Nd, int full, const void* ws, unsigned* __restrict__ rd) {
    const long image = blockIdx.y, m = (long)Md * Nd;
    const loe_tables t = tables_of(const_cast<void*>(ws), image);
    const long base = image * h * w * 3;
    for (long s = (long)blockIdx.x * 256 + threadIdx.x; s < m; s += (long)gridDim.x * 256) {
        const unsigned key = sample_key(a + base, b + base, s, h, w, Md, Nd, full != 0);
        rd[image * m + s] = t.R[key >> 8] + t.K[key & 255u] - 2u * t.C[key];
    }
}

// ---- CIEDE2000 ----
constexpr int DT = 256, PER = 4, TILE = DT * PER;                  // pixels per workgroup: thread t takes pixels t, t + 256, ... of the tile
constexpr double PI = 3.14159265358979323846, DEG = 180.0 / PI, RAD = PI / 180.0;

struct lab_t {
    double L, a, b;
};

__device__ __forceinline__ double lab_f(double t) {
    constexpr double d = 6.0 / 29.0;
    return t > d * d * d ? cbrt(t) : t / (3.0 * d * d) + 4.0 / 29.0;
}

__device__ __forceinline__ lab_t lab_of(double r, double g, double b) {
    const double fx = lab_f((0.4124564 * r + 0.3575761 * g + 0.1804375 * b) / 0.95047);
    const double fy = lab_f((0.2126729 * r + 0.7151522 * g + 0.0721750 * b) / 1.0);
    const double fz = lab_f((0.0193339 * r + 0.1191920 * g + 0.9503041 * b) / 1.08883);
    return {116.0 * fy - 16.0, 500.0 * (fx - fy), 200.0 * (fy - fz)};
}

// hue in degrees, [0, 360]; 0 where both are 0
__device__ __forceinline__ double hue_of(double b, double ap) {
    if (ap == 0.0 && b == 0.0) return 0.0;
    const double hd = atan2(b, ap) * DEG;
    return hd < 0.0 ? hd + 360.0 : hd;
}

// Sharma, Wu, Dalal 2005 with kL = kC = kH = 1, every step in the order tests/lowlight_ref.py writes it
__device__ double deltae00(lab_t p, lab_t q) {
    constexpr double P25 = 6103515625.0;                            // 25^7
    const double C1 = hypot(p.a, p.b), C2 = hypot(q.a, q.b), Cb = (C1 + C2) / 2.0;
    const double Cb7 = pow(Cb, 7.0);
    const double G = 0.5 * (1.0 - sqrt(Cb7 / (Cb7 + P25)));
    const double a1 = (1.0 + G) * p.a, a2 = (1.0 + G) * q.a;
    const double C1p = hypot(a1, p.b), C2p = hypot(a2, q.b);
    const double h1 = hue_of(p.b, a1), h2 = hue_of(q.b, a2);
    const double dL = q.L - p.L, dC = C2p - C1p;
    const bool z = C1p * C2p == 0.0;
    double dh = h2 - h1;
    dh = z ? 0.0 : dh > 180.0 ? dh - 360.0 : dh < -180.0 ? dh + 360.0 : dh;
    const double dH = 2.0 * sqrt(C1p * C2p) * sin(dh / 2.0 * RAD);
    const double Lb = (p.L + q.L) / 2.0, Cbp = (C1p + C2p) / 2.0;
    const double hs = h1 + h2, ad = fabs(h1 - h2);
    const double hb = z ? hs : ad <= 180.0 ? hs / 2.0 : hs < 360.0 ? (hs + 360.0) / 2.0 : (hs - 360.0) / 2.0;
    const double T = 1.0 - 0.17 * cos((hb - 30.0) * RAD) + 0.24 * cos(2.0 * hb * RAD) + 0.32 * cos((3.0 * hb + 6.0) * RAD) -
                     0.20 * cos((4.0 * hb - 63.0) * RAD);
    const double u = (hb - 275.0) / 25.0;
    const double dth = 30.0 * exp(-(u * u));
    const double Cp7 = pow(Cbp, 7.0);
    const double Rc = 2.0 * sqrt(Cp7 / (Cp7 + P25));
    const double l2 = (Lb - 50.0) * (Lb - 50.0);
    const double Sl = 1.0 + 0.015 * l2 / sqrt(20.0 + l2), Sc = 1.0 + 0.045 * Cbp, Sh = 1.0 + 0.015 * Cbp * T;
    const double Rt = -sin(2.0 * dth * RAD) * Rc;
    const double tl = dL / Sl, tc = dC / Sc, th = dH / Sh;
    return sqrt(tl * tl + tc * tc + th * th + Rt * tc * th);
}

// grid B * tiles; part [image][tile][2] = {sum, max} of the tile's pixels
__global__ __launch_bounds__(DT) void deltae_kernel(const unsigned char* __restrict__ a, const unsigned char* __restrict__ b, long npix, int bgr,
                                                    int tiles, float* __restrict__ map, double* __restrict__ part) {
    __shared__ double lin[256], wsum[DT / 64], wmax[DT / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    {   // sRGB decode of the 256 byte values, IEC 61966-2-1
        const double c = (double)tid / 255.0;
        lin[tid] = c <= 0.04045 ? c / 12.92 : pow((c + 0.055) / 1.055, 2.4);
    }
    __syncthreads();
    const long image = blockIdx.x / tiles;
    const long tile = blockIdx.x - image * tiles;
    const unsigned char *ia = a + image * npix * 3, *ib = b + image * npix * 3;
    const int ir = bgr ? 2 : 0, ib_ = bgr ? 0 : 2;
    double sum = 0.0, mx = 0.0;
#pragma unroll 1
    for (int k = 0; k < PER; ++k) {
        const long p = tile * TILE + k * DT + tid;
        if (p < npix) {
            const unsigned char *pa = ia + p * 3, *pb = ib + p * 3;
            const double de = deltae00(lab_of(lin[pa[ir]], lin[pa[1]], lin[pa[ib_]]), lab_of(lin[pb[ir]], lin[pb[1]], lin[pb[ib_]]));
            if (map) map[image * npix + p] = (float)de;
            sum += de;
            mx = de > mx ? de : mx;
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        sum += __shfl_down(sum, off);
        const double o = __shfl_down(mx, off);
        mx = o > mx ? o : mx;
    }
    if (lane == 0) {
        wsum[wave] = sum;
        wmax[wave] = mx;
    }
    __syncthreads();
    if (tid == 0) {
        for (int k = 1; k < DT / 64; ++k) {
            sum += wsum[k];
            mx = wmax[k] > mx ? wmax[k] : mx;
        }
        part[2 * (long)blockIdx.x] = sum;
        part[2 * (long)blockIdx.x + 1] = mx;
    }
}

// grid B: out[image] = {sum, max} of the image's tiles, thread t walking tiles t, t + 256, ... in order, then one fixed tree
__global__ __launch_bounds__(DT) void deltae_fold_kernel(const double* __restrict__ part, int tiles, double* __restrict__ out) {
    __shared__ double wsum[DT / 64], wmax[DT / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const double* p = part + 2 * (long)blockIdx.x * tiles;
    double sum = 0.0, mx = 0.0;
    for (int t = tid; t < tiles; t += DT) {
        sum += p[2 * (long)t];
        const double o = p[2 * (long)t + 1];
        mx = o > mx ? o : mx;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        sum += __shfl_down(sum, off);
        const double o = __shfl_down(mx, off);
        mx = o > mx ? o : mx;
    }
    if (lane == 0) {
        wsum[wave] = sum;
        wmax[wave] = mx;
    }
    __syncthreads();
    if (tid == 0) {
        for (int k = 1; k < DT / 64; ++k) {
            sum += wsum[k];
            mx = wmax[k] > mx ? wmax[k] : mx;
        }
        out[2 * blockIdx.x] = sum;
        out[2 * blockIdx.x + 1] = mx;
    }
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

}  // namespace

extern "C" int fdn_lowlight_abi_version(void) { return FDN_LOWLIGHT_ABI_VERSION; }

extern "C" int fdn_loe_sample_dims(int h, int w, int size, int* md, int* nd) {
    FDN_CHECK_ARG(md && nd && sample_dims(h, w, size, md, nd));
    return FDN_OK;
}

extern "C" long fdn_loe_ws(int B, int h, int w, int size) {
    int md, nd;
    if (B < 1 || !sample_dims(h, w, size, &md, &nd)) return 0;
    return B * LOE_WORDS;
}

extern "C" int fdn_loe_u8(const unsigned char* a, const unsigned char* b, int B, int h, int w, int size, void* ws, long* out,
                          fdn_stream_t stream) {
    int Md, Nd;
    FDN_CHECK_ARG(a && b && ws && out && aligned16(ws) && B >= 1 && sample_dims(h, w, size, &Md, &Nd));
    const long m = (long)Md * Nd;
    const int chunks = cdiv(m, CHUNK);
    if ((long)B * chunks > 0x7FFFFFFFL || (long)B * 16 > 0x7FFFFFFFL) return FDN_ERR_UNSUPPORTED;
    if (!fdn_allow_dynamic_lds(reinterpret_cast<const void*>(loe_hist_kernel), HIST_LDS)) return FDN_ERR_LAUNCH;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int full = Md == h && Nd == w;
    hipLaunchKernelGGL(loe_zero_kernel, dim3((unsigned)B * 16u), dim3(HT), 0, s, ws);
    hipLaunchKernelGGL(loe_hist_kernel, dim3((unsigned)(B * chunks)), dim3(HT), HIST_LDS, s, a, b, h, w, Md, Nd, full, chunks, ws);
    hipLaunchKernelGGL(loe_tables_kernel, dim3((unsigned)B), dim3(HT), 0, s, ws, m, out);
    return fdn_launch_status();
}

extern "C" int fdn_loe_map_u8(const unsigned char* a, const unsigned char* b, int B, int h, int w, int size, const void* ws, unsigned* rd,
                              fdn_stream_t stream) {
    int Md, Nd;
    FDN_CHECK_ARG(a && b && ws && rd && aligned16(ws) && B >= 1 && sample_dims(h, w, size, &Md, &Nd));
    if (B > 65535) return FDN_ERR_UNSUPPORTED;
    const long m = (long)Md * Nd;
    const long blocks = (m + 255) / 256;
    hipLaunchKernelGGL(loe_map_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096), (unsigned)B), dim3(256), 0, static_cast<hipStream_t>(stream),
                       a, b, h, w, Md, Nd, (int)(Md == h && Nd == w), ws, rd);
    return fdn_launch_status();
}

extern "C" long fdn_deltae00_ws(int B, int h, int w) {
    if (B < 1 || h < 1 || w < 1 || (long)h * w > 0x7FFFFFFFL) return 0;
    return 2L * B * (((long)h * w + TILE - 1) / TILE);
}

extern "C" int fdn_deltae00_u8(const unsigned char* a, const unsigned char* b, int B, int h, int w, int bgr, float* map, double* ws,
                               double* out, fdn_stream_t stream) {
    FDN_CHECK_ARG(a && b && ws && out && B >= 1 && h >= 1 && w >= 1 && (long)h * w <= 0x7FFFFFFFL);
    const long npix = (long)h * w;
    const int tiles = cdiv(npix, TILE);
    if ((long)B * tiles > 0x7FFFFFFFL) return FDN_ERR_UNSUPPORTED;
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(deltae_kernel, dim3((unsigned)(B * (long)tiles)), dim3(DT), 0, s, a, b, npix, bgr != 0 ? 1 : 0, tiles, map, ws);
    hipLaunchKernelGGL(deltae_fold_kernel, dim3((unsigned)B), dim3(DT), 0, s, (const double*)ws, tiles, out);
    return fdn_launch_status();
}
