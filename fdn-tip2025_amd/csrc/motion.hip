// Motion-compensated temporal consistency (include/fdn_motion.h, ABI 1; linked into libfdn_motion.so, beside libfdn_hip.so).  The header
// has the definitions.
//   fdn_motion_search   : search_kernel.  A workgroup of 256 threads walks 16 x 16 blocks of one frame.  Per block the current block and the
//                         (16 + 2R)^2 window of the previous frame are staged in LDS, clamped to the frame and to the top code as they are
//                         loaded, as packed samples: four to a dword for 8 bit, two for 10 bit.  Four neighbouring lanes share a candidate,
//                         four rows of the block each: a row of the window is read as aligned dwords, realigned to the candidate's column
//                         with v_alignbyte_b32 and summed against the block's row with v_sad_u8 / v_sad_u16; the four partial sums meet
//                         through two lane swaps.  key = SAD << 11 | rank; min over the wave by swaps, over the four waves through four
//                         words of LDS.  The one lane that holds the winning key writes the block's row and keeps the four totals, which
//                         leave the workgroup as at most four 64-bit atomic adds.
//   fdn_motion_residual : residual_kernel, one pass over the pixels with the block's vector: tiles of 64 x 16 pixels (four blocks side by
//                         side), a thread owns a column of four rows; the five sums as above.
// Every quantity is an integer and every sum is exact whatever the order.  One squared difference of differences is at most 2046^2 and a
// thread's four fit 32 bits unsigned; everything wider than a wave's sum of those is kept in 64 bits.
// The pitch of a window row is one dword more than the 48 samples need (13 dwords for 8 bit, 25 for 10 bit): odd, so the rows that the
// lanes of one LDS access touch - consecutive candidates, and the four row groups 4 rows apart - fall on different banks.
#include "common.hpp"

#include "../../include/fdn_motion.h"

namespace {

constexpr int BS = FDN_MOTION_BLOCK, MAXR = FDN_MOTION_MAX_RADIUS, WIN = BS + 2 * MAXR, NC = 2 * MAXR + 1;
constexpr int SEARCH_MAX_GRID = 1024, RESIDUAL_MAX_GRID = 256;      // workgroups per frame: what bounds the atomics on a frame's totals

static_assert(BS * BS == 256 && NC * NC < (1 << 11) && 256 * 1023 < (1 << 18), "one thread per pixel when staging; the key fits 29 bits");

// rank of (dy, dx) among the candidates of [-16, 16]^2 in the order (dy^2 + dx^2, dy, dx), at [(dy + 16) * 33 + dx + 16]: a counting sort
// by the squared length, the raster walk being the order (dy, dx) within one length
struct Ranks {
    unsigned short r[NC * NC];
};
constexpr Ranks make_ranks() {
    Ranks t{};
    int start[2 * MAXR * MAXR + 2] = {};
    for (int dy = -MAXR; dy <= MAXR; ++dy)
        for (int dx = -MAXR; dx <= MAXR; ++dx) ++start[dy * dy + dx * dx + 1];
    for (int i = 1; i < 2 * MAXR * MAXR + 2; ++i) start[i] += start[i - 1];
    for (int dy = -MAXR; dy <= MAXR; ++dy)
        for (int dx = -MAXR; dx <= MAXR; ++dx) t.r[(dy + MAXR) * NC + dx + MAXR] = (unsigned short)start[dy * dy + dx * dx]++;
    return t;
}
static __device__ const Ranks RANKS = make_ranks();

__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

template <typename S>
__device__ __forceinline__ unsigned sad_packed(unsigned a, unsigned b, unsigned acc) {
    if constexpr (sizeof(S) == 1) return __builtin_amdgcn_sad_u8(a, b, acc);
    else return __builtin_amdgcn_sad_u16(a, b, acc);
}

// sum over the workgroup of K 64-bit totals per thread -> atomic adds onto out[0 .. K), zeros left out
template <int K>
__device__ __forceinline__ void add_totals(unsigned long long (&acc)[K], unsigned long long (*s_acc)[K], unsigned long long* __restrict__ out) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        unsigned long long v = acc[k];
        for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
        if ((tid & 63) == 0) s_acc[tid >> 6][k] = v;
    }
    __syncthreads();
    if (tid < K) {
        const unsigned long long v = s_acc[0][tid] + s_acc[1][tid] + s_acc[2][tid] + s_acc[3][tid];
        if (v) atomicAdd(&out[tid], v);
    }
}

// grid (min(blocks of a frame, SEARCH_MAX_GRID), B).  T: the frames' sample type; S: the sample type of the LDS image
template <typename T, typename S>
__global__ __launch_bounds__(256) void search_kernel(const T* __restrict__ guide, const T* __restrict__ guide_prev, short* __restrict__ mv,
                                                     unsigned* __restrict__ sad, unsigned long long* __restrict__ stats, int h, int w, int nbx,
                                                     int nblk, int R, unsigned top) {
    constexpr int SPD = 4 / sizeof(S), ND = BS / SPD, PW = WIN / SPD + 1;     // samples per dword, dwords per block row, window pitch
    __shared__ unsigned s_win[WIN * PW];
    __shared__ unsigned s_cur[BS * ND];
    __shared__ unsigned short s_rank[NC * NC];
    __shared__ unsigned s_red[4];
    __shared__ unsigned s_sad0;
    __shared__ unsigned long long s_acc[4][4];
    const int tid = threadIdx.x, b = blockIdx.y;
    const long fs = (long)h * w + ((long)h * w >> 1);
    const T* cur = guide + b * fs;
    const T* prev = b ? cur - fs : guide_prev;
    const long row0 = (long)b * nblk;
    if (!prev) {                                                    // frame 0 without a predecessor: rows of 0 (stats is cleared already)
        for (int i = blockIdx.x * 256 + tid; i < nblk; i += gridDim.x * 256) {
            if (mv) mv[(row0 + i) * 2] = mv[(row0 + i) * 2 + 1] = 0;
            if (sad) sad[(row0 + i) * 2] = sad[(row0 + i) * 2 + 1] = 0u;
        }
        return;
    }
    for (int i = tid; i < NC * NC; i += 256) s_rank[i] = RANKS.r[i];
    S* win_s = reinterpret_cast<S*>(s_win);
    S* cur_s = reinterpret_cast<S*>(s_cur);
    const int n = 2 * R + 1, wn = BS + 2 * R, nitems = 4 * n * n;   // an item: four rows of one candidate
    const int q64 = 64 / n, r64 = 64 - q64 * n;                     // a thread's next candidate is 64 further in the raster walk
    const int rg = tid & 3;
    unsigned long long acc[4] = {0, 0, 0, 0};
    for (int blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
        const int y0 = (blk / nbx) * BS, x0 = (blk % nbx) * BS;
        const int bh = min(BS, h - y0), bw = min(BS, w - x0);
        {
            const int r = tid >> 4, c = tid & 15;                   // outside the frame the block holds 0, and the window is masked to 0
            cur_s[tid] = (r < bh && c < bw) ? (S)min((unsigned)cur[(long)(y0 + r) * w + x0 + c], top) : (S)0;
        }
        for (int i = tid; i < wn * wn; i += 256) {
            const int r = i / wn, c = i - r * wn;
            const int yy = clampi(y0 + r - R, h - 1), xx = clampi(x0 + c - R, w - 1);
            win_s[r * (PW * SPD) + c] = (S)min((unsigned)prev[(long)yy * w + xx], top);
        }
        __syncthreads();
        const bool full = bh == BS && bw == BS;
        unsigned cm[ND];                                            // per dword of a block row: the samples inside the frame
#pragma unroll
        for (int k = 0; k < ND; ++k) {
            const int v = min(max(bw - k * SPD, 0), SPD);
            cm[k] = v == SPD ? 0xFFFFFFFFu : (1u << (v * 8 * (int)sizeof(S))) - 1u;
        }
        unsigned best = 0xFFFFFFFFu;
        int bdy = 0, bdx = 0;
        int dyi = (tid >> 2) / n, dxi = (tid >> 2) - dyi * n;       // dy + R, dx + R
        for (int it = tid; it < nitems; it += 256) {
            const unsigned* wrow = s_win + (rg * 4 + dyi) * PW + dxi / SPD;
            const unsigned* crow = s_cur + rg * 4 * ND;
            const unsigned shift = (unsigned)(dxi % SPD) * (unsigned)sizeof(S);
            unsigned s = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                unsigned wd[ND + 1];
#pragma unroll
                for (int k = 0; k <= ND; ++k) wd[k] = wrow[j * PW + k];
                const unsigned rowmask = rg * 4 + j < bh ? 0xFFFFFFFFu : 0u;
#pragma unroll
                for (int k = 0; k < ND; ++k) {
                    unsigned a = __builtin_amdgcn_alignbyte(wd[k + 1], wd[k], shift);
                    if (!full) a &= cm[k] & rowmask;
                    s = sad_packed<S>(a, crow[j * ND + k], s);
                }
            }
            s += __shfl_xor(s, 1);                                  // the four lanes of a candidate run together: nitems is a multiple of 4
            s += __shfl_xor(s, 2);
            const unsigned key = (s << 11) | s_rank[(dyi - R + MAXR) * NC + dxi - R + MAXR];
            if (key < best) {
                best = key;
                bdy = dyi - R;
                bdx = dxi - R;
            }
            if (dyi == R && dxi == R && rg == 0) s_sad0 = s;
            dxi += r64;
            dyi += q64;
            if (dxi >= n) {
                dxi -= n;
                ++dyi;
            }
        }
        unsigned m = best;
        for (int o = 32; o; o >>= 1) m = min(m, (unsigned)__shfl_xor(m, o));
        if ((tid & 63) == 0) s_red[tid >> 6] = m;
        __syncthreads();
        m = min(min(s_red[0], s_red[1]), min(s_red[2], s_red[3]));
        if (best == m && rg == 0) {                                 // ranks differ, so one candidate holds the key, and one of its lanes has rg 0
            const unsigned sv = m >> 11, s0 = s_sad0;
            if (mv) {
                mv[(row0 + blk) * 2] = (short)bdy;
                mv[(row0 + blk) * 2 + 1] = (short)bdx;
            }
            if (sad) {
                sad[(row0 + blk) * 2] = sv;
                sad[(row0 + blk) * 2 + 1] = s0;
            }
            acc[0] += sv;
            acc[1] += s0;
            acc[2] += (unsigned)(abs(bdy) + abs(bdx));
            acc[3] += (bdy | bdx) != 0;
        }
        // the next block's staging overwrites s_cur / s_win only after every thread has passed the barrier above, its s_red and s_sad0
        // only after the barrier that follows the staging
    }
    add_totals<4>(acc, s_acc, stats + (long)b * 4);
}

// grid (min(tiles of a frame, RESIDUAL_MAX_GRID), B); a tile is 64 x 16 pixels, four blocks of one block row
template <typename T>
__global__ __launch_bounds__(256) void residual_kernel(const T* __restrict__ frames, const T* __restrict__ frames_prev, const T* __restrict__ guide,
                                                       const T* __restrict__ guide_prev, const short* __restrict__ mv,
                                                       unsigned long long* __restrict__ stats, int h, int w, int nbx, int nby, int tiles_x,
                                                       int tiles, unsigned top) {
    __shared__ unsigned long long s_acc[4][5];
    const int tid = threadIdx.x, b = blockIdx.y;
    const long fs = (long)h * w + ((long)h * w >> 1);
    const T* f = frames + b * fs;
    const T* g = guide + b * fs;
    const T* fp = b ? f - fs : frames_prev;
    const T* gp = b ? g - fs : guide_prev;
    if (!fp) return;                                                // both NULL (the launcher refuses one of two): the row stays 0
    const int tx = tid & 63, ty = tid >> 6;
    unsigned long long acc[5] = {0, 0, 0, 0, 0};
    for (int t = blockIdx.x; t < tiles; t += gridDim.x) {
        const int by = t / tiles_x, x = (t - by * tiles_x) * 64 + tx;
        if (x >= w) continue;
        const short* m = mv + (((long)b * nby + by) * nbx + (x >> 4)) * 2;
        const int dy = m[0], dx = m[1];
        const int xx = clampi(x + dx, w - 1);
        unsigned p[5] = {0, 0, 0, 0, 0};                            // four pixels: at most 4 * 2046^2 < 2^25
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int y = by * BS + ty + 4 * j;
            if (y < h) {
                const long at = (long)y * w + x, pat = (long)clampi(y + dy, h - 1) * w + xx;
                const int rd = (int)min((unsigned)f[at], top) - (int)min((unsigned)fp[pat], top);
                const int rgd = (int)min((unsigned)g[at], top) - (int)min((unsigned)gp[pat], top);
                const int e = rd - rgd;
                p[0] += (unsigned)abs(rd);
                p[1] += (unsigned)(rd * rd);
                p[2] += (unsigned)abs(rgd);
                p[3] += (unsigned)(rgd * rgd);
                p[4] += (unsigned)(e * e);
            }
        }
#pragma unroll
        for (int k = 0; k < 5; ++k) acc[k] += p[k];
    }
    add_totals<5>(acc, s_acc, stats + (long)b * 5);
}

bool frames_ok(int B, int h, int w, int bits) {
    return B >= 1 && B < 65536 && h >= 2 && w >= 2 && h % 2 == 0 && w % 2 == 0 && (long)h * w < (1L << 30) && (bits == 8 || bits == 10);
}

template <typename T, typename S>
void launch_search(const void* guide, const void* guide_prev, short* mv, unsigned* sad, long* stats, int B, int h, int w, int radius, unsigned top,
                   hipStream_t s) {
    const int nbx = cdiv(w, BS), nblk = nbx * cdiv(h, BS);
    hipLaunchKernelGGL((search_kernel<T, S>), dim3((unsigned)(nblk < SEARCH_MAX_GRID ? nblk : SEARCH_MAX_GRID), (unsigned)B), dim3(256), 0, s, static_cast<const T*>(guide),
                       static_cast<const T*>(guide_prev), mv, sad, reinterpret_cast<unsigned long long*>(stats), h, w, nbx, nblk, radius, top);
}

template <typename T>
void launch_residual(const void* frames, const void* frames_prev, const void* guide, const void* guide_prev, const short* mv, long* stats, int B,
                     int h, int w, unsigned top, hipStream_t s) {
    const int nbx = cdiv(w, BS), nby = cdiv(h, BS), tiles_x = cdiv(w, 64), tiles = tiles_x * nby;
    hipLaunchKernelGGL((residual_kernel<T>), dim3((unsigned)(tiles < RESIDUAL_MAX_GRID ? tiles : RESIDUAL_MAX_GRID), (unsigned)B), dim3(256), 0, s,
                       static_cast<const T*>(frames), static_cast<const T*>(frames_prev), static_cast<const T*>(guide),
                       static_cast<const T*>(guide_prev), mv, reinterpret_cast<unsigned long long*>(stats), h, w, nbx, nby, tiles_x, tiles, top);
}

}  // namespace

extern "C" int fdn_motion_abi_version(void) { return FDN_MOTION_ABI_VERSION; }

extern "C" int fdn_motion_search(const void* guide, const void* guide_prev, short* mv, unsigned* sad, long* stats, int B, int h, int w, int bits,
                                 int radius, fdn_stream_t stream) {
    FDN_CHECK_ARG(guide && stats && frames_ok(B, h, w, bits) && radius >= 0 && radius <= MAXR);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (hipMemsetAsync(stats, 0, (size_t)B * 4 * sizeof(long), s) != hipSuccess) return FDN_ERR_LAUNCH;
    if (bits == 8) launch_search<uint8_t, uint8_t>(guide, guide_prev, mv, sad, stats, B, h, w, radius, 255u, s);
    else launch_search<uint16_t, uint16_t>(guide, guide_prev, mv, sad, stats, B, h, w, radius, 1023u, s);
    return fdn_launch_status();
}

extern "C" int fdn_motion_residual(const void* frames, const void* frames_prev, const void* guide, const void* guide_prev, const short* mv,
                                   long* stats, int B, int h, int w, int bits, fdn_stream_t stream) {
    FDN_CHECK_ARG(frames && guide && mv && stats && frames_ok(B, h, w, bits) && (frames_prev == nullptr) == (guide_prev == nullptr));
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (hipMemsetAsync(stats, 0, (size_t)B * 5 * sizeof(long), s) != hipSuccess) return FDN_ERR_LAUNCH;
    if (bits == 8) launch_residual<uint8_t>(frames, frames_prev, guide, guide_prev, mv, stats, B, h, w, 255u, s);
    else launch_residual<uint16_t>(frames, frames_prev, guide, guide_prev, mv, stats, B, h, w, 1023u, s);
    return fdn_launch_status();
}
