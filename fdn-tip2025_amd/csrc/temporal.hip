// Video across frames (include/fdn_temporal.h; no reference counterpart, the reference reads PNGs): the ratio FDN is fed, kept steady
// from one frame of a stream to the next.
//   fdn_luma_hist    : codec frames -> one 256-bin luma histogram per frame.  HBM-bound, 1 - 2 B per pixel, integer and therefore exact
//   fdn_ratio_smooth : histograms + LPNet's ratios + the carried state -> filtered ratios, scene-cut flags, the state advanced; one
//                      small launch in frame order
// Both run on the stream the frames and the ratio are already on: nothing goes to the host between LPNet and FDN.
#include "common.hpp"

#include "../../include/fdn_temporal.h"

namespace {

constexpr int HIST_THREADS = 256, HIST_WAVES = HIST_THREADS / 64;
constexpr int HIST_VECS_PER_THREAD = 4;                              // 16-byte loads a thread makes when the grid is not capped
constexpr int HIST_MAX_BLOCKS = 4096;                                // per frame

template <typename T>
__device__ __forceinline__ unsigned luma_bin(unsigned code);
template <>
__device__ __forceinline__ unsigned luma_bin<unsigned char>(unsigned code) { return code; }
template <>
__device__ __forceinline__ unsigned luma_bin<unsigned short>(unsigned code) { return min(code, 1023u) >> 2; }   // above 1023 counts as 1023

// the bins of the samples of one 32-bit word, in memory order
template <typename T>
__device__ __forceinline__ void word_bins(unsigned word, unsigned (&bin)[4 / sizeof(T)]) {
    if constexpr (sizeof(T) == 1) {
#pragma unroll
        for (int j = 0; j < 4; ++j) bin[j] = (word >> (8 * j)) & 0xFFu;
    } else {
        bin[0] = luma_bin<T>(word & 0xFFFFu);
        bin[1] = luma_bin<T>(word >> 16);
    }
}

// Workgroup (x, b) walks 16-byte vectors x * 256 + tid, + gridDim.x * 256, ... of frame b's luma plane and counts into a sub-histogram
// that each of its four waves keeps for itself in LDS: a dark frame puts nearly all samples into a handful of bins, and one shared
// histogram would serialise all 256 threads on them.  Within a vector a run of equal bins becomes one add of its length (a flat region
// costs one LDS atomic per 16 bytes instead of 8 or 16).  A frame starts at b * h * w * 3 / 2 samples, which is in general only
// sample-aligned: the samples before the first 16-byte boundary and those after the last whole vector are counted one by one by the
// frame's workgroup 0.  The four sub-histograms are summed and added to the frame's 256 words (cleared by the entry point) with one
// vector atomic per non-zero bin.
template <typename T>
__global__ __launch_bounds__(HIST_THREADS) void luma_hist_kernel(const T* __restrict__ frames, unsigned* __restrict__ hist, long n) {
    constexpr int VS = 16 / sizeof(T), WS = 4 / sizeof(T);          // samples per vector, per word
    __shared__ unsigned sub[HIST_WAVES][256];
    const int tid = threadIdx.x, b = blockIdx.y;
    unsigned* mine = sub[tid >> 6];
#pragma unroll
    for (int k = 0; k < HIST_WAVES; ++k) sub[k][tid] = 0;
    __syncthreads();
    const T* f = frames + (long)b * (n + (n >> 1));
    const uintptr_t addr = reinterpret_cast<uintptr_t>(f);
    // samples before the first 16-byte boundary; a pointer that is not even sample-aligned never reaches one: all of the plane
    const long head = (addr % sizeof(T)) ? n : min(n, (long)(((0 - addr) & 15u) / sizeof(T)));
    const long nvec = (n - head) / VS;
    const fdn_u32x4* v = reinterpret_cast<const fdn_u32x4*>(f + head);
    const long step = (long)gridDim.x * HIST_THREADS;
    for (long i = (long)blockIdx.x * HIST_THREADS + tid; i < nvec; i += step) {
        const fdn_u32x4 q = v[i];
        const unsigned words[4] = {q.x, q.y, q.z, q.w};
        unsigned cur = 0, cnt = 0;                                   // the run of equal bins so far
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            unsigned bin[WS];
            word_bins<T>(words[k], bin);
#pragma unroll
            for (int j = 0; j < WS; ++j) {
                if (bin[j] != cur && cnt) {
                    atomicAdd(&mine[cur], cnt);
                    cnt = 0;
                }
                cur = bin[j];
                ++cnt;
            }
        }
        atomicAdd(&mine[cur], cnt);
    }
    if (blockIdx.x == 0) {
        const long tail = head + nvec * VS, left = head + (n - tail);
        for (long i = tid; i < left; i += HIST_THREADS) {
            const long s = i < head ? i : tail + (i - head);        // < n
            atomicAdd(&mine[luma_bin<T>(f[s])], 1u);
        }
    }
    __syncthreads();
    unsigned total = 0;
#pragma unroll
    for (int k = 0; k < HIST_WAVES; ++k) total += sub[k][tid];
    if (total) atomicAdd(&hist[(long)b * 256 + tid], total);
}

// One workgroup of four waves.  First every wave takes frames t = wave, wave + 4, ...: a lane holds four bins of frame t and of the
// frame before it (the state's for t = 0), the wave sums |difference| and writes dist[t] and cut[t].  Then one thread walks the frames in
// order - the filter is a recurrence - and last the state takes the histogram of frame B - 1.
__global__ __launch_bounds__(256) void ratio_smooth_kernel(const unsigned* __restrict__ hist, const float* ratio, unsigned* __restrict__ state,
                                                           float alpha, unsigned cut_above, int B, float* ratio_out,
                                                           unsigned* __restrict__ dist, int* __restrict__ cut) {
#pragma clang fp contract(off)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned flags = state[257];
    for (int t = wave; t < B; t += 4) {
        const unsigned* cur = hist + (long)t * 256;
        const unsigned* prev = t ? cur - 256 : state;
        const bool has_prev = t > 0 || (flags & 1u);
        unsigned d = 0;
        if (has_prev) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const unsigned a = cur[lane + 64 * k], p = prev[lane + 64 * k];
                d += a > p ? a - p : p - a;                          // the sum is at most 2 h w < 2^31
            }
        }
#pragma unroll
        for (int off = 32; off; off >>= 1) d += __shfl_xor(d, off);
        if (lane == 0) {
            dist[t] = d;
            cut[t] = (!has_prev || d > cut_above) ? 1 : 0;
        }
    }
    __syncthreads();                                                 // dist / cut are written, the state's histogram has been read
    if (tid == 0) {
        bool has_ratio = flags & 2u;
        float prev = __uint_as_float(state[256]);
        for (int t = 0; t < B; ++t) {
            const float r = ratio[t];
            float o = r;
            if (!cut[t] && has_ratio && alpha != 1.0f && __builtin_isfinite(r)) {
                const float diff = r - prev;                         // three operations, each rounded once
                const float move = alpha * diff;
                o = prev + move;
            }
            ratio_out[t] = o;
            if (__builtin_isfinite(o)) {                             // a non-finite value is handed out and forgotten
                prev = o;
                has_ratio = true;
            }
        }
        if (has_ratio) state[256] = __float_as_uint(prev);
        state[257] = 1u | (has_ratio ? 2u : 0u);
    }
    state[tid] = hist[(long)(B - 1) * 256 + tid];
}

}  // namespace

extern "C" int fdn_temporal_abi_version(void) { return FDN_TEMPORAL_ABI_VERSION; }

extern "C" int fdn_luma_hist(const void* frames, unsigned* hist, int B, int h, int w, int bits, fdn_stream_t stream) {
    FDN_CHECK_ARG(frames && hist && B > 0 && B < 65536 && h >= 2 && w >= 2 && h % 2 == 0 && w % 2 == 0 && (bits == 8 || bits == 10));
    const long n = (long)h * w;
    FDN_CHECK_ARG(n < (1L << 30));
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (hipMemsetAsync(hist, 0, (size_t)B * 256 * sizeof(unsigned), s) != hipSuccess) return FDN_ERR_LAUNCH;
    const long vecs = n / (bits == 8 ? 16 : 8);
    const dim3 grid(max(1, min(cdiv(vecs, (long)HIST_THREADS * HIST_VECS_PER_THREAD), HIST_MAX_BLOCKS)), B);
    if (bits == 8)
        hipLaunchKernelGGL(luma_hist_kernel<unsigned char>, grid, dim3(HIST_THREADS), 0, s, static_cast<const unsigned char*>(frames), hist, n);
    else
        hipLaunchKernelGGL(luma_hist_kernel<unsigned short>, grid, dim3(HIST_THREADS), 0, s, static_cast<const unsigned short*>(frames), hist, n);
    return fdn_launch_status();
}

extern "C" int fdn_ratio_smooth(const unsigned* hist, const float* ratio, unsigned* state, float alpha, int cut_above, int B,
                                float* ratio_out, unsigned* dist, int* cut, fdn_stream_t stream) {
    FDN_CHECK_ARG(hist && ratio && state && ratio_out && dist && cut && B > 0 && B < 65536);
    FDN_CHECK_ARG(alpha > 0.f && alpha <= 1.f && cut_above >= 0);   // a NaN alpha fails both comparisons
    hipLaunchKernelGGL(ratio_smooth_kernel, dim3(1), dim3(256), 0, static_cast<hipStream_t>(stream), hist, ratio, state, alpha,
                       (unsigned)cut_above, B, ratio_out, dist, cut);
    return fdn_launch_status();
}
