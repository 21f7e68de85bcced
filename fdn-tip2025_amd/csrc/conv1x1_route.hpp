// Which kernel fdn_conv1x1 runs for a descriptor: host arithmetic on the descriptor's integers and pointer VALUES (null-ness,
// alignment; nothing is dereferenced), no HIP call, no global.  fdn_conv1x1 launches what route_conv1x1 answers and
// fdn_conv1x1_route reports it, so the table below is the only place a shape is tied to a kernel; tests/test_host_cpu.py pins it
// (the shapes of the networks, the cases of the GPU tests, and a sweep in tests/conv1x1_routes.txt).
// The tile shapes and LDS sizes the decision depends on are defined here once, for the route and for the kernels' launchers.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/fdn_hip.h"

namespace c1x1 {

constexpr int KC = 32;                        // K chunk of every kernel (16 fp32 / 2 bf16 MFMA k-steps)
constexpr int TP = 128, TN = 128;             // pixel x channel tile of a workgroup of gemm_tile.hip / gemm_split.hip
constexpr int BLK = 3 * 2 * 2 * 128;          // split-bf16: 16-byte units of one operand chunk, [part][k-step][lane half][row]
constexpr int STRIP_MAX_N = 1024;             // widest output of the split-bf16 strip kernel (its bias lives in LDS)
constexpr int TRI_E = 10;                     // split-bf16 LN3_GATE: channels e per chunk (10 triples = 30 k + 2 zero columns)

inline long ceil_div(long a, long b) { return (a + b - 1) / b; }
inline int k_chunks(int K) { return (K + KC - 1) / KC; }
inline int n_tiles32(int N) { return (N + 31) / 32; }

// dynamic LDS of the small-K kernels, which keep the whole [K][N] weight matrix: gamma / beta tables and the transposed weights ...
inline size_t smallk_weight_lds(int nch, int N) {
    return (2UL * nch * KC + (size_t)nch * KC * (n_tiles32(N) * 32 + 1)) * sizeof(float);
}
inline size_t smallk_lds(int nch, int N) { return smallk_weight_lds(nch, N) + n_tiles32(N) * 32 * sizeof(float); }   // ... and the bias
// of the small-K kernels that stream the weights in 32-channel tiles (double buffered)
inline size_t smallk_stream_lds(int nch, int N) { return (2UL * nch * KC + 2UL * nch * KC * 33 + n_tiles32(N) * 32) * sizeof(float); }
// bytes of the packed split-bf16 weights (fdn_conv1x1_pack_bytes)
inline long split_pack_bytes(int N, int K, int ln3_E) {
    const long nch = ln3_E > 0 ? (ln3_E + TRI_E - 1) / TRI_E : k_chunks(K);
    return ceil_div(N, TN) * nch * BLK * 16;
}
// the strip kernel's direct-to-LDS form (strip2): whole 256-thread rounds per weight tile, and the packed weights behind one 2 GB descriptor
constexpr bool strip2_nks(int nks) { return (3 * nks * 2 * 32) % 256 == 0 && nks >= 6; }
// the generic kernel's 4-wave workgroups:
//  * measured (tools/gpu_gemm_shapes.py): 64-wide plain GEMMs (FDFFN project_out at level 2, 172 -> 64) gain from 4-wave workgroups at
//    3 waves per SIMD (13.5 -> 10.9 ms); wider tiles spill at that register budget
//  * wide tiles: two independent 4-wave workgroups per CU instead of one of 8 - their per-chunk barriers drift apart, so one
//    workgroup's MFMAs fill the other's load-issue / barrier phase (345 -> 128: 12.1 -> 11.3 ms); LN_MULADD spills at that budget
constexpr bool generic_nw4(int mt, int pro) {
    return pro == FDN_PRO_LN3_GATE ? mt >= 2 : ((mt == 2 && pro == FDN_PRO_NONE) || (mt >= 3 && pro != FDN_PRO_LN_MULADD));
}

}  // namespace c1x1

struct conv1x1_route {
    int status;                 // FDN_OK, FDN_ERR_ARG or FDN_ERR_UNSUPPORTED (then form = FDN_CONV1X1_REFUSED and the rest is 0)
    int form;                   // FDN_CONV1X1_* of include/fdn_hip.h: one per launcher template
    int n;                      // the form's first template parameter: MT (GENERIC, KSTREAM_VEC), NKS (SPLIT_STRIP), NCH (small-K forms), else 0
    int pro;                    // the PRO the kernel is instantiated for
    int nw, early;              // GENERIC: waves per workgroup, epilogue operands fetched ahead of the MFMAs
    int xbf, obf;               // bf16 storage of the input / of the output
    int strip2;                 // SPLIT_STRIP: the direct-to-LDS form
    int own_stats;              // the kernel takes the LayerNorm statistics itself when d.stats is null
    int bf16_pipe;              // the launch counts in fdn_bf16_mfma_launches
    int threads, tile_px;       // threads per workgroup, pixels per tile
};

namespace c1x1 {

// 8- / 16-byte lanes: P and the batch strides in whole 16-byte units, x, out and the operands the form reads or writes besides
// (p2, p3: null = none) 16-byte aligned
inline bool vec_aligned(const fdn_conv1x1_desc& d, const void* p2 = nullptr, const void* p3 = nullptr) {
    if (d.P % 4 != 0 || d.xbs[0] % 4 != 0 || d.obs % 4 != 0) return false;
    const uintptr_t a = reinterpret_cast<uintptr_t>(d.x[0]) | reinterpret_cast<uintptr_t>(d.out) | reinterpret_cast<uintptr_t>(p2) | reinterpret_cast<uintptr_t>(p3);
    return (a & 15) == 0;
}
// the vectorised project_out forms: residual or no epilogue operand, statistics allowed
inline bool vec_out_ok(const fdn_conv1x1_desc& d) {
    if (d.epi != FDN_EPI_NONE && d.epi != FDN_EPI_RES) return false;
    if (d.epi == FDN_EPI_RES && d.rbs % 4 != 0) return false;
    return vec_aligned(d, d.epi == FDN_EPI_RES ? d.res : nullptr, d.stats_out);
}
// the vectorised kernel covers: small-K shapes (see smallk_ok) with one segment, no epilogue operand, plain / LN prologue,
// P a multiple of 4 and 16-byte aligned tensors
inline bool smallk_vec_ok(const fdn_conv1x1_desc& d) {
    if (d.kseg[1] > 0 || d.kseg[2] > 0 || d.epi != FDN_EPI_NONE || (d.pro != FDN_PRO_NONE && d.pro != FDN_PRO_LN)) return false;
    return vec_aligned(d, d.pro != FDN_PRO_NONE ? d.stats : nullptr);
}
// plain deep-K convs for the 8-byte-lane K-streaming kernel
inline bool kstream_vec_ok(const fdn_conv1x1_desc& d) {
    if (d.pro != FDN_PRO_NONE || d.kseg[1] > 0 || d.kseg[2] > 0 || d.K <= 96 || d.N > 96) return false;   // (N = 128 spills: slower)
    return vec_out_ok(d);                          // measured: 172 -> 64 at level 2 10.2 -> 7.0 ms (71 TFLOP/s)
}
// K <= 128, N >= 2K, single input segment, plain/LN prologue, no muladd epilogue, weights too big for LDS
inline bool smallk_stream_ok(const fdn_conv1x1_desc& d) {
    if (d.K > 128 || d.K <= 64 || d.stats_out || d.kseg[1] > 0) return false;
    if (d.pro != FDN_PRO_NONE && d.pro != FDN_PRO_LN) return false;
    if (d.epi == FDN_EPI_MULADD) return false;
    return d.N >= 2 * d.K;
}
// narrow project_out convs for the vectorised kernel's TAIL form: K <= 96, N <= 32, no prologue, residual or no
// epilogue operand, statistics allowed
inline bool narrow_vec_ok(const fdn_conv1x1_desc& d) {
    if (d.K > 96 || d.N > 32 || d.pro != FDN_PRO_NONE || d.kseg[1] > 0 || d.kseg[2] > 0) return false;
    return vec_out_ok(d);
}
// true when the small-K kernel covers this problem
inline bool smallk_ok(const fdn_conv1x1_desc& d) {
    if (d.K > 64 || d.stats_out || d.pro == FDN_PRO_LN3_GATE) return false;
    if (d.N < 2 * d.K || d.N < 64) return false;                  // made for N >> K
    return smallk_weight_lds(k_chunks(d.K), d.N) <= 100 * 1024;
}
inline int pick_mt(int N) {
    // fewest computed 32-row tiles, then fewest passes; MT <= 5 keeps the accumulator at 80 VGPRs
    const int tiles = n_tiles32(N);
    int best = 1, best_cost = 1 << 30;
    for (int mt = 1; mt <= 5; ++mt) {
        const int passes = (tiles + mt - 1) / mt;
        const int cost = passes * mt * 100 + passes;
        if (cost < best_cost || (cost == best_cost && mt > best)) { best_cost = cost; best = mt; }
    }
    return best;
}

inline conv1x1_route refused(int status) {
    conv1x1_route r = {};
    r.status = status;
    return r;
}
inline conv1x1_route taken(int form, int n, int pro, int threads, int tile_px) {
    conv1x1_route r = {};
    r.form = form; r.n = n; r.pro = pro; r.threads = threads; r.tile_px = tile_px;
    return r;
}

// gemm_split.hip: the deep shapes and the wide project_in convs on the bf16 matrix pipe (split operands), when the caller supplies
// packed weights.  FDN_CONV1X1_REFUSED = not a shape of these kernels (another form is picked)
inline conv1x1_route split_route(const fdn_conv1x1_desc& d, bool pipe_f32) {
    const conv1x1_route no = refused(FDN_ERR_UNSUPPORTED);
    if (pipe_f32) return no;
    // lanes past the pixel count are masked with a byte offset of 2^31: it must stay outside every descriptor of this kernel
    if ((unsigned long long)(d.N > d.K ? d.N : d.K) * 4ull * (unsigned long long)d.P > 0x7FFFFFFFull) return no;
    if (!d.wpk || d.kseg[2] > 0 || d.act != FDN_ACT_NONE || d.x_bf16 || d.out_bf16) return no;
    const bool two = d.kseg[1] > 0;                       // two inputs: the K-streaming kernel only, plain prologue, whole chunks per input
    if (two && (d.pro != FDN_PRO_NONE || d.kseg[0] % KC != 0 || d.K < 96 || d.N < 96)) return no;
    if ((long)d.B * ceil_div(d.P, TP) * ceil_div(d.N, TN) > 0x7FFFFFFFL) return no;
    // short K, wide N, no epilogue: the activation strip stays in registers and the weights stream
    const bool strip = !two && d.N <= STRIP_MAX_N && d.epi == FDN_EPI_NONE && !d.stats_out && (d.pro == FDN_PRO_NONE || d.pro == FDN_PRO_LN);
    int nks = 0;
    // the project_in convs of levels 1-2 as well (32 -> 86, 64 -> 172; FDN_lolv1 24 -> 64, 48 -> 129): on the fp32 MFMA they kept
    // the vector ALU's datapath 60-90 % busy (64 -> 172: 0.49 -> 0.41 ms, 32 -> 86: 0.82 -> 0.75 ms here)
    if (strip && d.K > 16 && d.K <= 64 && 2 * d.N >= 5 * d.K) nks = d.K > 48 ? 4 : d.K > 32 ? 3 : 2;
    else if (d.K < 96 || d.N < 96 || (d.stats_out && d.N > TN)) return no;
    else if (d.K <= 128 && d.N >= 256 && strip) nks = d.K > 112 ? 8 : d.K > 96 ? 7 : 6;          // (K = 96: FDN_lolv1)
    conv1x1_route r;
    if (nks) {
        r = taken(FDN_CONV1X1_SPLIT_STRIP, nks, d.pro, 256, TP);
        r.strip2 = strip2_nks(nks) && split_pack_bytes(d.N, d.K, 0) < 0x7FFFFFFFL;
    } else {
        if (d.pro < FDN_PRO_NONE || d.pro > FDN_PRO_LN_MULADD) return no;
        r = taken(FDN_CONV1X1_SPLIT, 0, d.pro, 256, TP);
        r.own_stats = d.pro == FDN_PRO_LN3_GATE || d.pro == FDN_PRO_LN_MULADD;
    }
    r.bf16_pipe = 1;
    return r;
}

// gemm_tile.hip: 459 -> 128 (LN3 * v_value), 345 -> 128, 128 -> 128 at level 3
inline conv1x1_route tile_route(const fdn_conv1x1_desc& d) {
    const conv1x1_route no = refused(FDN_ERR_UNSUPPORTED);
    if (d.N > TN || d.N < 96 || d.K < 96 || d.kseg[1] > 0 || d.kseg[2] > 0 || d.act != FDN_ACT_NONE || d.x_bf16 || d.out_bf16) return no;
    if (d.epi != FDN_EPI_NONE && d.epi != FDN_EPI_RES) return no;
    if ((long)d.B * ceil_div(d.P, TP) > 0x7FFFFFFFL) return no;
    if (d.pro != FDN_PRO_NONE && d.pro != FDN_PRO_LN3_GATE) return no;
    return taken(FDN_CONV1X1_TILE, 0, d.pro, 256, TP);
}

// The pixel-pair forms (8-byte lanes, 256 pixels per 4-wave tile), for fp32 and for bf16 storage of the one operand the form allows
inline conv1x1_route kstream_route(const fdn_conv1x1_desc& d) {
    const int tiles = n_tiles32(d.N);
    conv1x1_route r = taken(FDN_CONV1X1_KSTREAM_VEC, tiles < 3 ? tiles : 3, FDN_PRO_NONE, 256, 4 * 32 * 2);
    r.xbf = d.x_bf16 != 0;
    return r;
}
inline conv1x1_route narrow_route(const fdn_conv1x1_desc& d) {
    conv1x1_route r = taken(FDN_CONV1X1_NARROW_TAIL, d.K <= KC ? 1 : d.K <= 2 * KC ? 2 : 3, FDN_PRO_NONE, 256, 4 * 32 * 2);
    r.xbf = d.x_bf16 != 0;
    return r;
}
// measured (tools/bench_kernels.py to_hidden ffn_in, B=8 720p): 8-byte lanes win for K <= 32 (32->152: 1.65 -> 1.44 ms,
// 32->86: 0.92 -> 0.76 ms) and for K <= 64 while the weight matrix leaves room for 3 workgroups per CU (64->172:
// 0.74 -> 0.59 ms; 64->304 is slower vectorised: refused = not taken); 16-byte lanes spill with the LN prologue
inline conv1x1_route smallk_vec_route(const fdn_conv1x1_desc& d) {
    int nch;
    if (d.K <= KC) nch = 1;                    // (8-byte lanes only: the kernel static_asserts VEC == 2; 16-byte lanes measure the same with LN)
    else if (smallk_weight_lds(2, d.N) <= 52 * 1024) nch = 2;
    else return refused(FDN_ERR_UNSUPPORTED);
    conv1x1_route r = taken(FDN_CONV1X1_SMALLK_VEC, nch, d.pro, 256, 4 * 32 * 2);
    r.obf = d.out_bf16 != 0;
    return r;
}

}  // namespace c1x1

inline conv1x1_route route_conv1x1(const fdn_conv1x1_desc& d, bool pipe_f32) {
    using namespace c1x1;
#define C1X1_CHECK_ARG(cond) \
    if (!(cond)) return refused(FDN_ERR_ARG)
    C1X1_CHECK_ARG(d.B > 0 && d.K > 0 && d.N > 0 && d.P > 0);
    C1X1_CHECK_ARG(d.x[0] && d.w && d.out);
    C1X1_CHECK_ARG(d.kseg[0] + d.kseg[1] + d.kseg[2] == d.K);
    C1X1_CHECK_ARG(d.kseg[1] == 0 || d.x[1]);
    C1X1_CHECK_ARG(d.kseg[2] == 0 || d.x[2]);
    // stats == NULL with a LayerNorm prologue: the K-streaming split-bf16 kernel takes the statistics itself (LN3_GATE / LN_MULADD with packed
    // weights on a deep shape); every other kernel wants them from fdn_chan_stats or a producer's epilogue
    const bool own_stats = d.pro != FDN_PRO_NONE && !d.stats;
    if (own_stats) C1X1_CHECK_ARG(d.pro == FDN_PRO_LN3_GATE || d.pro == FDN_PRO_LN_MULADD);
    if (d.pro >= FDN_PRO_LN3_GATE) C1X1_CHECK_ARG(d.gamma && d.beta);
    if (d.pro == FDN_PRO_LN3_GATE) C1X1_CHECK_ARG(d.xb && d.ln_group * 3 == d.K && d.kseg[0] == d.K);
    if (d.pro == FDN_PRO_LN_MULADD) C1X1_CHECK_ARG(d.xb);
    if (d.epi == FDN_EPI_RES) C1X1_CHECK_ARG(d.res);
    if (d.epi == FDN_EPI_MULADD) C1X1_CHECK_ARG(d.mul && d.add);
    if (d.stats_out) C1X1_CHECK_ARG(d.N <= 160);
#undef C1X1_CHECK_ARG
    const conv1x1_route no = refused(FDN_ERR_UNSUPPORTED);
    // 32-bit buffer offsets: every per-image plane set must stay below 4 GiB (incl. the padded K / N tails)
    const unsigned long long lim = 0xFFFFFFFFull, P4 = 4ull * d.P;
    if ((unsigned long long)(d.K + 40) * P4 > lim || (unsigned long long)(d.N + 200) * P4 > lim) return no;
    if (d.kseg[1] > 0 && ((d.kseg[0] & 1) || (d.kseg[1] & 1))) return no;   // k-step pairs must not straddle segments
    // bf16 STORAGE of one operand (the block-internal FDFFN tensors of levels 1-2): the pixel-pair kernels only -
    //   x_bf16  : the project_out convs (narrow TAIL form / K-streaming form), fp32 result;
    //   out_bf16: the project_in convs (small-K form, plain or LayerNorm prologue), fp32 input.
    if (d.x_bf16 || d.out_bf16) {
        if ((d.x_bf16 && d.out_bf16) || own_stats) return no;
        if (d.x_bf16) return kstream_vec_ok(d) ? kstream_route(d) : narrow_vec_ok(d) ? narrow_route(d) : no;
        return smallk_ok(d) && smallk_vec_ok(d) ? smallk_vec_route(d) : no;
    }
    // level 3 with packed weights: fp32 on the bf16 matrix pipe
    if (const conv1x1_route r = split_route(d, pipe_f32); r.form) return r;
    if (own_stats) return no;
    if (const conv1x1_route r = tile_route(d); r.form) return r;
    const int nch = k_chunks(d.K);
    // K = 64 with a weight matrix too big to sit in LDS three times per CU (level-2 to_hidden, 64 -> 304): stream the weights too (15.1 -> 12.4 ms)
    if (nch == 2 && d.N >= 256 && !d.stats_out && smallk_vec_ok(d)) return taken(FDN_CONV1X1_SMALLK_STREAM_VEC, 2, d.pro, 512, 8 * 32 * 2);
    if (smallk_stream_ok(d)) {                                    // (K in 65 .. 128: three or four chunks)
        const int pro = d.pro == FDN_PRO_LN ? FDN_PRO_LN : FDN_PRO_NONE;
        if (smallk_vec_ok(d)) return taken(FDN_CONV1X1_SMALLK_STREAM_VEC, nch == 3 ? 3 : 4, pro, 512, 8 * 32 * 2);   // 128->612: 21.3 -> 20.0 ms, 128->345: 13.1 -> 10.9 ms
        return taken(FDN_CONV1X1_SMALLK_STREAM, nch == 3 ? 3 : 4, pro, 512, 8 * 32);
    }
    if (kstream_vec_ok(d)) return kstream_route(d);
    if (narrow_vec_ok(d)) return narrow_route(d);
    if (smallk_ok(d)) {
        if (smallk_vec_ok(d)) {
            if (const conv1x1_route r = smallk_vec_route(d); r.form) return r;      // (K > 32 with a wide weight matrix: the dword form below)
        }
        const int pro = d.pro == FDN_PRO_NONE || d.pro == FDN_PRO_LN ? d.pro : FDN_PRO_LN_MULADD;
        return taken(FDN_CONV1X1_SMALLK, nch == 1 ? 1 : 2, pro, 512, 8 * 32);
    }
    if (d.pro < FDN_PRO_NONE || d.pro > FDN_PRO_LN_MULADD) return refused(FDN_ERR_ARG);
    const int mt = pick_mt(d.N);
    conv1x1_route r = taken(FDN_CONV1X1_GENERIC, mt, d.pro, 0, 0);
    // narrow, shallow problems with an epilogue operand are load-latency bound: 4-wave workgroups (finer register
    // granularity per CU) that fetch the epilogue operands ahead of the MFMAs
    r.early = d.pro != FDN_PRO_LN3_GATE && mt <= 2 && d.epi != FDN_EPI_NONE && d.K <= 64;
    r.nw = r.early || generic_nw4(mt, d.pro) ? 4 : 8;
    r.threads = r.nw * 64;
    r.tile_px = r.nw * 32;
    return r;
}
