// Host planning of the full-image FFTs: which kernel a length runs on (Route), its radices, and the twiddle tables on the device.
// Host code only; included by fft2d.hip after its kernels, whose kernel-visible declarations it reads (Plan, Rader, ColPlan,
// RowPlan, NT, EMAX, MAX_STAGES).
#pragma once
#include <math.h>

#include <map>
#include <mutex>
#include <type_traits>
#include <vector>

namespace {

template <int V> using IC = std::integral_constant<int, V>;

// Run time value -> template argument: calls f(IC<V>{}) for the one V of Vs that equals v.  The launch sites name the
// instantiations that exist; a value outside the list launches nothing.
template <int... Vs, typename F>
int dispatch(int v, F&& f) {
    int e = FDN_ERR_UNSUPPORTED;
    (void)((v == Vs && ((e = f(IC<Vs>{})), true)) || ...);
    return e;
}

// ------------------------------------------------------------------------------------------
// The compile-time plans.  A plan is added here, in one line (and in PLANNED_H / PLANNED_W of tests/common.py): the length
// lookup, the routes, the launches of every mode and fdn_fft_prepare are generated from these two lists.
//   columns, H = R * P: 23 * {32, 16, 8} (720p pyramid), 17 * {32, 16, 8} (1080p levels 2, 3 and 544-row inputs), 34 * 32
//     (1088 rows: 1080p level 1), and the shapes the reference's own drivers feed: LOL-Blur frames 640 x 1120
//     (inference_fdn_lolblur.py:16-17, already x32) and LOL-v1 400 x 600 padded to 416 x 608 (inference_fdn_lolv1.py:52-64)
//   rows, W = 2 * R1 * P: 20 (720p) and 30 (1080p) x {32, 16, 8}; LOL-v1 padded 608 / 304 (152 = 2 x 19 x 4 stays generic);
//     LOL-Blur 1120 / 560 / 280
// ------------------------------------------------------------------------------------------
#define FDN_COL_PLANS(X) \
    X(23, 32) X(23, 16) X(23, 8) X(17, 32) X(17, 16) X(17, 8) X(34, 32) X(20, 32) X(20, 16) X(20, 8) X(13, 32) X(13, 16) X(13, 8)
#define FDN_ROW_PLANS(X) \
    X(20, 32) X(20, 16) X(20, 8) X(30, 32) X(30, 16) X(30, 8) X(19, 16) X(19, 8) X(35, 16) X(35, 8) X(35, 4)

// The FDN_* code f(IC<R>{}, IC<P>{}) returns for the plan of column length H / row width W; FDN_ERR_UNSUPPORTED (f not
// called) for a length without one
template <typename F>
int col_plan(int H, F&& f) {
#define X(R, P) if (H == R * P) return f(IC<R>{}, IC<P>{});
    FDN_COL_PLANS(X)
#undef X
    return FDN_ERR_UNSUPPORTED;
}
template <typename F>
int row_plan(int W, F&& f) {
#define X(R1, P) if (W == 2 * R1 * P) return f(IC<R1>{}, IC<P>{});
    FDN_ROW_PLANS(X)
#undef X
    return FDN_ERR_UNSUPPORTED;
}

// ------------------------------------------------------------------------------------------
// twiddle tables: immutable, built on first use per (device, table)
// ------------------------------------------------------------------------------------------
// e^{-2 pi i t / N}, exact on the axes (so DC / Nyquist bins of real data stay exactly real); "+0" keeps zeros positive
float2 root_of_unity(long t, long N) {
    t %= N;
    double c, s;
    if ((4 * t) % N == 0) {
        const int q = (int)((4 * t) / N);             // quarter turns
        c = (q == 0) ? 1.0 : (q == 2 ? -1.0 : 0.0);
        s = (q == 1) ? 1.0 : (q == 3 ? -1.0 : 0.0);
    } else {
        const double a = 2.0 * M_PI * (double)t / (double)N;
        c = cos(a);
        s = sin(a);
    }
    float2 w = make_float2((float)c, (float)(-s) + 0.0f);
    if (w.y == 0.0f) w.y = 0.0f;
    if (w.x == 0.0f) w.x = 0.0f;
    return w;
}

template <typename T>
const T* upload(const std::vector<T>& h) {
    T* d = nullptr;
    if (hipMalloc(&d, sizeof(T) * h.size()) != hipSuccess) return nullptr;
    if (hipMemcpy(d, h.data(), sizeof(T) * h.size(), hipMemcpyHostToDevice) != hipSuccess) return nullptr;
    return d;
}

enum { TAB_N, TAB_COLS_RP, TAB_ROWS_RP };
std::mutex g_mu;
std::map<std::pair<int, int>, const float2*> g_tables;   // (device, table id) -> device table

// the table (kind, a, b) of the current device: a = N, or (a, b) = (R, P) with P <= 32; fill(h) writes its values on first use
template <typename Fill>
const float2* cached_table(int kind, int a, int b, Fill&& fill) {
    int devid = 0;
    if (hipGetDevice(&devid) != hipSuccess) return nullptr;
    std::lock_guard<std::mutex> lk(g_mu);
    const int id = (a * 64 + b) * 4 + kind;
    auto it = g_tables.find({devid, id});
    if (it != g_tables.end()) return it->second;
    std::vector<float2> h;
    fill(h);
    const float2* d = upload(h);
    if (d) g_tables[{devid, id}] = d;
    return d;
}

// W_N^t, t in [0, N)
const float2* get_table(int N) {
    return cached_table(TAB_N, N, 0, [&](std::vector<float2>& h) {
        for (int t = 0; t < N; ++t) h.push_back(root_of_unity(t, N));
    });
}

// transposed twiddles of the R x P split of the planned columns: tab[n2 * R + k1] = W_H^{n2 k1}
const float2* get_table_rp(int R, int P) {
    return cached_table(TAB_COLS_RP, R, P, [&](std::vector<float2>& h) {
        for (int n2 = 0; n2 < P; ++n2)
            for (int k1 = 0; k1 < R; ++k1) h.push_back(root_of_unity((long)n2 * k1, (long)R * P));
    });
}

// planned rows: [ (P-1) * R1 transposed twiddles W_M^{n2 k1} | M + 1 split twiddles W_W^k ]
const float2* get_table_rows_rp(int R1, int P) {
    return cached_table(TAB_ROWS_RP, R1, P, [&](std::vector<float2>& h) {
        const int M = R1 * P;
        for (int n2 = 1; n2 < P; ++n2)
            for (int k1 = 0; k1 < R1; ++k1) h.push_back(root_of_unity((long)n2 * k1, M));
        for (int k = 0; k <= M; ++k) h.push_back(root_of_unity(k, 2 * M));
    });
}

// ------------------------------------------------------------------------------------------
// generic plans: the radix decomposition of a length
// ------------------------------------------------------------------------------------------
// the radix decomposition alone (host arithmetic, no table): what make_plan runs and what fdn_fft_route reports
bool plan_radices(int N, Plan* p) {
    p->N = N;
    p->nst = 0;
    p->tw = nullptr;
    p->tab_mul = 0;
    int n = N;
    auto push = [&](int r) { if (p->nst < MAX_STAGES) p->radix[p->nst++] = r; };
    int n2 = n, odd[MAX_STAGES], nodd = 0;
    while (n2 % 2 == 0) n2 /= 2;
    for (int f = 3; (long)f * f <= n2; f += 2)
        while (n2 % f == 0) { if (nodd < MAX_STAGES) odd[nodd++] = f; n2 /= f; }
    if (n2 > 1 && nodd < MAX_STAGES) odd[nodd++] = n2;
    for (int i = nodd - 1; i >= 0; --i) { push(odd[i]); n /= odd[i]; }     // largest odd prime first
    while (n % 4 == 0) { push(4); n /= 4; }
    while (n % 2 == 0) { push(2); n /= 2; }
    int prod = 1;
    for (int i = 0; i < p->nst; ++i) prod *= p->radix[i];
    return prod == N;
}

bool make_plan(int N, int tabN, Plan* p) {
    if (!plan_radices(N, p) || tabN % N != 0) return false;
    p->tw = get_table(tabN);
    p->tab_mul = tabN / N;
    return p->tw != nullptr;
}

// ------------------------------------------------------------------------------------------
// Rader's host set-up (struct Rader, fft2d.hip)
// ------------------------------------------------------------------------------------------
std::map<std::pair<int, int>, Rader> g_rader;

bool is_prime(int n) {
    if (n < 2) return false;
    for (int f = 2; (long)f * f <= n; ++f)
        if (n % f == 0) return false;
    return true;
}

// radices with a register butterfly at every BIG >= 1 tier of fft_pass and a case in fft_run_inplace: the in-place column passes and
// the Rader sub-transforms take only these
bool reg_radix(int R) { return R == 2 || R == 3 || R == 4 || R == 5 || R == 7 || R == 17 || R == 23; }

// Rader applies to p: a prime >= 29 whose p-1 factors into reg_radix radices (sub = that plan's radices, no table)
bool rader_ok(int p, Plan* sub) {
    if (p < 29 || !is_prime(p) || !plan_radices(p - 1, sub)) return false;
    for (int i = 0; i < sub->nst; ++i)
        if (!reg_radix(sub->radix[i])) return false;
    return true;
}

// returns false when p is not prime / p-1 needs a radix without a register butterfly (caller keeps the gather pass)
bool get_rader(int p, Rader* out) {
    int devid = 0;
    if (hipGetDevice(&devid) != hipSuccess) return false;
    {
        std::lock_guard<std::mutex> lk(g_mu);
        auto it = g_rader.find({devid, p});
        if (it != g_rader.end()) { *out = it->second; return out->p != 0; }
    }
    Rader r = {};
    auto fail = [&]() { std::lock_guard<std::mutex> lk(g_mu); g_rader[{devid, p}] = Rader{}; return false; };
    if (!rader_ok(p, &r.sub)) return fail();
    const int n = p - 1;
    if (!make_plan(n, n, &r.sub)) return fail();
    auto powmod = [&](long b, long e) { long x = 1; b %= p; while (e) { if (e & 1) x = x * b % p; b = b * b % p; e >>= 1; } return x; };
    int g = 0;
    for (int c = 2; c < p && !g; ++c) {
        bool ok = true;
        int m = n;
        for (int f = 2; f <= m && ok; ++f)
            if (m % f == 0) { if (powmod(c, n / f) == 1) ok = false; while (m % f == 0) m /= f; }
        if (ok) g = c;
    }
    if (!g) return fail();
    const long ginv = powmod(g, p - 2);
    std::vector<int> pin(n), pout(n);
    long a = 1, b = 1;
    for (int q = 0; q < n; ++q) { pin[q] = (int)a; pout[q] = (int)b; a = a * g % p; b = b * ginv % p; }
    std::vector<double> br(n), bi(n);
    for (int m = 0; m < n; ++m) {                     // b[m] = w^(g^-m)
        const double ang = -2.0 * M_PI * (double)pout[m] / (double)p;
        br[m] = cos(ang); bi[m] = sin(ang);
    }
    std::vector<float2> bh(n);
    for (int k = 0; k < n; ++k) {                     // plain DFT in double: n^2 = 4e5 terms, once per (device, p)
        double sr = 0, si = 0;
        for (int m = 0; m < n; ++m) {
            const double ang = -2.0 * M_PI * (double)((long)k * m % n) / (double)n;
            const double c = cos(ang), sn = sin(ang);
            sr += br[m] * c - bi[m] * sn;
            si += br[m] * sn + bi[m] * c;
        }
        bh[k] = make_float2((float)(sr / n), (float)(si / n));
    }
    r.p = p; r.perm_in = upload(pin); r.perm_out = upload(pout); r.bhat = upload(bh);
    if (!r.perm_in || !r.perm_out || !r.bhat) return fail();
    std::lock_guard<std::mutex> lk(g_mu);
    g_rader[{devid, p}] = r;
    *out = r;
    return true;
}

// ------------------------------------------------------------------------------------------
// routes
// ------------------------------------------------------------------------------------------
bool plan_big(const Plan& p) {
    for (int i = 0; i < p.nst; ++i)
        if (p.radix[i] == 17 || p.radix[i] == 23) return true;
    return false;
}
bool plan_big2(const Plan& p) {
    for (int i = 0; i < p.nst; ++i)
        if (p.radix[i] == 13 || p.radix[i] == 37 || p.radix[i] == 41) return true;
    return false;
}

int pick_tc(int H) {
    const long per_col = 2L * H * sizeof(float2);
    if (per_col * 16 <= 56 * 1024) return 16;
    if (per_col * 8 <= 140 * 1024) return 8;
    if (per_col * 4 <= 140 * 1024) return 4;
    if (per_col * 2 <= 140 * 1024) return 2;
    return 0;
}

int pick_rpb(int M) {
    // rows per workgroup from an LDS budget for the ping-pong buffers.  Swept on the B=8 720p forward (row kernels, ms per
    // step r2c / c2r): 16 KiB 16.6 / 15.0, 24 KiB 13.3 / 13.4, 32 KiB 13.3 / 12.0, 40 KiB 14.0 / 13.4, 48 KiB 14.1 / 13.4,
    // 64 KiB 15.4 / 14.5 - the passes are latency bound, so workgroups per CU count for more than rows per workgroup
    // (M = 640: 3 rows, 41 KiB with the tables, 3 workgroups per CU, 480 radix-4 jobs for 256 threads)
    int rpb = (int)((32 * 1024) / (2L * M * sizeof(float2)));
    if (rpb > 8) rpb = 8;
    if (rpb < 1) rpb = 1;
    return rpb;
}

// in-place passes possible: every radix has a register butterfly and its jobs fit NT*JMAX threads-slots
int inplace_tc(const Plan& p, int H) {
    for (int tc = 32; tc >= 8; tc >>= 1) {
        if ((long)H * tc > (long)NT * 24) continue;               // keep the buffer <= 48 KiB: 3 workgroups per CU
        bool ok = true;
        for (int i = 0; i < p.nst && ok; ++i) {
            const int R = p.radix[i];
            if (!reg_radix(R)) ok = false;
            else if ((long)(H / R) * tc > (long)NT * (EMAX / R)) ok = false;
        }
        if (ok) return tc;
    }
    return 0;
}

// The route a length takes, decided on the host from the length alone.  The launchers and fdn_fft_route both read it, so
// the query cannot drift from what runs.
constexpr size_t LDS_MAX = 160 * 1024;        // per workgroup (gfx950)

struct Route {
    int kind;                  // FDN_FFT_REFUSED / _PLANNED / _INPLACE / _PINGPONG / _RADER (include/fdn_hip.h)
    int big;                   // BIG of the kernel instantiation
    int width;                 // columns per workgroup (tc) / rows per workgroup (rpb)
    Plan p;                    // radices only (no table); FDN_FFT_PLANNED: (R, P)
    Plan sub;                  // FDN_FFT_RADER: the length p-1 sub-plan
    size_t lds;                // of the generic kernels (a planned kernel's is ColPlan / RowPlan::lds)
};

int planned_route(Route* r, int N, int R, int P, int width) {
    r->kind = FDN_FFT_PLANNED;
    r->width = width;
    r->p.N = N;
    r->p.nst = 2;
    r->p.radix[0] = R;
    r->p.radix[1] = P;
    return FDN_OK;
}

// columns of length H on the generic kernel: in-place passes if every radix has an in-place butterfly and fits, else ping-pong
// passes with pick_tc columns per workgroup; refused when no tc fits or the buffers plus the twiddle table exceed the LDS of a
// workgroup
void cols_route_generic(int H, Route* r) {
    *r = Route{};
    if (!plan_radices(H, &r->p)) return;
    const int itc = inplace_tc(r->p, H);
    if (itc > 0) {
        r->kind = FDN_FFT_INPLACE;
        r->width = itc;
        r->big = plan_big(r->p) ? 1 : 0;
        r->lds = ((size_t)H * itc + H) * sizeof(float2);
        return;
    }
    const int tc = pick_tc(H);
    const size_t lds = (2UL * H * tc + H) * sizeof(float2);
    if (tc == 0 || lds > LDS_MAX) return;
    r->kind = FDN_FFT_PINGPONG;
    r->width = tc;
    r->big = plan_big2(r->p) ? 2 : plan_big(r->p) ? 1 : 0;
    r->lds = lds;
}

// columns of length H: its compile-time plan, else the generic route (fdn_fft_cols_c2c takes the generic route for every length)
void cols_route(int H, Route* r) {
    *r = Route{};
    if (col_plan(H, [&](auto R, auto P) { return planned_route(r, H, R, P, 256 / P); }) == FDN_OK) return;
    cols_route_generic(H, r);
}

// rows of width W (half-length M = W / 2): the compile-time plan if the caller's buffers allow its 8-byte accesses
// (planned_ok), else the generic kernels: Stockham passes, or (forward only) Rader for a prime M; refused when the ping-pong
// rows, the table and the Rader scratch exceed the LDS of a workgroup
void rows_route(int W, bool fwd, bool planned_ok, Route* r) {
    *r = Route{};
    const int M = W / 2;
    if (planned_ok && row_plan(W, [&](auto R1, auto P) { return planned_route(r, M, R1, P, RowPlan<R1, P>::RW); }) == FDN_OK) return;
    if (!plan_radices(M, &r->p)) return;
    const bool rader = fwd && r->p.nst == 1 && rader_ok(M, &r->sub);   // prime half-length: convolution form instead of the O(N^2) gather
    const int rpb = pick_rpb(M);
    const size_t lds = (2UL * rpb * M + W + (rader ? (size_t)M + rpb : 0)) * sizeof(float2);
    if (lds > LDS_MAX) return;
    r->kind = rader ? FDN_FFT_RADER : FDN_FFT_PINGPONG;
    r->width = rpb;
    r->big = (plan_big(r->p) || (rader && plan_big(r->sub))) ? 1 : 0;
    r->lds = lds;
}

bool aligned8(const void* a, const void* b = nullptr) {
    return ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) & 7) == 0;
}

}  // namespace
