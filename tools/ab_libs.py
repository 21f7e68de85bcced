"""Interleaved A/B timing of several builds of libfdn_hip.so in ONE process: tools/ab_libs.py [--edge] [--l2] [kernel,...] lib.so [lib.so ...]
Sequential runs of two builds differ by up to 15 % on this part (clock / temperature), so the builds take turns: R rounds of
(lib A x n, lib B x n, ...), median per build.  Kernels: mid, fused, gate, tail, core, out (level-1 shapes, B = 8; --l2: level 2), and the
fdn_conv1x1 forms c1x1:<case> of C1X1 below (`c1x1` = all of them; the level's own convs, and the deep level-3 shapes at 184 x 320)."""
import ctypes, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fdn-tip2025_amd"))
import torch
import fdn_hip
from fdn_hip import ops

args = sys.argv[1:]
lvl = 1
edge = False
if args and args[0] == "--edge":          # zero patches, tiny values and an exact constant in the inputs: the replace_denormals paths are exercised
    edge, args = True, args[1:]
if args and args[0] == "--l2":
    lvl, args = 2, args[1:]
C1X1 = {   # case: K, N, prologue, epilogue, statistics epilogue, packed weights, deep (level-3 size: 184 x 320)
    "to_hidden": (None, "4E", "ln", None, 0, 0, 0), "to_hidden_pk": (None, "4E", "ln", None, 0, 1, 0), "ffn_in": (None, "Hd", "ln", None, 0, 0, 0),
    "ffn_out": ("Hd", None, None, "res", 1, 0, 0), "attn_out": ("3E", None, "ln3", "res", 1, 0, 0), "fca_in": (None, None, "muladd", "muladd", 0, 0, 0),
    "l3_hidden": (128, 612, "ln", None, 0, 0, 1), "l3_hidden_pk": (128, 612, "ln", None, 0, 1, 1), "l3_ffn_in_pk": (128, 345, "ln", None, 0, 1, 1),
    "l3_ffn_out": (345, 128, None, "res", 1, 0, 1), "l3_ffn_out_pk": (345, 128, None, "res", 1, 1, 1), "l3_attn_out": (459, 128, "ln3", "res", 1, 0, 1),
    "l3_attn_out_pk": (459, 128, "ln3", "res", 1, 1, 1), "l3_fca_in_pk": (128, 128, "muladd", "muladd", 0, 1, 1),
}
kernels = args[0].split(",") if args and not args[0].endswith(".so") and args[0] != "default" else ["mid", "fused", "gate", "tail", "core", "out"]
paths = [a for a in args if a.endswith(".so") or a == "default"] or ["default"]
libs = []
for p in paths:
    l = ctypes.CDLL(fdn_hip.lib_path() if p == "default" else os.path.abspath(p))
    fdn_hip._declare(l, missing_ok=True)        # (a build of an older ABI lacks the newer entry points)
    libs.append((p, l))
kernels = [c for k in kernels for c in (["c1x1:" + n for n in C1X1] if k == "c1x1" else [k])]
dev = torch.device("cuda:0")
B = 8
C = 32 * lvl
H, W = 736 // lvl, 1280 // lvl
E, Hd = int(C * 1.2), int(C * 2.7)
r = lambda *s: torch.randn(*s, device=dev)
P = lambda t: ctypes.c_void_p(t.data_ptr())
st_ = fdn_hip.stream
x = r(B, C, H, W); stats = ops.chan_stats(x); g, b_ = r(C), r(C)
h = r(B, Hd, H, W); w0, w2, fa, fp = r(Hd, 1, 3, 3), r(Hd, 1, 3, 3), r(Hd, 1, 1, 8, 5), r(Hd, 1, 1, 8, 5)
wg = r(2 * Hd, 1, 3, 3); wo = r(C, Hd) / Hd ** .5
wh = r(4 * E, C) / C ** .5; dw, fw = r(4 * E, 1, 3, 3), r(E, 1, 1, 8, 5)
hid = r(B, 4 * E, H, W); wp = r(C, 3 * E) / (3 * E) ** .5; g3, b3 = r(3 * E), r(3 * E)
if edge:
    for t in (x, h, hid):
        t[:, :, :16, :64] = 0.0
        t[:, 3::7, 16:24, :] *= 1e-12
        t[:, 1::5, 32:40, 64:128] = 0.5
        t[:, :, 48:56, :32] = -0.0
    stats = ops.chan_stats(x)
out_h, out_c, out_4e = torch.empty_like(h), torch.empty_like(x), torch.empty_like(hid)
st_out = torch.empty(B, 1, 2, H * W, device=dev)


c1x1_descs = {}               # emptied after each case: its tensors are gigabytes


def c1x1_desc(l, case):
    """the descriptor of a C1X1 case for build `l` (the packed weights belong to the build; the tensors are shared and seeded per case)"""
    if (id(l), case) in c1x1_descs:
        return c1x1_descs[id(l), case]
    K, N, pro, epi, so, packed, deep = C1X1[case]
    dims = {None: C, "4E": 4 * E, "Hd": Hd, "3E": 3 * E}
    K, N = dims.get(K, K), dims.get(N, N)
    h_, w_ = (184, 320) if deep else (H, W)
    P_ = h_ * w_
    g_ = torch.Generator(device=dev).manual_seed(sum(map(ord, case)))
    rn = lambda *s: torch.randn(*s, device=dev, generator=g_)
    t = dict(x=rn(B, K, h_, w_) * 1.5 + 0.3, w=rn(N, K) / K ** .5, bias=rn(N), out=torch.empty(B, N, h_, w_, device=dev), gamma=rn(K), beta=rn(K),
             stats_out=torch.empty(B, 2, P_, device=dev))
    if pro in ("ln3", "muladd"):
        t["xb"] = rn(B, K // 3 if pro == "ln3" else K, h_, w_)
    for name in {"res": ("res",), "muladd": ("mul", "add")}.get(epi, ()):
        t[name] = rn(B, N, h_, w_)
    if edge:
        t["x"][:, :, :16, :64] = 0.0
        t["x"][:, 3::7, 16:24, :] *= 1e-12
    t["stats"] = ops.chan_stats(t["x"], groups=3 if pro == "ln3" else 1)
    d = fdn_hip.Conv1x1Desc()
    d.x[0], d.xbs[0], d.kseg[0] = P(t["x"]), K * P_, K
    d.w, d.bias, d.out, d.obs = P(t["w"]), P(t["bias"]), P(t["out"]), N * P_
    d.B, d.K, d.N, d.P = B, K, N, P_
    d.pro, d.ln_group = {None: 0, "ln": 1, "ln3": 2, "muladd": 3}[pro], K // 3 if pro == "ln3" else K
    if pro:
        d.stats = P(t["stats"])
    if pro in ("ln3", "muladd"):
        d.gamma, d.beta, d.xb, d.xbbs = P(t["gamma"]), P(t["beta"]), P(t["xb"]), t["xb"].shape[1] * P_
    d.epi = {None: 0, "res": 1, "muladd": 2}[epi]
    if epi == "res":
        d.res, d.rbs = P(t["res"]), N * P_
    elif epi == "muladd":
        d.mul, d.add, d.mbs = P(t["mul"]), P(t["add"]), N * P_
    if so:
        d.stats_out = P(t["stats_out"])
    if packed:
        e3 = K // 3 if pro == "ln3" else 0
        t["wpk"] = torch.empty(l.fdn_conv1x1_pack_bytes(N, K, e3), device=dev, dtype=torch.uint8)
        assert l.fdn_conv1x1_pack(P(t["w"]), N, K, e3, P(t["wpk"]), st_()) == 0
        d.wpk = P(t["wpk"])
    c1x1_descs[id(l), case] = (d, t)
    return d, t


def call(l, k):
    if k.startswith("c1x1:"):
        return l.fdn_conv1x1(ctypes.byref(c1x1_desc(l, k[5:])[0]), st_())
    if k == "mid":
        return l.fdn_fdffn_mid(P(h), P(w0), P(w2), P(fa), P(fp), P(out_h), B, Hd, H, W, 0, 0, st_())
    if k == "gate":
        return l.fdn_dwconv_gate(P(h), P(wg), P(out_h), B, Hd, H, W, 0, 0, st_())
    if k == "tail":
        return l.fdn_ffn_tail(P(h), P(wg), P(wo), P(x), P(out_c), P(st_out), B, Hd, C, H, W, 0, 1, st_())
    if k == "core":
        return l.fdn_fdsa_core(P(hid), P(dw), P(fw), P(out_4e), B, E, H, W, st_())
    if k == "out":
        return l.fdn_fdsa_out(P(hid), P(wp), P(g3), P(b3), P(x), P(out_c), P(st_out), B, E, C, H * W, 0, st_())
    if k == "fused":
        return l.fdn_fdsa_fused(P(x), ctypes.c_long(C * H * W), P(stats), P(wpks[id(l)]), P(dw), P(fw), P(out_4e), B, C, E, H, W, 0, st_())
    raise SystemExit("unknown kernel " + k)


wpks = {}
for _, l in libs:                       # (the packed operand layout belongs to the build)
    nb = (E + 7) // 8 * (3 * ((C + 15) // 16) + 1) * 64 * 4
    wpk = torch.empty(max(nb, (E + 7) // 8 * (C // 2 + 1) * 64), device=dev)
    assert l.fdn_fdsa_pack(P(wh), P(g), P(b_), P(wpk), C, E, st_()) == 0
    wpks[id(l)] = wpk


def timeit(l, k, n=8):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        rc = call(l, k)
    e1.record(); torch.cuda.synchronize()
    assert rc == 0, (k, rc)
    return e0.elapsed_time(e1) / n


for k in kernels:
    for _, l in libs:
        timeit(l, k, 2)
    res = {p: [] for p, _ in libs}
    for rnd in range(7):
        for p, l in libs:
            res[p].append(timeit(l, k))
    print(f"L{lvl} {k:6s} " + "   ".join(f"{p}: {statistics.median(v):.3f} ms (min {min(v):.3f})" for p, v in res.items()), flush=True)
    if len(libs) > 1:                  # do the builds agree?  (same inputs: the output buffer of the kernel after each build's call)
        outs = []
        for p, l in libs:
            if k.startswith("c1x1:"):              # (result and statistics epilogue as one tensor)
                t = c1x1_desc(l, k[5:])[1]
                t["out"].fill_(float("nan")); t["stats_out"].fill_(float("nan"))
                call(l, k)
                torch.cuda.synchronize()
                outs.append(torch.cat([t["out"].flatten(), t["stats_out"].flatten() if C1X1[k[5:]][4] else t["out"].new_zeros(0)]))
                continue
            ob = {"mid": out_h, "gate": out_h, "tail": out_c, "out": out_c, "core": out_4e, "fused": out_4e}[k]
            ob.fill_(float("nan"))
            call(l, k)
            torch.cuda.synchronize()
            outs.append(ob.clone())
        for (p, _), o in zip(libs[1:], outs[1:]):
            same = torch.equal(outs[0], o)
            print(f"         {paths[0]} vs {p}: bit-identical {same}" + ("" if same else f", max |diff| {(outs[0] - o).abs().max().item():.3e}, nan {int(torch.isnan(o).sum())}"), flush=True)
            if not same and k in ("core", "fused"):         # which of out1 | out2 | out3 | v_value differ
                print("           per output: " + " ".join(f"{n}={torch.equal(a_, b_)}" for n, a_, b_ in zip(("out1", "out2", "out3", "vv"), outs[0].chunk(4, 1), o.chunk(4, 1))), flush=True)
    c1x1_descs.clear()
