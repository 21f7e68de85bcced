"""The descriptors of tests/conv1x1_routes.txt (the fdn_conv1x1 route sweep of tests/test_host_cpu.py), one per line, to stdout:
    B K N P pro epi act stats_out stats k0 k1 k2 wpk x_bf16 out_bf16 misaligned pipe
(stats_out / stats / wpk: 1 = a pointer, 0 = NULL; misaligned: bits of MISALIGN below; pipe: 0 = bf16, 1 = f32; tests/common.py
conv1x1_case_desc turns a line into a descriptor.)  This regenerates the descriptors only: the route behind the `|` of each line of the
committed file was recorded from the library BEFORE fdn_conv1x1_route existed (its if-ladder, instrumented to name the launcher it
reached), and the file is the record that the table of csrc/conv1x1_route.hpp still answers the same.  A new line gets its route from
a reviewed run of fdn_conv1x1_route, never silently.
python tools/gen_conv1x1_route_cases.py > descriptors.txt"""
NONE, LN, LN3, LNM = 0, 1, 2, 3            # FDN_PRO_*
E_NONE, E_RES, E_MULADD = 0, 1, 2          # FDN_EPI_*
MISALIGN = {"x": 1, "out": 2, "res": 4, "stats": 8, "stats_out": 16, "xbs": 32, "obs": 64, "rbs": 128}
P4, P_ODD = 84 * 131, 83 * 131             # a multiple of 4 (16-byte lanes) / odd, as the GPU geometry tests
# large P: past the 2^31 mask offset of the split kernels, past the 4 GiB plane set of every kernel (K + 40 or N + 200 planes)
P_BIG = (4_200_000, 2_000_004, 16_777_216, 3_000_001)
KS = (16, 32, 48, 64, 96, 112, 128, 160, 256, 345, 459)


def widths(K):
    return sorted({32, 64, 96, 128, 160, 256, 2 * K, (5 * K + 1) // 2})


def line(B, K, N, P, pro, epi, act=0, so=0, st=1, segs=None, wpk=0, xbf=0, obf=0, mis=0, pipe=0):
    k = list(segs or (K,)) + [0, 0]
    return " ".join(str(v) for v in (B, K, N, P, pro, epi, act, so, st, k[0], k[1], k[2], wpk, xbf, obf, mis, pipe))


class Lcg:
    """a generator of our own: the file must not depend on the Python version"""
    def __init__(self, seed):
        self.s = seed

    def below(self, n):
        self.s = (self.s * 6364136223846793005 + 1442695040888963407) % (1 << 64)
        return (self.s >> 33) % n

    def pick(self, seq):
        return seq[self.below(len(seq))]


def grid():
    """every K x N across the thresholds, the prologue / epilogue pairs the networks use, with and without packed weights"""
    out = []
    for K in KS:
        for N in widths(K):
            pairs = [(NONE, E_NONE), (LN, E_NONE), (NONE, E_RES), (LN, E_RES), (LNM, E_MULADD), (LN3, E_RES) if K % 3 == 0 else (LNM, E_NONE)]
            for pro, epi in pairs:
                for wpk in (0, 1):
                    out.append(line(2, K, N, P4, pro, epi, wpk=wpk))
    return out


def scattered(n, seed):
    """every axis at once, around the thresholds: K, N one off, odd / huge P, segments, activation, statistics, bf16 storage,
    misaligned pointers and strides, both pipes"""
    g, out = Lcg(seed), []
    for _ in range(n):
        K = g.pick(KS + (24, 86, 172, 114, 300)) + g.pick((0, 0, 0, 1, -1))
        N = g.pick(widths(K) + [16, 48, 112, 304, 612, 1024]) + g.pick((0, 0, 0, 1, -1))
        pro = g.pick((NONE, NONE, LN, LN, LN3, LNM))
        if pro == LN3 and g.below(4):
            K = K // 3 * 3 or 3
        epi = g.pick((E_NONE, E_NONE, E_RES, E_MULADD))
        P = g.pick((P4, P4, P4, P_ODD, 128, 4)) if g.below(12) else g.pick(P_BIG)
        B = g.pick((1, 2, 2, 8)) if g.below(40) else 600_000
        segs = None
        kind = g.below(8)
        if kind == 0 and K > 40:            # two segments: odd, even, a multiple of 32
            k0 = g.pick((K // 2 | 1, K // 2 & ~1, 32, 64, 96))
            k0 = min(k0, K - 1)
            segs = (k0, K - k0)
        elif kind == 1 and K > 40:
            segs = (16, K - 32, 16) if g.below(2) else (K - 8, 0, 8)
        bf = g.below(10)
        out.append(line(B, K, N, P, pro, epi, act=g.pick((0, 0, 0, 1, 4)), so=int(g.below(4) == 0), st=int(g.below(6) != 0), segs=segs,
                        wpk=g.below(2), xbf=int(bf == 0 or bf == 2), obf=int(bf == 1 or bf == 2),
                        mis=(1 << g.below(8)) if g.below(4) == 0 else 0, pipe=int(g.below(5) == 0)))
    return out


def bf16_storage():
    """the pixel-pair forms with bf16 storage of one operand, across their K / N ladders"""
    out = []
    for K, N in ((172, 64), (172, 32), (172, 96), (172, 97), (97, 64), (96, 32), (86, 32), (64, 32), (32, 32), (33, 16), (86, 33), (345, 96)):
        for epi in (E_NONE, E_RES):
            for so in (0, 1):
                out.append(line(2, K, N, P4, NONE, epi, so=so, xbf=1))
    for K, N in ((32, 86), (32, 152), (32, 64), (32, 63), (64, 172), (64, 304), (64, 128), (24, 64), (48, 129), (33, 192), (64, 193), (16, 43)):
        for pro in (NONE, LN):
            out.append(line(2, K, N, P4, pro, E_NONE, obf=1))
    return out


def cases():
    return grid() + bf16_storage() + scattered(1100, 2025)


if __name__ == "__main__":
    print("\n".join(cases()))
