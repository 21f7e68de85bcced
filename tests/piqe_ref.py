"""numpy restatement of include/fdn_piqe.h (PIQE), in two forms that share the integer codes, the taps and nothing else
(each has its own filter, its own block statistics and its own lines of classification):

  ordered   float64, every sum in the header's order (r = r + g_t * x, row sums left to right then top to bottom, the tile partials and
            the 256-slot fold), no fused multiply-add: numpy rounds the product and the sum separately - what the device is expected to
            reproduce bit for bit;
  plain     scipy.ndimage.correlate1d(mode='nearest') on the replicate-padded plane for the filter, np.var / np.std(ddof=1) on slices
            for every block statistic: the textbook statement, in whatever order numpy and scipy sum.  It is the check on the ordered
            form (tests/test_piqe_cpu.py).

Also the inputs of the tests and the host step."""
import numpy as np

BLOCK, TILE_H, TILE_W = 16, 32, 64
ACTIVE, WNDC, WNC = 1, 2, 4
T_ACTIVE, T_SEG = 0.1, 0.1


def taps():
    """the 7 taps: exp(-t^2 / (2 (7/6)^2)), t = -3 .. 3, normalised, float64 (fdn_hip.piqe.piqe_taps; the CPU test holds the two equal)"""
    t = np.arange(7, dtype=np.float64) - 3.0
    k = np.exp(-(t * t) / (2.0 * (7.0 / 6.0) * (7.0 / 6.0)))
    return k / k.sum()


def dims(h, w):
    """-> (H, W, block rows, block columns, tile rows, tile columns)"""
    H, W = -(-h // BLOCK) * BLOCK, -(-w // BLOCK) * BLOCK
    return H, W, H // BLOCK, W // BLOCK, -(-H // TILE_H), -(-W // TILE_W)


# ---- planes ---------------------------------------------------------------------------------------------------------------------------
def plane_u8(img, bgr=False):
    """uint8 [h][w][3] -> (int64 codes, q): (299 R + 587 G + 114 B + 500) // 1000, q = 1"""
    x = img.astype(np.int64)
    r, g, b = (x[..., 2], x[..., 1], x[..., 0]) if bgr else (x[..., 0], x[..., 1], x[..., 2])
    return (299 * r + 587 * g + 114 * b + 500) // 1000, 1


def plane_luma(frame, h, w, bits):
    """one frame of samples, Y first -> (int64 codes, q): 8 bit q = 1; 10 bit a code above 1023 counts as 1023 and q = 4"""
    y = np.asarray(frame).reshape(-1)[:h * w].astype(np.uint16 if bits == 10 else np.uint8).astype(np.int64).reshape(h, w)
    return (np.minimum(y, 1023), 4) if bits == 10 else (y, 1)


def _samples(code, q):
    x = code.astype(np.float64) / float(q)
    assert np.array_equal(x * q, code)                                            # exact
    return x


# ---- MSCN -----------------------------------------------------------------------------------------------------------------------------
def mscn_ordered(code, q, g=None):
    """int64 codes [h][w] -> n float64 [H][W] in the header's order"""
    g = taps() if g is None else g
    h, w = code.shape
    H, W = dims(h, w)[:2]
    x = _samples(code, q)
    yi, xi = np.clip(np.arange(-3, H + 3), 0, h - 1), np.clip(np.arange(-3, W + 3), 0, w - 1)
    xp = x[yi][:, xi]                                                             # the padded plane with the filter's reach

    def filt(a):
        r = np.zeros((H + 6, W))
        for t in range(7):
            r = r + g[t] * a[:, t:t + W]
        m = np.zeros((H, W))
        for t in range(7):
            m = m + g[t] * r[t:t + H, :]
        return m

    mu, m2 = filt(xp), filt(xp * xp)
    sd = np.sqrt(np.abs(m2 - mu * mu))
    return (xp[3:3 + H, 3:3 + W] - mu) / (sd + 1.0)


def mscn_plain(code, q, g=None):
    from scipy.ndimage import correlate1d
    g = taps() if g is None else g
    h, w = code.shape
    H, W = dims(h, w)[:2]
    x = np.pad(_samples(code, q), ((0, H - h), (0, W - w)), mode="edge")
    filt = lambda a: correlate1d(correlate1d(a, g, axis=1, mode="nearest"), g, axis=0, mode="nearest")      # noqa: E731
    mu, m2 = filt(x), filt(x * x)
    return (x - mu) / (np.sqrt(np.abs(m2 - mu * mu)) + 1.0)


# ---- per block ------------------------------------------------------------------------------------------------------------------------
def blocks_of(n):
    """[H][W] -> [H/16][W/16][16][16]"""
    H, W = n.shape
    return n.reshape(H // BLOCK, BLOCK, W // BLOCK, BLOCK).transpose(0, 2, 1, 3)


def _seq(terms):
    """0.0 + t_0 + t_1 + ... one at a time, elementwise"""
    s = np.zeros_like(terms[0])
    for t in terms:
        s = s + t
    return s


def _rows_then_down(b, cols):
    """the header's two-stage sum: per row the columns `cols` left to right, then the 16 row sums top to bottom"""
    rs = _seq([b[..., :, j] for j in cols])                                       # [..][16]
    return _seq([rs[..., i] for i in range(BLOCK)])


def _classify(v, minseg, csd):
    """the decisions of the ordered form, as the header writes them: -> dict of sigma, beta, active, wndc, wnc, cls, d"""
    with np.errstate(all="ignore"):
        sigma = np.sqrt(v)
        beta = np.abs(sigma - csd) / np.fmax(sigma, csd)
        active, wndc, wnc = v > T_ACTIVE, minseg < T_SEG, sigma > 2.0 * beta
        d = np.where(wndc, 1.0 - v, 0.0) + np.where(wnc, v, 0.0)
    cls = np.where(active, ACTIVE | np.where(wndc, WNDC, 0) | np.where(wnc, WNC, 0), 0).astype(np.uint8)
    return {"sigma": sigma, "beta": beta, "active": active, "wndc": wndc, "wnc": wnc, "cls": cls, "d": d}


def block_stats_ordered(n):
    """MSCN [H][W] -> dict of [H/16][W/16] arrays: v, minseg (the smallest of the 44 segment stds), cstd, sstd, csd and _classify's"""
    b = blocks_of(n)
    allc, sur = list(range(BLOCK)), [j for j in range(BLOCK) if j not in (7, 8)]
    mean = _rows_then_down(b, allc) / 256.0
    dv = b - mean[..., None, None]
    v = _rows_then_down(dv * dv, allc) / 255.0
    edges = (b[..., 0, :], b[..., :, 15], b[..., 15, :], b[..., :, 0])
    minseg = np.full(v.shape, np.inf)
    for e in edges:
        for s in range(11):
            seg = [e[..., s + i] for i in range(6)]
            m = _seq(seg) / 6.0
            std = np.sqrt(_seq([(x - m) * (x - m) for x in seg]) / 5.0)
            minseg = np.minimum(minseg, std)
    centre = [b[..., i, c] for c in (7, 8) for i in range(BLOCK)]                 # column 7 top to bottom, then column 8
    cm = _seq(centre) / 32.0
    cstd = np.sqrt(_seq([(x - cm) * (x - cm) for x in centre]) / 31.0)
    sm = _rows_then_down(b, sur) / 224.0
    ds = b - sm[..., None, None]
    sstd = np.sqrt(_rows_then_down(ds * ds, sur) / 223.0)
    with np.errstate(all="ignore"):
        csd = cstd / sstd
    csd = np.where(np.isnan(csd), 0.0, csd)
    return {"v": v, "minseg": minseg, "cstd": cstd, "sstd": sstd, "csd": csd, **_classify(v, minseg, csd)}


def classify_plain(v, minseg, csd):
    """the decisions of the plain form, block by block in Python floats, written from the paper's wording and not from _classify"""
    out = {k: np.zeros(v.shape, dtype=t) for k, t in (("sigma", float), ("beta", float), ("active", bool), ("wndc", bool), ("wnc", bool),
                                                       ("cls", np.uint8), ("d", float))}
    for i, j in np.ndindex(*v.shape):
        var, c = float(v[i, j]), float(csd[i, j])
        sigma = var ** 0.5
        big = max(sigma, c)
        beta = abs(sigma - c) / big if big > 0.0 and big != float("inf") else float("nan")
        wndc = bool(minseg[i, j] < 0.1)
        wnc = beta == beta and sigma > 2.0 * beta
        d = 0.0
        if wndc:
            d += 1.0 - var
        if wnc:
            d += var
        active = var > 0.1
        cls = (1 + 2 * wndc + 4 * wnc) if active else 0
        for k, val in (("sigma", sigma), ("beta", beta), ("active", active), ("wndc", wndc), ("wnc", wnc), ("cls", cls), ("d", d)):
            out[k][i, j] = val
    return out


def block_stats_plain(n):
    b = blocks_of(n)
    nby, nbx = b.shape[:2]
    v, minseg, csd = np.zeros((nby, nbx)), np.zeros((nby, nbx)), np.zeros((nby, nbx))
    for i in range(nby):
        for j in range(nbx):
            k = b[i, j]
            v[i, j] = np.var(k, ddof=1)
            minseg[i, j] = min(np.std(e[s:s + 6], ddof=1) for e in (k[0, :], k[:, 15], k[15, :], k[:, 0]) for s in range(11))
            with np.errstate(all="ignore"):
                c = np.std(k[:, 7:9], ddof=1) / np.std(np.delete(k, (7, 8), axis=1), ddof=1)
            csd[i, j] = 0.0 if np.isnan(c) else c
    return {"v": v, "minseg": minseg, "csd": csd, **classify_plain(v, minseg, csd)}


# ---- the result -----------------------------------------------------------------------------------------------------------------------
def fold_ordered(d, active):
    """[H/16][W/16] d and active -> (D, NHSA) in the header's order: tile partials (row-major within the tile), 256 slots walking the
    tiles t, t + 256, ..., then the tree"""
    nby, nbx = d.shape
    th, tw = TILE_H // BLOCK, TILE_W // BLOCK
    parts = []
    for ty in range(-(-nby // th)):
        for tx in range(-(-nbx // tw)):
            p = 0.0
            for i in range(ty * th, min(ty * th + th, nby)):
                for j in range(tx * tw, min(tx * tw + tw, nbx)):
                    if active[i, j]:
                        p = p + float(d[i, j])
            parts.append(p)
    slot = [0.0] * 256
    for t, p in enumerate(parts):
        slot[t % 256] = slot[t % 256] + p
    st = 128
    while st:
        for t in range(st):
            slot[t] = slot[t] + slot[t + st]
        st //= 2
    return slot[0], int(active.sum())


def score(D, nhsa):
    return (D + 1.0) / (1.0 + float(nhsa)) * 100.0


def plane_result(code, q):
    """int64 codes -> dict: mscn, the block arrays of block_stats_ordered, D, nhsa, piqe"""
    n = mscn_ordered(code, q)
    st = block_stats_ordered(n)
    D, nhsa = fold_ordered(st["d"], st["active"])
    return {"mscn": n, **st, "D": D, "nhsa": nhsa, "piqe": score(D, nhsa)}


def plane_result_plain(code, q):
    n = mscn_plain(code, q)
    st = block_stats_plain(n)
    D = float(st["d"][st["active"]].sum())
    nhsa = int(st["active"].sum())
    return {"mscn": n, **st, "D": D, "nhsa": nhsa, "piqe": score(D, nhsa)}


_cache = {}


def result_u8(img, bgr=False):
    """plane_result of an image, computed once per distinct input and shared (do not modify it)"""
    key = (img.shape, bool(bgr), img.tobytes())
    if key not in _cache:
        _cache[key] = plane_result(*plane_u8(img, bgr))
    return _cache[key]


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------
def box(x, k):
    """k x k mean of a float plane, edges replicated"""
    p = np.pad(x, k // 2, mode="edge")
    h, w = x.shape
    return sum(p[i:i + h, j:j + w] for i in range(k) for j in range(k)) / (k * k)


def block_means(x, k=8):
    """every k x k cell replaced by its mean (cells cut at the right and bottom edges)"""
    out = np.empty_like(x)
    for i in range(0, x.shape[0], k):
        for j in range(0, x.shape[1], k):
            out[i:i + k, j:j + k] = x[i:i + k, j:j + k].mean()
    return out


def texture(h, w, seed=0):
    """float [h][w] around 128: white noise smoothed by a 5 x 5 mean, stretched to a contrast a camera would give"""
    g = np.random.default_rng(977 * h + w + 31 * seed)
    return 128.0 + 5.0 * 22.0 * (box(g.standard_normal((h, w)), 5))


def to_u8(x):
    return np.clip(np.rint(x), 0, 255).astype(np.uint8)


def gray3(y):
    """a gray plane as an R = G = B image: its gray code is the plane"""
    return np.ascontiguousarray(np.repeat(to_u8(y)[..., None], 3, axis=2))


def degradations(h, w, seed=0):
    """-> dict of uint8 [h][w][3]: the smooth texture clean, with white noise of sigma 10 and 25, and as its 8 x 8 block means"""
    t = texture(h, w, seed)
    g = np.random.default_rng(5 + seed)
    return {"clean": gray3(t), "noise10": gray3(t + 10.0 * g.standard_normal((h, w))), "noise25": gray3(t + 25.0 * g.standard_normal((h, w))),
            "blocks": gray3(block_means(t))}


def quadrants(h, w, seed=0):
    """uint8 [h][w][3]: four quadrants - a smooth ramp (top left), white noise (top right), the 5 x 5-smoothed texture (bottom left), the
    8 x 8 block means of that texture (bottom right) - with a slow colour cast, so that the gray code has three channels to weigh"""
    g = np.random.default_rng(131 * h + w + 7 * seed)
    hy, hx = (h + 1) // 2, (w + 1) // 2
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    t = texture(h, w, seed)
    out = 40.0 + 150.0 * (x / max(w - 1, 1)) * (y / max(h - 1, 1)) * 4.0
    out[:hy, hx:] = g.integers(0, 256, (h, w))[:hy, hx:]
    out[hy:, :hx] = t[hy:, :hx]
    out[hy:, hx:] = block_means(t)[hy:, hx:]
    tint = np.stack([np.rint(6.0 * np.sin(x / 17.0 + c) * np.cos(y / 23.0 - c)) for c in range(3)], -1)     # smooth: it adds no noise
    return np.clip(np.rint(out)[..., None] + tint, 0, 255).astype(np.uint8)


def luma_frames(B, h, w, bits, seed=0):
    """B 4:2:0 frames [B][h * w * 3 / 2] of uint8 / uint16 whose Y planes are quadrants(); the 10-bit fixture holds codes above 1023"""
    g = np.random.default_rng(17 * h + w + bits + seed)
    n = h * w * 3 // 2
    out = np.zeros((B, n), dtype=np.uint16 if bits == 10 else np.uint8)
    for f in range(B):
        y = plane_u8(quadrants(h, w, seed + f))[0]
        if bits == 10:
            y = y * 4 + g.integers(0, 4, (h, w))
            y[g.random((h, w)) < 0.02] = 1024 + int(g.integers(0, 60000))
        out[f, :h * w] = y.reshape(-1)
        out[f, h * w:] = g.integers(0, 1 << bits if bits == 8 else 1024, n - h * w)
    return out
