"""The guided denoiser of include/rpt.h ("guided denoiser") restated in numpy float32, operation for operation: what the kernels of
csrc/k_gdn.hip are held to bit for bit (tests/test_gpu_denoise_guided.py) and what is held, with neutral guides, to the pinned
colour-only filter of the oracle (tests/test_denoise_guided.py).  Every pixel of an iteration at once, by array shifts.

numpy has no fused multiply-add and this Python no math.fma: fma32 takes the product in float64 (exact: 24 x 24 bits), adds in
float64, turns that sum into the round-to-odd one with TwoSum's error term, and casts to float32 — a double rounding that
round-to-odd makes innocuous (53 >= 2 * 24 + 2)."""
import numpy as np

F = np.float32
H = (0.25, 0.5, 0.25)
FLOOR = F(1.0 / 64.0)
INF = F(np.inf)

# rpt_guide as 16 float32 words
POS, KEY, NS, T, NG, KIND, ALBEDO, RESERVED = slice(0, 3), 3, slice(4, 7), 7, slice(8, 11), 11, slice(12, 15), 15
HIT_NONE, HIT_SPHERE, HIT_PLANE, HIT_TRIANGLE = range(4)


def fma32(a, b, c):
    """fma(a, b, c) in float32 with one rounding."""
    a, b, c = (np.asarray(x, F).astype(np.float64) for x in (a, b, c))
    with np.errstate(all="ignore"):
        p = a * b                                                       # exact
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)                                  # TwoSum: p + c = s + err exactly (finite s)
        s, err = np.broadcast_arrays(s, err)
        bits = s.copy().view(np.int64)
        fix = np.isfinite(s) & (err != 0.0) & ((bits & 1) == 0)          # inexact and even: the odd neighbour on err's side
        up = (err > 0.0) == (s > 0.0)                                    # the exact sum is larger in magnitude than s
        bits = np.where(fix, np.where(up, bits + 1, bits - 1), bits)
        return bits.view(np.float64).astype(F)


def neutral_guides(n):
    """n records of the RPT_HIT_NONE guide."""
    g = np.zeros((n, 16), F)
    g[:, T] = np.inf
    g[:, ALBEDO] = 1.0
    return g


def pack(rays, hits, surfaces):
    """rpt_denoise_guides: [n, 8], [n, 8], [n, 16] float32 records -> [n, 16]."""
    rays, hits, surfaces = (np.ascontiguousarray(x, F) for x in (rays, hits, surfaces))
    n = rays.shape[0]
    hu = hits.view(np.uint32)
    kind = hu[:, 1]
    g = np.zeros((n, 16), F)
    gu = g.view(np.uint32)
    with np.errstate(all="ignore"):
        t = hits[:, 0]
        g[:, POS] = rays[:, 0:3] + rays[:, 4:7] * t[:, None]
        ident = np.where(kind == HIT_TRIANGLE, hu[:, 3], hu[:, 2])
        gu[:, KEY] = ((kind.astype(np.uint64) << 28) & 0xFFFFFFFF).astype(np.uint32) | (ident & np.uint32(0x0FFFFFFF))
        g[:, NS] = surfaces[:, 3:6]
        g[:, T] = t
        g[:, NG] = surfaces[:, 0:3]
        g[:, ALBEDO] = surfaces[:, 6:9]
    miss = kind == HIT_NONE
    g[miss] = neutral_guides(int(miss.sum()))
    gu[:, KIND] = kind
    return g


def _tap(a, oy, ox):
    """a shifted by (oy, ox): out[y, x] = a[y + oy, x + ox] (zeros elsewhere), and where that lies inside the image."""
    h, w = a.shape[:2]
    q = np.zeros_like(a)
    valid = np.zeros((h, w), bool)
    y0, y1 = max(0, -oy), min(h, h - oy)
    x0, x1 = max(0, -ox), min(w, w - ox)
    if y0 < y1 and x0 < x1:
        q[y0:y1, x0:x1] = a[y0 + oy:y1 + oy, x0 + ox:x1 + ox]
        valid[y0:y1, x0:x1] = True
    return q, valid


def _sq3(d):
    return fma32(d[..., 0], d[..., 0], fma32(d[..., 1], d[..., 1], d[..., 2] * d[..., 2]))


def floored(albedo):
    return np.where(albedo < FLOOR, FLOOR, albedo).astype(F)


def compress(img, guides):
    """(c', a, e): step 1 of the filter on an image [h, w, 4] and its guides [h * w, 16]."""
    h, w = img.shape[:2]
    with np.errstate(all="ignore"):
        a = floored(guides[:, ALBEDO].reshape(h, w, 3))
        e = img[..., :3] / a
        return e / (F(1.0) + e), a, e


def denoise_guided(img, guides, iterations, edge_k, normal_k, plane_k):
    """img: (height, width, 4) float32, guides: (height * width, 16) float32.  Returns the filtered image in float32."""
    img = np.ascontiguousarray(img, F)
    guides = np.ascontiguousarray(guides, F)
    h, w = img.shape[:2]
    assert guides.shape == (h * w, 16)
    pos, ns, ng = (guides[:, s].reshape(h, w, 3) for s in (POS, NS, NG))
    key = guides.view(np.uint32)[:, KEY].reshape(h, w)
    t = guides[:, T].reshape(h, w)
    normal_k, plane_k = F(normal_k), F(plane_k)
    with np.errstate(all="ignore"):
        c, a, e0 = compress(img, guides)
        kx = (plane_k / (t * t)).astype(F) if plane_k > 0 else np.zeros((h, w), F)
        k = F(edge_k)
        for i in range(iterations):
            s = 1 << i
            acc = np.zeros((h, w, 3), F)
            wsum = np.zeros((h, w), F)
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    cq, inside = _tap(c, dy * s, dx * s)
                    pq, nq, kq = _tap(pos, dy * s, dx * s)[0], _tap(ns, dy * s, dx * s)[0], _tap(key, dy * s, dx * s)[0]
                    d2 = _sq3(c - cq)
                    dn2 = _sq3(ns - nq)
                    r = pq - pos
                    dpl = fma32(ng[..., 0], r[..., 0], fma32(ng[..., 1], r[..., 1], ng[..., 2] * r[..., 2]))
                    dp2 = dpl * dpl
                    use = inside & (kq == key) & (d2 < INF) & (dn2 < INF) & (dp2 < INF)
                    tc, tn, tx = fma32(-d2, k, F(1.0)), fma32(-dn2, normal_k, F(1.0)), fma32(-dp2, kx, F(1.0))
                    gc, gn, gx = (np.where(v > 0, v, F(0.0)).astype(F) for v in (tc, tn, tx))
                    wt = ((F(H[dy + 1] * H[dx + 1]) * (gc * gc)) * (gn * gn)) * (gx * gx)
                    acc = np.where(use[..., None], fma32(cq, wt[..., None], acc), acc)
                    wsum = np.where(use, wsum + wt, wsum)
            c = np.where((wsum > 0)[..., None], acc / wsum[..., None], c).astype(F)        # out of place
            k = F(k * F(4.0))
        out = img.copy()
        keep = (np.isfinite(e0) & (e0 != F(-1.0))).all(-1)
        out[..., :3] = np.where(keep[..., None], (c / (F(1.0) - c)) * a, img[..., :3])
    return out
