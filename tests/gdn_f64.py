"""The guided denoiser of include/rpt.h ("guided denoiser") restated in float64 from the header's text alone, not from
tests/gdn_np.py or csrc/k_gdn.hip: an independent statement of the specification that the float32 restatement is measured against
with dn_f64.distance (tests/test_denoise_guided.py).  numpy only; every pixel of an iteration at once, by array shifts.

The keyword arguments of denoise_guided() are deliberate mistakes (tests/test_denoise_guided.py shows that each one is caught)."""
import numpy as np

from dn_f64 import _tap

H = (0.25, 0.5, 0.25)
FLOOR = 1.0 / 64.0
F32_OVERFLOW = 2.0 ** 128 - 2.0 ** 103                               # the smallest magnitude that rounds to infinity in f32

# The largest distance dn_f64.distance may report between the float32 restatement (tests/gdn_np.py) and this one, per iteration, in
# units of 2^-23, both outputs divided by the floored albedo first (float64): the distance is then taken in the filter's own
# compressed space, e / (1 + e) — that of the outputs themselves has its pole at an output of -1, which after remodulation is no
# longer the filter's pole.  Basis (tests/gdn_fuzz.py: fuzzed frames of 3-5 key regions, smooth positions with jumps, unit / zero /
# NaN normals, special t, albedo and colours, at 41x29, 64x37, 97x70, 50x50 and 80x33; normal_k and plane_k at 0, at their defaults
# and large, edge_k 1e-6 ... 3e37, iterations 1-6): the largest distance per iteration was 1.80.  The bound keeps a margin of about
# 2x.  The weights are continuous in every input (g = max(t, 0), squared), so no near-tie exclusions are needed.
ULP_PER_ITERATION = 4.0


def denoise_guided(img, guides, iterations, edge_k, normal_k, plane_k, drop_key=False, ns_for_plane=False, no_demodulation=False,
                   remodulate_unfloored=False, kx_without_t2=False, skipped_counts=False):
    """img: (height, width, 4) float32, guides: (height * width, 16) float32 rpt_guide records.  Returns float64.

    Mistakes, for tests that show the comparison has teeth: drop_key (taps cross keys), ns_for_plane (the plane distance uses ns_p),
    no_demodulation (the colour is not divided by the albedo, nor multiplied back), remodulate_unfloored (multiplied back by the
    albedo itself, not the floored one), kx_without_t2 (kx = plane_k), skipped_counts (a pixel none of whose taps has weight takes
    acc / wsum whenever some tap was not skipped, instead of keeping its colour)."""
    img = np.asarray(img, np.float32)
    g = np.asarray(guides, np.float32)
    h, w = img.shape[:2]
    pos = g[:, 0:3].astype(np.float64).reshape(h, w, 3)
    key = g.view(np.uint32)[:, 3].astype(np.float64).reshape(h, w, 1)
    ns = g[:, 4:7].astype(np.float64).reshape(h, w, 3)
    ng = (ns if ns_for_plane else g[:, 8:11].astype(np.float64).reshape(h, w, 3))
    albedo = g[:, 12:15].astype(np.float64).reshape(h, w, 3)
    c = img[..., :3].astype(np.float64)
    with np.errstate(all="ignore"):
        a = np.where(albedo < FLOOR, FLOOR, albedo)
        if no_demodulation:
            a = np.ones_like(a)
        e0 = c / a
        e0 = np.where(np.abs(e0) >= F32_OVERFLOW, np.copysign(np.inf, e0), e0)      # e is an f32 quotient: it overflows where f32 does
        cc = e0 / (1.0 + e0)
        if plane_k > 0:                                             # kx_p is the f32 value plane_k / (t * t): t * t over- and underflows as f32
            t32 = g[:, 7].reshape(h, w)
            kx = np.full((h, w), float(np.float32(plane_k))) if kx_without_t2 else (np.float32(plane_k) / (t32 * t32)).astype(np.float64)
        else:
            kx = np.zeros((h, w))
        k = np.float32(edge_k)                                      # k_i is the f32 value edge_k * 4^i: inf where that overflows
        nk = float(np.float32(normal_k))
        for i in range(iterations):
            s = 1 << i
            acc = np.zeros_like(cc)
            wsum = np.zeros((h, w))
            present = np.zeros((h, w), bool)
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    cq, inside = _tap(cc, dy * s, dx * s, False)
                    pq, nq, kq = (_tap(x, dy * s, dx * s, False)[0] for x in (pos, ns, key))
                    d2 = ((cc - cq) ** 2).sum(-1)
                    dn2 = ((ns - nq) ** 2).sum(-1)
                    dp2 = ((ng * (pq - pos)).sum(-1)) ** 2
                    use = inside & (d2 < np.inf) & (dn2 < np.inf) & (dp2 < np.inf)
                    if not drop_key:
                        use &= (kq == key)[..., 0]
                    gs = []
                    for d, kk in ((d2, np.float64(k)), (dn2, nk), (dp2, kx)):
                        tt = 1.0 - d * kk
                        gs.append(np.where(tt > 0.0, tt, 0.0))          # (a NaN has no weight)
                    wt = np.where(use, H[dy + 1] * H[dx + 1] * gs[0] ** 2 * gs[1] ** 2 * gs[2] ** 2, 0.0)
                    acc += np.where(use[..., None], cq * wt[..., None], 0.0)
                    wsum += wt
                    present |= use
            take = present if skipped_counts else wsum > 0.0
            cc = np.where(take[..., None], acc / np.where(take, wsum, 1.0)[..., None], cc)
            k = np.float32(k * np.float32(4.0))
        out = img.astype(np.float64)
        keep = (np.isfinite(e0) & (e0 != -1.0)).all(-1)
        back = albedo if remodulate_unfloored else a
        out[..., :3] = np.where(keep[..., None], cc / (1.0 - cc) * back, img[..., :3])
    return out
