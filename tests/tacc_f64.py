"""Temporal accumulation of include/rpt.h ("temporal accumulation") restated in float64 from the header's text alone, not from
tests/tacc_np.py or csrc/k_tacc.hip: an independent statement of the specification that the float32 restatement is measured against
(tests/test_temporal.py), and the float64 camera model — rays out, projection back — that the geometry tests build their guides and
expectations with.  numpy only; every pixel at once.

The keyword arguments of accumulate() are deliberate mistakes (tests/test_temporal.py shows that each one is caught)."""
import math

import numpy as np

F32_OVERFLOW = 2.0 ** 128 - 2.0 ** 103                               # the smallest magnitude that rounds to infinity in f32


class Camera:
    """A pinhole as the header's host part prepares it, in float64: o, the basis u, v, w (u and v NOT normalised), the half extents."""

    def __init__(self, cam, width, height):
        cam = np.asarray(cam, np.float32).astype(np.float64)
        self.width, self.height = width, height
        self.half_width = math.tan(math.radians(float(cam[6])) * 0.5)
        self.half_height = self.half_width / (width / height)
        self.o = cam[0:3]
        w = cam[0:3] - cam[3:6]
        self.w = w / np.sqrt((w * w).sum())
        self.u = np.cross(np.array([0.0, 1.0, 0.0]), self.w)
        self.v = np.cross(self.w, self.u)

    def ray(self, fx, fy):
        """The unnormalised direction through image position (fx, fy): pixel centres at integers, row 0 on top."""
        sx, sy = (np.asarray(fx, np.float64) + 0.5) / self.width, 1.0 - (np.asarray(fy, np.float64) + 0.5) / self.height
        return (self.u * (self.half_width * (2.0 * sx - 1.0))[..., None] + self.v * (self.half_height * (2.0 * sy - 1.0))[..., None]) - self.w

    def project(self, d, sy_not_flipped=False, no_half_pixel=False):
        """(lam, fx, fy) of directions d [..., 3]: the inverse of ray()."""
        with np.errstate(all="ignore"):
            lam = -(d * self.w).sum(-1)
            a, b = (d * self.u).sum(-1) / lam, (d * self.v).sum(-1) / lam
            sx = a * (0.5 / (self.half_width * (self.u * self.u).sum())) + 0.5
            sy = b * (0.5 / (self.half_height * (self.v * self.v).sum())) + 0.5
            half = 0.0 if no_half_pixel else 0.5
            return lam, sx * self.width - half, (sy if sy_not_flipped else 1.0 - sy) * self.height - half


def accumulate(pixels, guides, cam, prev_guides, prev_history, prev_cam, prev_positions, n_max, normal_min, plane_k, drop_key=False,
               ns_for_plane=False, kx_without_distance=False, sy_not_flipped=False, no_half_pixel=False, invalid_counts=False, al_from_nh=False):
    """The arguments of tacc_np.accumulate (no `tan`: float64 has its own).  Returns (out [h, w, 4] float64 with the input's alpha,
    history [h * w, 8] float64, decisions, scale [h * w, 5]) — scale: per r, g, b, m1, m2 the largest magnitude that entered the
    value's sums (the taps' values and the new sample), the yardstick its rounding error is measured by.

    Mistakes: drop_key (taps cross keys), ns_for_plane (the plane distance uses ns), kx_without_distance (kx = plane_k),
    sy_not_flipped (row 0 at the bottom), no_half_pixel (fx = sx * W), invalid_counts (an invalid tap's weight counted in wsum),
    al_from_nh (al = 1 / n_h)."""
    pixels = np.asarray(pixels, np.float32)
    h, w = pixels.shape[:2]
    n = w * h
    px = pixels.reshape(n, 4).astype(np.float64)
    g32 = np.ascontiguousarray(guides, np.float32)
    first = prev_guides is None
    n_max, normal_min, plane_k = (float(np.float32(x)) for x in (n_max, normal_min, plane_k))
    wsum = np.zeros(n)
    acc = np.zeros((n, 6))
    big = np.zeros((n, 6))
    dec = dict(lam=np.zeros(n, bool), inside=np.zeros(n, bool), cell=np.zeros((n, 2), np.int64), valid=np.zeros((n, 4), bool), clamp=np.zeros(n, bool))
    with np.errstate(all="ignore"):
        if not first:
            pg32 = np.ascontiguousarray(prev_guides, np.float32)
            ph = np.asarray(prev_history, np.float32).astype(np.float64)
            cam32, pcam32 = np.asarray(cam, np.float32), np.asarray(prev_cam, np.float32)
            identity = cam32.tobytes() == pcam32.tobytes() and prev_positions is None
            A, B = Camera(cam32, w, h), Camera(pcam32, w, h)
            key, surface = g32.view(np.uint32)[:, 3], g32.view(np.uint32)[:, 11] != 0
            pos, ns, ng = (g32[:, s].astype(np.float64) for s in (slice(0, 3), slice(4, 7), slice(8, 11)))
            src = pos
            if prev_positions is not None:
                src = np.where(surface[:, None], np.asarray(prev_positions, np.float32)[:, 0:3].astype(np.float64), pos)
            xs, ys = np.arange(n) % w, np.arange(n) // w
            d = np.where(surface[:, None], src - B.o, A.ray(xs, ys))
            kx = np.zeros(n)
            if plane_k > 0:
                kx = np.full(n, plane_k) if kx_without_distance else plane_k / (d * d).sum(-1)
            if identity:
                taps = [(xs, ys, np.ones(n, bool), np.ones(n))]
                dec["lam"][:], dec["inside"][:] = True, True
                dec["cell"][:, 0], dec["cell"][:, 1] = xs, ys
            else:
                lam, fx, fy = B.project(d, sy_not_flipped, no_half_pixel)
                ok = (lam > 0) & (fx > -1) & (fx < w) & (fy > -1) & (fy < h)
                x0, y0 = np.where(ok, np.floor(fx), 0).astype(np.int64), np.where(ok, np.floor(fy), 0).astype(np.int64)
                wx, wy = fx - np.floor(fx), fy - np.floor(fy)
                wts = [(1 - wx) * (1 - wy), wx * (1 - wy), (1 - wx) * wy, wx * wy]
                taps = [(x0 + (t & 1), y0 + (t >> 1), None, wts[t]) for t in range(4)]
                taps = [(qx, qy, ok & (qx >= 0) & (qy >= 0) & (qx < w) & (qy < h), wt) for qx, qy, _, wt in taps]
                dec["lam"], dec["inside"] = lam > 0, ok
                dec["cell"][:, 0], dec["cell"][:, 1] = x0, y0
            for t, (qx, qy, inside, wt) in enumerate(taps):
                q = np.clip(qy, 0, h - 1) * w + np.clip(qx, 0, w - 1)
                hq = ph[q]
                gq = pg32[q]
                valid = inside & (hq[:, 3] >= 1) & np.isfinite(hq[:, [0, 1, 2, 4, 5]]).all(1)
                if not drop_key:
                    valid &= gq.view(np.uint32)[:, 3] == key
                dpl = ((ns if ns_for_plane else ng) * (gq[:, 0:3].astype(np.float64) - src)).sum(-1)
                geo = ((ns * gq[:, 4:7].astype(np.float64)).sum(-1) >= normal_min) & (1.0 - dpl * dpl * kx > 0)
                valid &= ~surface | geo
                dec["valid"][:, t] = valid
                wsum += np.where(valid | (invalid_counts & inside), wt, 0.0)
                vals = hq[:, [0, 1, 2, 3, 4, 5]]
                acc += np.where(valid[:, None], vals * wt[:, None], 0.0)
                big = np.where(valid[:, None], np.maximum(big, np.abs(vals)), big)
        c = np.where(np.isfinite(px[:, 0:3]).all(1)[:, None], px[:, 0:3], 0.0)
        L = 0.2126 * c[:, 0] + 0.7152 * c[:, 1] + 0.0722 * c[:, 2]
        L2 = L * L
        L2 = np.where(L2 >= F32_OVERFLOW, np.inf, L2)                      # L * L is an f32 product: it overflows where f32 does
        has = wsum > 0
        hist = acc / np.where(has, wsum, 1.0)[:, None]
        np1 = hist[:, 3] + 1.0
        n1 = np.where(np1 < n_max, np1, n_max)
        dec["clamp"] = has & ~(np1 < n_max)
        al = 1.0 / (hist[:, 3] if al_from_nh else n1)
        new = np.concatenate([c, L[:, None], L2[:, None]], 1)
        old = hist[:, [0, 1, 2, 4, 5]]
        res = np.where(has[:, None], (1.0 - al)[:, None] * old + new * al[:, None], new)
        res = np.where(np.abs(res) >= F32_OVERFLOW, np.copysign(np.inf, res), res)
        out = np.concatenate([res[:, 0:3], px[:, 3:4]], 1)
        history = np.zeros((n, 8))
        history[:, 0:3], history[:, 3], history[:, 4], history[:, 5] = res[:, 0:3], np.where(has, n1, 1.0), res[:, 3], res[:, 4]
        scale = np.maximum(np.where(has[:, None], big[:, [0, 1, 2, 4, 5]], 0.0), np.abs(new))
    return out.reshape(h, w, 4), history, dec, scale
