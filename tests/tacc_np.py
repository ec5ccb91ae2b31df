"""Temporal accumulation of include/rpt.h ("temporal accumulation") restated in numpy float32, operation for operation: what the
kernels of csrc/k_tacc.hip are held to bit for bit (tests/test_gpu_temporal.py).  Every pixel at once.  fma32 is gdn_np's exact fused
multiply-add.  A camera is seven float32 words (origin, center, fov in degrees: rpt_camera); `tan` is the strict tangent the library
uses for a camera's field of view (float32 -> float32: the oracle's, tests/oracle_lib.py, math(100, .))."""
import numpy as np

from gdn_np import F, KEY, KIND, NG, NS, POS, fma32

HIT_NONE = 0
# rpt_history as 8 float32 words
H_RGB, H_N, H_M1, H_M2 = slice(0, 3), 3, 4, 5


def camera(origin, center, fov):
    return np.array(list(origin) + list(center) + [fov], F)


def dot(a, b):
    return fma32(a[..., 0], b[..., 0], fma32(a[..., 1], b[..., 1], a[..., 2] * b[..., 2]))


def _cross(a, b):
    return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]], F)


def basis(cam, width, height, tan):
    """o, u, v, w, half_width, half_height: a render's preparation of a camera (camera/pinhole.rs:38-54), nothing fused."""
    cam = np.asarray(cam, F)
    W, Hh = F(width), F(height)
    ratio = F(W / Hh)
    half_width = F(tan(F(F(cam[6] * F(F(3.14159265358979323846) / F(180.0))) * F(0.5))))
    half_height = F(half_width / ratio)
    o, c = cam[0:3], cam[3:6]
    w = (o - c).astype(F)
    wl = np.sqrt(F(F(w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]))
    w = (w / wl).astype(F)
    u = _cross(np.array([0.0, 1.0, 0.0], F), w)
    v = _cross(w, u)
    return o, u, v, w, half_width, half_height


def host_part(cam, prev_cam, width, height, tan):
    """The host part: the current camera's rd0, horizontal, vertical, psx, psy and the previous camera's o, u, v, w, gx, gy."""
    with np.errstate(all="ignore"):
        o, u, v, w, hw, hh = basis(cam, width, height, tan)
        lower_left = (((o - u * hw) - v * hh) - w).astype(F)
        part = dict(rd0=(lower_left - o).astype(F), horizontal=(u * F(hw * F(2.0))).astype(F), vertical=(v * F(hh * F(2.0))).astype(F),
                    psx=F(F(1.0) / F(width)), psy=F(F(1.0) / F(height)))
        if prev_cam is not None:
            o, u, v, w, hw, hh = basis(prev_cam, width, height, tan)
            part.update(o=o, u=u, v=v, w=w, gx=F(F(0.5) / F(hw * dot(u, u))), gy=F(F(0.5) / F(hh * dot(v, v))))
    return part


def project(part, d, width, height):
    """Step 2: (lam, fx, fy) of directions d [n, 3] through the previous camera."""
    W, Hh = F(width), F(height)
    with np.errstate(all="ignore"):
        lam = -dot(part["w"][None, :], d)
        a = (dot(part["u"][None, :], d) / lam).astype(F)
        b = (dot(part["v"][None, :], d) / lam).astype(F)
        sx, sy = fma32(a, part["gx"], F(0.5)), fma32(b, part["gy"], F(0.5))
        return lam, fma32(sx, W, F(-0.5)), fma32(F(1.0) - sy, Hh, F(-0.5))


def accumulate(pixels, guides, cam, prev_guides, prev_history, prev_cam, prev_positions, n_max, normal_min, plane_k, tan):
    """pixels [h, w, 4], guides [h * w, 16], prev_history [h * w, 8]; the three prev_ all None on the first frame.  Returns
    (out [h, w, 4], history [h * w, 8], decisions): the last a dict of the discrete decisions taken per pixel — `lam` (lam > 0),
    `inside` (the window test), `cell` [n, 2], `valid` [n, 4] and `clamp` (n_h + 1 >= n_max) — for comparisons that must leave out
    pixels where two restatements decided differently."""
    pixels = np.ascontiguousarray(pixels, F)
    guides = np.ascontiguousarray(guides, F)
    h, w = pixels.shape[:2]
    n = w * h
    px = pixels.reshape(n, 4)
    n_max, normal_min, plane_k = F(n_max), F(normal_min), F(plane_k)
    first = prev_guides is None
    assert (prev_history is None) == first and (prev_cam is None) == first
    wsum = np.zeros(n, F)
    acc = np.zeros((n, 6), F)
    dec = dict(lam=np.zeros(n, bool), inside=np.zeros(n, bool), cell=np.zeros((n, 2), np.int64), valid=np.zeros((n, 4), bool), clamp=np.zeros(n, bool))
    with np.errstate(all="ignore"):
        if not first:
            prev_guides = np.ascontiguousarray(prev_guides, F)
            prev_history = np.ascontiguousarray(prev_history, F)
            cam, prev_cam = np.asarray(cam, F), np.asarray(prev_cam, F)
            part = host_part(cam, prev_cam, w, h, tan)
            identity = cam.tobytes() == prev_cam.tobytes() and prev_positions is None
            gu = guides.view(np.uint32)
            key, surface = gu[:, KEY], gu[:, KIND] != HIT_NONE
            src = guides[:, POS]
            if prev_positions is not None:
                src = np.where(surface[:, None], np.ascontiguousarray(prev_positions, F)[:, 0:3], src)
            xs, ys = (np.arange(n) % w), (np.arange(n) // w)
            W, Hh = F(w), F(h)
            pxx = (xs.astype(F) / W).astype(F)
            pyy = (F(1.0) - ((ys + 1).astype(F) / Hh).astype(F)).astype(F)
            sh, sv = (part["psx"] * F(0.5) + pxx).astype(F), (part["psy"] * F(0.5) + pyy).astype(F)
            sky = ((part["rd0"][None, :] + part["horizontal"][None, :] * sh[:, None]).astype(F) + part["vertical"][None, :] * sv[:, None]).astype(F)
            d = np.where(surface[:, None], (src - part["o"][None, :]).astype(F), sky).astype(F)
            kx = (plane_k / dot(d, d)).astype(F) if plane_k > 0 else np.zeros(n, F)
            if identity:
                taps = [(xs, ys, np.ones(n, bool), np.ones(n, F))]
                dec["lam"][:] = True
                dec["inside"][:] = True
                dec["cell"][:, 0], dec["cell"][:, 1] = xs, ys
            else:
                lam, fx, fy = project(part, d, w, h)
                ok = (lam > 0) & (fx > F(-1.0)) & (fx < W) & (fy > F(-1.0)) & (fy < Hh)
                x0f, y0f = np.floor(fx), np.floor(fy)
                wx, wy = (fx - x0f).astype(F), (fy - y0f).astype(F)
                x0, y0 = np.where(ok, x0f, 0).astype(np.int64), np.where(ok, y0f, 0).astype(np.int64)
                one = F(1.0)
                wts = [(one - wx) * (one - wy), wx * (one - wy), (one - wx) * wy, wx * wy]
                taps = []
                for t in range(4):
                    qx, qy = x0 + (t & 1), y0 + (t >> 1)
                    taps.append((qx, qy, ok & (qx >= 0) & (qy >= 0) & (qx < w) & (qy < h), wts[t].astype(F)))
                dec["lam"], dec["inside"] = lam > 0, ok
                dec["cell"][:, 0], dec["cell"][:, 1] = x0, y0
            for t, (qx, qy, inside, wt) in enumerate(taps):
                q = np.clip(qy, 0, h - 1) * w + np.clip(qx, 0, w - 1)
                ph, pg = prev_history[q], prev_guides[q]
                valid = inside & (ph[:, H_N] >= F(1.0)) & np.isfinite(ph[:, [0, 1, 2, H_M1, H_M2]]).all(1) & (pg.view(np.uint32)[:, KEY] == key)
                dpl = dot(guides[:, NG], (pg[:, POS] - src).astype(F))
                geo = (dot(guides[:, NS], pg[:, NS]) >= normal_min) & (fma32(-(dpl * dpl), kx, F(1.0)) > 0)
                valid &= ~surface | geo
                dec["valid"][:, t] = valid
                wsum = np.where(valid, wsum + wt, wsum).astype(F)
                for k, col in enumerate((0, 1, 2, H_N, H_M1, H_M2)):
                    acc[:, k] = np.where(valid, fma32(ph[:, col], wt, acc[:, k]), acc[:, k])
        bits = px[:, 0:3].view(np.uint32) & np.uint32(0x7F800000)
        bad = (bits == np.uint32(0x7F800000)).any(1)
        c = np.where(bad[:, None], F(0.0), px[:, 0:3]).astype(F)
        L = fma32(F(0.2126), c[:, 0], fma32(F(0.7152), c[:, 1], F(0.0722) * c[:, 2]))
        L2 = (L * L).astype(F)
        has = wsum > 0
        hist = (acc / np.where(has, wsum, F(1.0))[:, None]).astype(F)
        np1 = (hist[:, 3] + F(1.0)).astype(F)
        n1 = np.where(np1 < n_max, np1, n_max).astype(F)
        dec["clamp"] = has & ~(np1 < n_max)
        al = (F(1.0) / n1).astype(F)
        keep = (F(1.0) - al).astype(F)
        new = np.concatenate([c, L[:, None], L2[:, None]], 1)              # r g b L L^2 against hist's r g b (n) m1 m2
        old = hist[:, [0, 1, 2, 4, 5]]
        mixed = ((keep[:, None] * old).astype(F) + (new * al[:, None]).astype(F)).astype(F)
        res = np.where(has[:, None], mixed, new).astype(F)
        out = np.empty((n, 4), F)
        out[:, 0:3], out[:, 3] = res[:, 0:3], px[:, 3]
        history = np.zeros((n, 8), F)
        history[:, 0:3], history[:, H_N], history[:, H_M1], history[:, H_M2] = res[:, 0:3], np.where(has, n1, F(1.0)), res[:, 3], res[:, 4]
    return out.reshape(h, w, 4), history, dec
