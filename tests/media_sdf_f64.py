"""Participating media and the procedural SDF object restated in float64 on top of tests/pt_f64.py, from the text of include/rpt.h
("procedural SDF object", "participating media") and NOT from oracle/rpt_oracle.hpp: the second, independent statement that the
oracle (tests/test_media_sdf_f64.py) and the device kernels (tests/test_gpu_media_sdf_f64.py) are held to, sample by sample.  Both
features are PROJECT-DEFINED: the reference declares a Medium and never reads it (material.rs:8-34, Readme.md:13) and has no SDF
scene (Readme.md:18), so the header is the only source here; every function below cites the header's block and line of text.

Arithmetic as in pt_f64: plain Python floats, the f32 constants widened (0.9, 0.001, 0.25, INV_4_PI = f32(1 / (4 PI)), TWO_PI), scene
data f32 and widened; exp is math.exp, ln is pt_f64.ln.  1 / k of the smooth union is "computed once" per evaluation as a quotient of
the arithmetic at hand (a double here).

What pt_f64 records as a branch margin is recorded here for every comparison the two features add: the march's `dist < hit_eps * t`
and `t > max_t` at every step, the SDF hit against the running closest distance and against any_hit's max_dist, the free-flight
distance against the segment, |g| against 0.001, dot(dir, normal) at the boundary rule.  (smin's `a < b` and its max(.., 0) select
between values that agree where the branch flips: no margin.)

Besides the margin a sample leaves EVENT COUNTERS (Trace.ev, EVENTS below): which statements of the header it exercised.  The CPU leg
asserts from them that the shared inputs reach every statement often enough to give the MUTANTS below teeth."""
import math

import numpy as np

import pt_f64 as P
from pt_f64 import F_MAX, INF, ONE3, ZERO3, add, clamp, cos, div3, dot, dv, f32, fmax, length, ln, mul, neg, normalize, scale, sin, sqrt, sub

# include/rpt.h
MAT_MEDIUM = 1 << 13
MEDIUM_NONE, MEDIUM_ABSORB, MEDIUM_SCATTER, MEDIUM_EMISSIVE = 0, 1, 2, 3
SDF_SPHERE, SDF_TORUS_Y = 0, 1
SCENE_MEDIA = P.SCENE_MEDIA
INV_4_PI = float(np.float32(1.0 / (4.0 * math.pi)))                  # "INV_4_PI = 1 / (4 * PI)  (f32)"
TWO_PI = P.TWO_PI
G_CLAMP = f32(0.9)                                                    # material.rs:126
G_ISOTROPIC = f32(0.001)

EVENTS = ("scatter", "absorb_segment", "emissive_segment", "nee_in_medium_lit", "entered", "left", "scatter_g_beyond_clamp",
          "scatter_g_isotropic", "emitter_scatter_then_surface", "sdf_hit_at_0", "sdf_steps_exhausted", "sdf_max_t_exit", "sdf_first",
          "sdf_won", "sdf_lost", "any_hit_sdf_ignoring_max_dist", "any_hit_sdf_under_max_dist", "any_hit_sdf_beyond_max_dist", "smin_blend", "torus_eval",
          "plain_surface_in_medium")

# Wrong restatements, each a plausible mis-transcription of the header; tests/test_media_sdf_f64.py shows that every one is caught, by
# the f64 oracle to rounding and by the f32 oracle (the device's twin) at the bounds the device is held to.
MUTANTS = {
    "g_not_clamped": "Material::finalize leaves the anisotropy as set",
    "emitter_flag_kept": "state.is_emitter is not cleared at the top of an iteration",
    "scatter_ray_offset_eps": "the ray leaving a scatter point starts at p + eps * dir",
    "hit_eps_without_t": "the march hits when sdf(p) < hit_eps",
    "nee_medium_unattenuated": "the light sample taken at a scatter point is not attenuated by the medium",
    "nee_surface_unattenuated": "direct_light at a surface inside a medium is not attenuated by it",
    "entering_by_ffnormal": "in_medium = dot(ray.direction, state.ffnormal) < 0",
    "phase_cos_sign_in_nee": "the scatter point's light sample uses phase_hg(dot(ray.direction, light.direction), g)",
    "sample_hg_about_d": "sample_hg about +ray.direction",
    "smin_half": "smin subtracts h*h*k*0.5",
    "central_difference_normal": "the SDF normal from six central-difference samples",
    "torus_about_z": "the torus lies around the z axis",
    "emissive_without_density": "EMISSIVE adds (color * seg) * throughput",
    "absorb_with_color": "ABSORB attenuates by exp(-((color.c * seg) * density))",
    "sdf_unconditional": "a hit of the SDF object is accepted whatever the running closest distance",
    "sdf_any_hit_ignores_max_dist": "any_hit lets the SDF object occlude whatever max_dist",
    "sdf_before_planes": "the SDF object is tested between the spheres and the planes",
    "scatter_transmittance_per_channel": "a SCATTER medium's transmittance per channel, exp(-(((1 - color.c) * dist) * density))",
    "phase_pdf_not_stored": "scatter_sample.pdf keeps the last surface bounce's pdf after a medium scatter",
    "in_medium_cleared_by_plain_surface": "a surface whose material has no medium sets in_medium = false",
    "medium_after_emission": "the medium acts on the segment after State::finalize and the surface's emission",
}


def exp(x):
    try:
        return math.exp(x)
    except OverflowError:
        return INF


def fmin(a, b):                                 # f32::min: a NaN operand yields the other
    if a != a:
        return b
    if b != b:
        return a
    return a if a < b else b


class Trace(P.Margin):
    """pt_f64's Margin with the sample's event counters."""
    __slots__ = ("ev",)

    def __init__(self):
        P.Margin.__init__(self)
        self.ev = {}


def count(M, what):
    ev = getattr(M, "ev", None)
    if ev is not None:
        ev[what] = ev.get(what, 0) + 1


# ---- Medium, Material (material.rs:8-34, 75, 107, 126; include/rpt.h "participating media") -------------------------------------------
class Medium:
    __slots__ = ("type", "density", "color", "g", "g_raw")

    def __init__(self, type=MEDIUM_NONE, density=0.0, color=ZERO3, g=0.0, g_raw=None):       # material.rs:25-32
        self.type, self.density, self.color, self.g = type, density, color, g
        self.g_raw = g if g_raw is None else g_raw


class Material(P.Material):
    __slots__ = ("medium",)

    def __init__(self, rgb_default=1.5):
        P.Material.__init__(self, rgb_default)
        self.medium = Medium()                                                                  # material.rs:107

    def finalize(self, mut=()):
        """Material::finalize with material.rs:126 ("g = the medium's anisotropy, clamped to [-0.9, 0.9] by Material::finalize")."""
        P.Material.finalize(self)
        md = self.medium
        g = md.g if "g_not_clamped" in mut else clamp(md.g, -G_CLAMP, G_CLAMP)
        self.medium = Medium(md.type, md.density, md.color, g, md.g)
        return self


def phase_hg(c, g):
    """"phase_hg(c, g) = INV_4_PI * (1 - g*g) / (d * sqrt(d)),  d = 1 + g*g + 2*g*c"."""
    d = P.noisy(1.0 + g * g + 2.0 * g * c)
    return dv(INV_4_PI * (1.0 - g * g), d * sqrt(d))


def sample_hg(v, g, r1, r2, M=None):
    """"sample_hg(v, g, r1, r2): cos = |g| < 0.001 ? 1 - 2*r2 : -(1 + g*g - q*q) / (2*g), q = (1 - g*g) / (1 + g - 2*g*r2); phi = r1 *
    TWO_PI; sin = clamp(sqrt(1 - cos*cos), 0, 1); (t, b) = onb(v); dir = (sin * cos(phi)) * t + (sin * sin(phi)) * b + cos * v"."""
    M = M or P.Margin()
    M.rel(abs(g), G_ISOTROPIC)
    if abs(g) < G_ISOTROPIC:
        cos_t = 1.0 - 2.0 * r2
    else:
        q = dv(1.0 - g * g, 1.0 + g - 2.0 * g * r2)
        cos_t = dv(-(1.0 + g * g - q * q), 2.0 * g)
    phi = r1 * TWO_PI
    sin_t = clamp(sqrt(1.0 - cos_t * cos_t), 0.0, 1.0)
    t, b = P.onb(v, M)
    return add(add(scale(sin_t * cos(phi), t), scale(sin_t * sin(phi), b)), scale(cos_t, v))


def transmittance(md, dist, mut=()):
    """Step 3 *: "ABSORB exp(-(((1 - color.c) * dist) * density)) per channel, SCATTER exp(-(dist * density)), EMISSIVE 1" (step 2's
    ABSORB line is the same expression over seg)."""
    if md.type == MEDIUM_ABSORB:
        if "absorb_with_color" in mut:
            return tuple(exp(-((c * dist) * md.density)) for c in md.color)
        return tuple(P.noisy(exp(-P.noisy(((1.0 - c) * dist) * md.density))) for c in md.color)
    if md.type == MEDIUM_SCATTER:
        if "scatter_transmittance_per_channel" in mut:
            return tuple(exp(-(((1.0 - c) * dist) * md.density)) for c in md.color)
        e = P.noisy(exp(-P.noisy(dist * md.density)))
        return (e, e, e)
    return ONE3


# ---- the scene: pt_f64.DescScene with material media and the SDF object ----------------------------------------------------------------
class MediaSdfDescScene(P.DescScene):
    """An rpt_scene_desc whose RPT_SCENE_MEDIA flag, RPT_MAT_MEDIUM patches and rpt_sdf are read too."""
    MEDIA_AND_SDF = True

    def __init__(self, desc):
        P.DescScene.__init__(self, desc)
        v3 = lambda a: (float(a[0]), float(a[1]), float(a[2]))              # noqa: E731
        self.media = bool(self.flags & SCENE_MEDIA)
        # "RPT_MAT_MEDIUM writes all four medium fields"
        self.medium_of = [Medium(int(m.medium_type), float(m.medium_density), v3(m.medium_color), float(m.medium_anisotropy))
                          if int(m.mask) & MAT_MEDIUM else None for m in desc.materials[:desc.n_materials]]
        self.sdf = None
        s = desc.sdf
        if int(s.n_prims) > 0:
            self.sdf = dict(prims=[(int(p.kind), v3(p.center), (float(p.params[0]), float(p.params[1]))) for p in s.prims[:s.n_prims]],
                            material=int(s.material), k=float(s.smooth_k), max_steps=int(s.max_steps), hit_eps=float(s.hit_eps),
                            max_t=float(s.max_t), normal_eps=float(s.normal_eps))

    def patch(self, k, d, hp, mat, mut, M):
        P.DescScene.patch(self, k, d, hp, mat, mut, M)
        if self.medium_of[k] is not None:
            mat.medium = self.medium_of[k]

    # -- "procedural SDF object" ----------------------------------------------------------------------------------------------------
    def sdf_prim(self, pr, p, mut=(), M=None):
        """"Sphere: length(p - c) - r.  Torus about y: sqrt(qx*qx + q.y*q.y) - r_minor, with qx = sqrt(q.x*q.x + q.z*q.z) - R"."""
        kind, c, (p0, p1) = pr
        q = sub(p, c)
        if kind == SDF_TORUS_Y:
            count(M, "torus_eval")
            if "torus_about_z" in mut:
                qx = sqrt(q[0] * q[0] + q[1] * q[1]) - p0
                return sqrt(qx * qx + q[2] * q[2]) - p1
            qx = sqrt(q[0] * q[0] + q[2] * q[2]) - p0
            return sqrt(qx * qx + q[1] * q[1]) - p1
        return length(q) - p0

    def sdf_eval(self, p, mut=(), M=None):
        """"Left to right from primitive 0.  h = max(k - |a - b|, 0) * (1/k), m = a < b ? a : b, result m - h*h*k*0.25"."""
        s = self.sdf
        k = s["k"]
        inv_k = dv(1.0, k)
        a = self.sdf_prim(s["prims"][0], p, mut, M)
        for pr in s["prims"][1:]:
            b = self.sdf_prim(pr, p, mut, M)
            h = fmax(k - abs(a - b), 0.0) * inv_k
            if h > 0.0:
                count(M, "smin_blend")
            m = a if a < b else b
            a = m - h * h * k * (0.5 if "smin_half" in mut else 0.25)
        return a

    def march(self, o, d, mut=(), M=None):
        """"t = 0.  At most max_steps times: evaluate at o + t*d; hit when dist < hit_eps * t (an origin inside the object hits at
        t = 0); t = t + dist; leave as a miss when t > max_t" -> t or None."""
        M = M or P.Margin()
        s = self.sdf
        t = 0.0
        for _ in range(s["max_steps"]):
            dist = self.sdf_eval(add(o, scale(t, d)), mut, M)
            bound = s["hit_eps"] if "hit_eps_without_t" in mut else s["hit_eps"] * t
            M.rel(dist, bound)
            if dist < bound:
                if t == 0.0:
                    count(M, "sdf_hit_at_0")
                return t
            t = t + dist
            M.rel(t, s["max_t"])
            if t > s["max_t"]:
                count(M, "sdf_max_t_exit")
                return None
        count(M, "sdf_steps_exhausted")
        return None

    def sdf_normal(self, p, mut=(), M=None):
        """"The four offsets (1,-1,-1), (-1,-1,1), (-1,1,-1), (1,1,1), each scaled by normal_eps.  The sum is taken in that order.  Then
        normalize"."""
        e = self.sdf["normal_eps"]
        if "central_difference_normal" in mut:
            ax = ((1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0))
            return normalize(tuple(self.sdf_eval(add(p, scale(e, a)), mut, M) - self.sdf_eval(sub(p, scale(e, a)), mut, M) for a in ax))
        n = ZERO3
        for i, k in enumerate(((1.0, -1.0, -1.0), (-1.0, -1.0, 1.0), (-1.0, 1.0, -1.0), (1.0, 1.0, 1.0))):
            term = scale(self.sdf_eval(add(p, scale(e, k)), mut, M), k)
            n = term if i == 0 else add(n, term)
        return normalize(n)

    def _sdf_closest(self, o, d, st, first, hit, dist, mut, M):
        """"The object is ... accepted when first || t < dist, and then it updates dist"."""
        t = self.march(o, d, mut, M)
        if t is not None:
            if not first:
                M.rel(t, dist)
            if first or t < dist or "sdf_unconditional" in mut:
                if first or hit:
                    count(M, "sdf_first" if first else "sdf_won")
                hp = add(o, scale(t, d))
                st.hit_dist, st.normal = t, self.sdf_normal(hp, mut, M)
                self.patch(self.sdf["material"], d, hp, st.material, mut, M)
                hit, dist = True, t
            else:
                count(M, "sdf_lost")
        return hit, dist

    def closest_hit(self, o, d, st, ls, mut, M):
        """pt_f64.DescScene.closest_hit's spheres and planes (analytical.rs:36-127), then "the object is tested after the planes ...
        After it come sample_lights"."""
        dist = F_MAX
        hit = False
        first = True
        if self.large is not None:
            cands = self._large_hits(o, d, M)
        else:
            cands = ((k, P.sphere(o, d, s[0], s[1], mut, M)) for k, s in enumerate(self.spheres))
        for k, t in cands:
            if t is not None:
                if not first:
                    M.rel(t, dist)
                if first or t < dist:
                    c = self.spheres[k][0]
                    hp = add(o, scale(t, d))
                    st.hit_dist, st.normal = t, normalize(sub(hp, c))
                    self.patch(self.spheres[k][2], d, hp, st.material, mut, M)
                    hit, dist = True, t
            first = False
        if self.spheres:
            first = False
        if self.sdf is not None and "sdf_before_planes" in mut:
            hit, dist = self._sdf_closest(o, d, st, first, hit, dist, mut, M)
            first = False
        for n, p, md, m, mt in self.planes:
            t = P.plane(o, d, n, p, md, mt, M)
            if t is not None:
                if not first:
                    M.rel(t, dist)
                if first or t < dist:
                    st.hit_dist, st.normal = t, n
                    self.patch(m, d, add(o, scale(t, d)), st.material, mut, M)
                    hit, dist = True, t
            first = False
        if self.sdf is not None and "sdf_before_planes" not in mut:
            hit, dist = self._sdf_closest(o, d, st, first, hit, dist, mut, M)
        if self.sample_lights(o, d, st, ls, mut, M):
            hit = True
        return hit

    def any_hit(self, o, d, max_dist, mut, M):
        """pt_f64.DescScene.any_hit, then "the object goes last, with the scene's max_dist rule"."""
        if P.DescScene.any_hit(self, o, d, max_dist, mut, M):
            return True
        if self.sdf is not None:
            t = self.march(o, d, mut, M)
            if t is not None:
                if not self.flags & P.SCENE_ANYHIT_USES_MAX_DIST:
                    count(M, "any_hit_sdf_ignoring_max_dist")
                    return True
                count(M, "any_hit_sdf_under_max_dist")
                M.rel(t, max_dist)
                if t < max_dist or "sdf_any_hit_ignores_max_dist" in mut:
                    return True
                count(M, "any_hit_sdf_beyond_max_dist")
        return False


# ---- the path: Tracer::render's closure body with include/rpt.h's steps 1-4 ------------------------------------------------------------
class MediaSdfPath(P.Path):
    def __init__(self, scene, mut=(), roulette=False):
        for m in mut:
            assert m in MUTANTS or m in P.MUTANTS, m
        P.Path.__init__(self, scene, [m for m in mut if m in P.MUTANTS], roulette)
        self.mut = frozenset(mut)

    def direct_light(self, d, st, draw, M, rays, phase=None, inside=None):
        """tracer.rs:126-170 as pt_f64.Path.direct_light has it, with the header's two additions: at a scatter point (phase: the
        medium) "scatter_pos = p (no offset) and the phase function in place of the BSDF: f = pdf = phase_hg(dot(-ray.direction,
        light.direction), g), same MIS weight, same pdf > 0 guard"; and (inside: the medium the path is in) "when in_medium and
        light_sample.dist is finite, the unoccluded light's li is multiplied by the medium's transmittance over light_sample.dist" —
        at a scatter point too ("the medium NEE of step 2 is attenuated like step 3's")."""
        sc, mut = self.scene, self.mut
        ld = ZERO3
        scatter_pos = st.fhp if phase is not None else add(st.fhp, scale(self.eps, st.ffnormal))
        n = len(sc.lights)
        if n > 0:
            random = draw() * float(n)
            k = round(random)
            if 1 <= k <= n - 1:
                M.rel(random, float(k))
            light = sc.lights[min(int(random), n - 1)]
            ls = P.sample_light(sc, light, scatter_pos, draw, M)
            li = ls.emission
            fac = dot(ls.direction, ls.normal)
            M.of(fac, 1.0)
            if fac < 0.0:
                max_dist = ls.dist - self.eps
                rays.append(scatter_pos + ls.direction + (max_dist,))
                if not sc.any_hit(scatter_pos, ls.direction, max_dist, mut, M):
                    if inside is not None and ls.dist <= F_MAX:
                        count(M, "nee_in_medium_lit")
                        if ("nee_medium_unattenuated" if phase is not None else "nee_surface_unattenuated") not in mut:
                            li = mul(li, transmittance(inside, ls.dist, mut))
                    if phase is not None:
                        back = d if "phase_cos_sign_in_nee" in mut else neg(d)
                        pdf = phase_hg(dot(back, ls.direction), phase.g)
                        f = (pdf, pdf, pdf)
                    else:
                        f, pdf = P.disney_eval(st.material, st.eta, neg(d), st.ffnormal, ls.direction, mut, M)
                    mis = 1.0
                    if light[6] > 0.0:
                        mis = P.power_heuristic(ls.pdf, pdf, mut)
                    if pdf > 0.0:
                        ld = add(ld, scale(mis, mul(li, div3(f, (ls.pdf, ls.pdf, ls.pdf)))))
        return ld

    def russian_roulette(self, ps, bounce, depth, draw, M):
        """include/rpt.h, RPT_RENDER_RUSSIAN_ROULETTE (as pt_f64.Path.sample has it) -> True: the path ends."""
        if self.roulette and 2 <= bounce + 1 < depth:
            t = ps.throughput
            q = clamp(fmax(fmax(t[0], t[1]), t[2]), f32(0.05), 1.0)
            r = draw()
            M.rel(r, q)
            if r >= q:
                return True
            ps.throughput = div3(t, (q, q, q))
        return False

    def medium_segment(self, ps, st, draw, M, rays):
        """Step 2: "if in_medium, over seg = state.hit_dist" -> True when the path scattered."""
        mut = self.mut
        md = ps.medium
        seg = st.hit_dist
        if md.type == MEDIUM_ABSORB:
            count(M, "absorb_segment")
            ps.throughput = mul(ps.throughput, transmittance(md, seg, mut))
        elif md.type == MEDIUM_EMISSIVE:
            count(M, "emissive_segment")
            e = scale(seg, md.color)
            if "emissive_without_density" not in mut:
                e = scale(md.density, e)
            ps.radiance = add(ps.radiance, mul(e, ps.throughput))
        elif md.type == MEDIUM_SCATTER:
            r = draw()
            flight = dv(-ln(r), md.density)
            M.rel(flight, seg)
            dd = fmin(flight, seg)
            if dd < seg:
                count(M, "scatter")
                if abs(md.g_raw) > G_CLAMP:
                    count(M, "scatter_g_beyond_clamp")
                if abs(md.g) < G_ISOTROPIC:
                    count(M, "scatter_g_isotropic")
                if st.is_emitter:
                    ps.emitter_scatter = True
                ps.throughput = mul(ps.throughput, md.color)
                p = add(ps.o, scale(dd, ps.d))
                ps.o = p
                st.fhp = p
                ps.radiance = add(ps.radiance, mul(self.direct_light(ps.d, st, draw, M, rays, phase=md, inside=md), ps.throughput))
                r1 = draw()
                r2 = draw()
                about = ps.d if "sample_hg_about_d" in mut else neg(ps.d)
                new = sample_hg(about, md.g, r1, r2, M)
                if "phase_pdf_not_stored" not in mut:
                    ps.ss_pdf = phase_hg(dot(neg(ps.d), new), md.g)
                ps.ss_l = new
                ps.d = new
                if "scatter_ray_offset_eps" in mut:
                    ps.o = add(p, scale(self.eps, new))
                return True
        return False

    def sample(self, col, row, width, height, draws):
        """-> (radiance, rays, margin), as pt_f64.Path.sample; self.events: the sample's event counters."""
        sc, mut = self.scene, self.mut
        M = Trace()
        rays = []
        it = iter(draws)
        draw = lambda: float(next(it))                   # noqa: E731
        j = height - 1 - row                             # tracer.rs:29-47, as pt_f64.Path.sample
        xx = float(col) / width
        yy = (float(height) - float(j)) / height
        a = draw()
        b = draw()
        ps = PathState()
        ps.o, ps.d = P.gen_ray(sc.cam, (xx, 1.0 - yy), (a, b), float(width), float(height))
        st = P.State()
        ls = P.LightSampleRec()
        depth = sc.depth
        media = sc.media
        late = "medium_after_emission" in mut
        for bounce in range(depth):
            st.material = Material()
            if media and "emitter_flag_kept" not in mut:                  # step 1
                st.is_emitter = False
            rays.append(ps.o + ps.d + (-1.0,))
            if not sc.closest_hit(ps.o, ps.d, st, ls, mut, M):
                ps.radiance = add(ps.radiance, mul(sc.background(ps.d), ps.throughput))
                break
            if media and ps.in_medium and not late:                      # step 2
                if self.medium_segment(ps, st, draw, M, rays):
                    if self.russian_roulette(ps, bounce, depth, draw, M):
                        break
                    continue
            # step 3: State::finalize, globals.rs:50-62
            o, d = ps.o, ps.d
            st.fhp = add(o, scale(st.hit_dist, d))
            nd = dot(st.normal, d)
            M.of(nd, 1.0)
            st.ffnormal = st.normal if nd <= 0.0 else neg(st.normal)
            st.material.finalize(mut)
            st.eta = dv(1.0, st.material.ior) if nd < 0.0 else st.material.ior
            ps.radiance = add(ps.radiance, mul(st.material.emission, ps.throughput))
            if media and ps.in_medium and late:
                if self.medium_segment(ps, st, draw, M, rays):
                    if self.russian_roulette(ps, bounce, depth, draw, M):
                        break
                    continue
            if st.is_emitter:
                mis = 1.0
                if depth > 0:
                    mis = P.power_heuristic(ps.ss_pdf, ls.pdf, mut)
                ps.radiance = add(ps.radiance, mul(scale(mis, ls.emission), ps.throughput))
                break
            if ps.emitter_scatter:
                count(M, "emitter_scatter_then_surface")
                ps.emitter_scatter = False
            inside = ps.medium if media and ps.in_medium else None
            ps.radiance = add(ps.radiance, mul(self.direct_light(d, st, draw, M, rays, inside=inside), ps.throughput))
            f, ps.ss_l, ps.ss_pdf = P.disney_sample(st.material, st.eta, neg(d), st.ffnormal, ps.ss_l, draw, mut, M)
            if ps.ss_pdf > 0.0:
                ps.throughput = mul(ps.throughput, div3(f, (ps.ss_pdf, ps.ss_pdf, ps.ss_pdf)))
            else:
                break
            ps.d = ps.ss_l
            ps.o = add(st.fhp, scale(self.eps, ps.d))
            if media:                                                    # step 4
                if st.material.medium.type != MEDIUM_NONE:
                    side = dot(ps.d, st.ffnormal if "entering_by_ffnormal" in mut else st.normal)
                    M.of(side, 1.0)
                    was = ps.in_medium
                    ps.in_medium = side < 0.0
                    if ps.in_medium:
                        ps.medium = st.material.medium
                    if ps.in_medium != was:
                        count(M, "entered" if ps.in_medium else "left")
                elif ps.in_medium:
                    count(M, "plain_surface_in_medium")
                    if "in_medium_cleared_by_plain_surface" in mut:
                        ps.in_medium = False
            if self.russian_roulette(ps, bounce, depth, draw, M):
                break
        self.events = M.ev
        return ps.radiance, rays, M.m


class PathState:
    """What the bounce loop carries besides State: the ray, radiance and throughput, ScatterSampleRec's l and pdf, and "in_medium
    (false at the camera) and a copy of the medium it is in"."""
    __slots__ = ("o", "d", "radiance", "throughput", "ss_l", "ss_pdf", "in_medium", "medium", "emitter_scatter")

    def __init__(self):
        self.o = self.d = ZERO3
        self.radiance = ZERO3
        self.throughput = ONE3
        self.ss_l, self.ss_pdf = ZERO3, 0.0
        self.in_medium = False
        self.medium = Medium()
        self.emitter_scatter = False


def n_draws_of(scene):
    """Two jitter draws, then per iteration at most: the free-flight draw, the light index, the light's two, two of the phase function
    or the BSDF, the specular arm's one, the roulette's one."""
    return 2 + 8 * max(scene.depth, 1)


def sample_many(scene, oracle, seed, items, width, height, mut=(), roulette=False):
    """items: (col, row, frame) triples -> (radiance [n, 3], margins [n], rays, events: one dict per sample)."""
    path = MediaSdfPath(scene, mut, roulette)
    out = np.zeros((len(items), 3))
    marg = np.zeros(len(items))
    rays, events = [], []
    nd = n_draws_of(scene)
    for k, (c, r, f) in enumerate(items):
        dr = oracle.rng_f32(seed, int(f), int(r) * width + int(c), nd)
        P.noise_begin(seed, int(f), int(r) * width + int(c))
        rad, ry, m = path.sample(int(c), int(r), width, height, dr)
        out[k] = rad
        marg[k] = m
        rays.append(ry)
        events.append(path.events)
    return out, marg, rays, events


def total(events):
    """The event counters of `events` (a list of per-sample dicts) summed, every name of EVENTS present."""
    t = dict.fromkeys(EVENTS, 0)
    for e in events:
        for k, v in e.items():
            t[k] += v
    return t
