"""One pixel-sample of the path tracer restated in float64, from the reference's source text and include/rpt.h, NOT from
oracle/rpt_oracle.hpp: a second, independent statement that the oracle (tests/test_path_f64.py) and the device kernels
(tests/test_gpu_path_f64.py) are held to, sample by sample.  A statement carried into the oracle and the kernels in lockstep, or
mis-transcribed on day one and copied faithfully since, makes them disagree with this file.

Sources, cited per function below (paths relative to the reference crate rust-pathtracer v0.2.4):
  Tracer::render's per-pixel body, direct_light, sample_light, disney_sample, disney_eval and helpers   src/tracer.rs
  Scene::sample_lights, Scene::to_linear                                                               src/scene.rs
  AnalyticalScene (closest_hit, any_hit, sphere, plane, background, the scene itself)                  renderer/src/analytical.rs
  State::new / State::finalize, LightSampleRec, ScatterSampleRec                                       src/globals.rs
  Material::new / Material::finalize                                                                   src/material.rs
  Pinhole::gen_ray                                                                                     src/camera/pinhole.rs
  F3 arithmetic (normalize = v / length, dot, cross, the operators)                                    src/fx.rs, src/math.rs
  the constants PI, INV_PI, TWO_PI and F = f32                                                         src/lib.rs:6-10
Every quirk of SURVEY.md's ledger (Q1-Q14) is reproduced as the Rust has it; the MUTANTS table below names wrong restatements.

Arithmetic: plain Python floats (IEEE double) over `math`, whose sin / cos / tan / pow / log2 are the glibc double routines.
Constants are the f32 values of the Rust literals widened to double (F = f32, lib.rs:6): f32(0.005), f32(0.212671), ...; scene
data are f32 and widened.  IEEE semantics the Python operators lack (x / 0, sqrt / log2 / pow out of domain, f32::max's NaN rule)
are spelled out by the helpers below.

Draws: the stream Oracle.rng_f32(seed, frame, pixel, n) (pinned by tests/test_oracle_kat.py, test_rng_golden_and_float_conversion;
the reference's thread_rng, tracer.rs:44, is OS-seeded and cannot be replayed), consumed in the order the Rust calls rng.gen():
the two jitter draws (tracer.rs:45), then per bounce the light index (:137), the light's r1, r2 (:191-192), the BSDF's r1, r2
(:446-447), and in the specular arm one more (:534).

Project-defined semantics (include/rpt.h, not the reference), restated from the header's text:
  * an rpt_scene_desc's material is a PATCH (mask + values) applied over Material::new() each time a primitive is accepted, in
    primitive order (spheres, then planes, then Scene::sample_lights); RPT_PROC_CHECKER_DIR sets rgb whatever the mask;
  * planes: dot(point - o, n) / dot(n, d), rejected when |dot(n, d)| <= min_denom (and when t > max_t if max_t > 0); the first
    primitive of the scene is accepted whenever it is hit (analytical.rs:43 has no `d < dist` test), every later one only when
    nearer than the running closest distance (a plane updates that distance too: the header lists planes "in order" after the
    spheres; analytical.rs:101-119 can omit the update only because its plane is the last primitive);
  * RPT_SCENE_ANYHIT_USES_MAX_DIST: any_hit accepts an occluder only when d < max_dist; off: any occluder (analytical.rs:130);
  * max_depth is Scene::recursion_depth() (scene.rs:28-30), and the constant State.depth the MIS test reads (Q2);
  * RPT_RENDER_RUSSIAN_ROULETTE: after bounce b's next ray is set, when 2 <= b + 1 < depth, q = clamp(max(t.x, t.y, t.z), 0.05, 1)
    (f32::max), one more draw r, r >= q ends the path, else throughput /= q;
  * RPT_SCENE_SAMPLE_ALL_LIGHT_TYPES: rectangular lights (position + a u + b v, 2 draws, pdf = dist^2 / (area |n.dir|),
    n = normalize(u x v), hit from the side n points to like a spherical light, with pdf = dist^2 / (area cos)) and distant lights
    (direction = normalize(position), no draws, dist = +inf, pdf 1, area 0).  The header does not state a distant light's normal;
    normalize(scatter_pos - position) is taken (the one statement not from the header), and the light-types scene keeps the facing
    test of that light far from its edge, so the comparison does not rest on it;
  * a non-finite sample is blended as black (render-level; oracle_sample_pixels reports the raw radiance).
Media and the SDF object are restated on top of this file by tests/media_sdf_f64.py (DescScene refuses a description that has
either); the denoiser is out of scope here (tests/dn_f64.py).

Outputs of sample(): the radiance (three doubles), the rays it queried in oracle_sample_rays' layout ({o, d, max_dist}, max_dist =
-1 for closest_hit), and the smallest relative BRANCH MARGIN over every comparison the sample took: how far (relatively) the two
sides of each test lay apart.  A sample whose margin is below the rounding error of the arithmetic compared against can take
another branch there, legitimately; every other sample must agree to rounding.

The noise mode (perturbed(), below the constants): the same statements with f32-sized relative noise on the result of every vector
and divide helper, from which tests/f32_spread.py takes each sample's own f32 error bound.  Off, nothing here changes a bit."""
import contextlib
import math

import numpy as np


def f32(x):
    return float(np.float32(x))


# src/lib.rs:8-10 (f32 constants)
PI = f32(math.pi)
INV_PI = float(np.float32(1.0) / np.float32(math.pi))
TWO_PI = float(np.float32(math.pi) * np.float32(2.0))
F_MAX = float(np.finfo(np.float32).max)
F32_TINY = float(np.finfo(np.float32).tiny)
DEG = float(np.float32(math.pi) / np.float32(180.0))          # f32::to_radians multiplies by PI / 180.0 in f32
INF = float("inf")
NAN = float("nan")

# include/rpt.h constants (kept here so that this file needs no import of the package)
MAT_RGB, MAT_EMISSION, MAT_ANISOTROPIC, MAT_METALLIC, MAT_ROUGHNESS, MAT_SUBSURFACE, MAT_SPECULAR_TINT, MAT_SHEEN, MAT_SHEEN_TINT, \
    MAT_CLEARCOAT, MAT_CLEARCOAT_GLOSS, MAT_SPEC_TRANS, MAT_IOR = (1 << i for i in range(13))
PROC_CHECKER_DIR = 1
LIGHT_RECTANGULAR, LIGHT_SPHERICAL, LIGHT_DISTANT = 0, 1, 2
BG_CONSTANT, BG_GRADIENT_Y = 0, 1
SCENE_ANYHIT_USES_MAX_DIST, SCENE_SAMPLE_ALL_LIGHT_TYPES, SCENE_MEDIA = 1, 2, 4
RENDER_RUSSIAN_ROULETTE = 1 << 5

# Wrong restatements, each a plausible mis-transcription; tests/test_path_f64.py shows that every one is caught.
MUTANTS = {
    "Q1_hit_dist_reset": "state.hit_dist starts every bounce at F::MAX, so sample_lights sees this bounce's geometry only",
    "Q2_mis_past_bounce0": "the emitter's MIS weight only from bounce 1 on (as if State.depth were the bounce index)",
    "Q3_honoured": "any_hit honours max_dist whatever the scene flag",
    "Q4_fresh_l": "disney_sample's Fresnel reads the freshly reflected l, not the stale one",
    "Q5_ln": "GTR1 with ln(a^2) instead of log2(a^2)",
    "Q6_r2": "sample_gtr1 draws phi from r2",
    "Q7_checker_by_hit_point": "the checker of the hit point (x, z), not of the ray direction",
    "Q8_offset_ffnormal": "the next ray starts at fhp + eps * ffnormal",
    "Q9_near_root": "a sphere hit from inside returns the near (negative) root",
    "Q12_rgb_one": "Material::new().rgb = (1, 1, 1)",
    "eps_0.001": "Tracer.eps = 0.001",
    "balance_heuristic": "a / (a + b) in place of the power heuristic",
    "jitter_swapped": "the camera jitter's two draws swapped",
    "image_not_flipped": "coord.y = yy instead of 1 - yy",
}


# ---- the noise mode ----------------------------------------------------------------------------------------------------------
# How much f32 rounding a sample amplifies is a property of the sample.  Within `with perturbed(seed, run):` the arithmetic helpers
# below (PERTURBED) multiply every component of their result by 1 + delta, delta uniform in +-2^-24 (half an ulp of f32, relatively);
# how far the sample moves is its sensitivity (tests/f32_spread.py).  Draws, table integers, scene data and the branch margins'
# own arithmetic are never perturbed; comparisons see the perturbed values, as an f32 computation's do.  The generator is seeded
# from (seed, run, the key noise_begin() is given): the sample's own seed, frame and stream index, so that a sample's noise does not
# depend on which other samples were evaluated.  Outside the block _NOISE is None and every helper returns the bits it always did.
NOISE_EPS = 2.0 ** -24
PERTURBED = ("add", "sub", "mul", "scale", "dot", "cross", "dv", "sqrt", "mix3", "mix1", "length, normalize and div3 through sqrt and dv")
_NOISE = None


class Noise:
    __slots__ = ("seed", "run", "rng", "buf", "i")

    def __init__(self, seed, run):
        self.seed, self.run = int(seed), int(run)
        self.begin()

    def begin(self, *key):
        self.rng = np.random.default_rng([self.seed, self.run] + [int(k) & 0xFFFFFFFF for k in key])
        self.buf, self.i = (), 0

    def factor(self):
        if self.i >= len(self.buf):
            self.buf, self.i = (1.0 + self.rng.uniform(-NOISE_EPS, NOISE_EPS, 1024)).tolist(), 0
        self.i += 1
        return self.buf[self.i - 1]

    def v3(self, r):
        f = self.factor
        return (r[0] * f(), r[1] * f(), r[2] * f())

    def array(self, x):
        x = np.asarray(x, np.float64)
        return x * (1.0 + self.rng.uniform(-NOISE_EPS, NOISE_EPS, x.shape))


@contextlib.contextmanager
def perturbed(seed, run=0):
    """Within the block the helpers in PERTURBED carry f32-sized relative noise."""
    global _NOISE
    saved, _NOISE = _NOISE, Noise(seed, run)
    try:
        yield
    finally:
        _NOISE = saved


def noise_begin(*key):
    """Called by every loop over samples before a sample starts, with what identifies the sample (its seed, frame and stream
    index): re-seeds the noise for it.  Nothing happens outside perturbed()."""
    if _NOISE is not None:
        _NOISE.begin(*key)


def noisy(x):
    """A float computed outside the helpers (the mesh restatements' numpy arithmetic) that the device computes in f32."""
    return x if _NOISE is None else x * _NOISE.factor()


def noisy_array(x):
    return x if _NOISE is None else _NOISE.array(x)


# ---- IEEE helpers ------------------------------------------------------------------------------------------------------------
def dv(a, b):
    try:
        r = a / b
    except ZeroDivisionError:
        if a != a or a == 0.0:
            return NAN
        return math.copysign(INF, a) * math.copysign(1.0, b)
    return r if _NOISE is None else r * _NOISE.factor()


def sqrt(x):
    r = math.sqrt(x) if x >= 0.0 else (x if x != x else NAN)
    return r if _NOISE is None else r * _NOISE.factor()


def log2(x):
    if x > 0.0:
        return math.log2(x)
    return -INF if x == 0.0 else NAN


def ln(x):
    if x > 0.0:
        return math.log(x)
    return -INF if x == 0.0 else NAN


def powf(x, y):
    try:
        return math.pow(x, y)
    except ValueError:
        return NAN if x < 0.0 else INF          # (0 ^ negative)
    except OverflowError:
        return INF


def sin(x):
    return math.sin(x) if math.isfinite(x) else NAN


def cos(x):
    return math.cos(x) if math.isfinite(x) else NAN


def fmax(a, b):                                 # f32::max: a NaN operand yields the other
    if a != a:
        return b
    if b != b:
        return a
    return a if a > b else b


def clamp(x, lo, hi):                           # f32::clamp: NaN stays NaN
    if x < lo:
        return lo
    if x > hi:
        return hi
    return x


def add(a, b):
    r = (a[0] + b[0], a[1] + b[1], a[2] + b[2])
    return r if _NOISE is None else _NOISE.v3(r)


def sub(a, b):
    r = (a[0] - b[0], a[1] - b[1], a[2] - b[2])
    return r if _NOISE is None else _NOISE.v3(r)


def mul(a, b):
    r = (a[0] * b[0], a[1] * b[1], a[2] * b[2])
    return r if _NOISE is None else _NOISE.v3(r)


def scale(s, a):
    r = (s * a[0], s * a[1], s * a[2])
    return r if _NOISE is None else _NOISE.v3(r)


def neg(a):
    return (-a[0], -a[1], -a[2])


def dot(a, b):
    r = a[0] * b[0] + a[1] * b[1] + a[2] * b[2]
    return r if _NOISE is None else r * _NOISE.factor()


def cross(a, b):
    r = (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])
    return r if _NOISE is None else _NOISE.v3(r)


def length(a):                                  # (perturbed through sqrt)
    return sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2])


def normalize(a):                               # fx.rs: each component over the length (perturbed through length and dv)
    n = length(a)
    return (dv(a[0], n), dv(a[1], n), dv(a[2], n))


def div3(a, b):                                 # (perturbed through dv)
    return (dv(a[0], b[0]), dv(a[1], b[1]), dv(a[2], b[2]))


def mix3(a, b, v):                              # math.rs mix: (1 - v) * a + b * v per channel
    r = ((1.0 - v) * a[0] + b[0] * v, (1.0 - v) * a[1] + b[1] * v, (1.0 - v) * a[2] + b[2] * v)
    return r if _NOISE is None else _NOISE.v3(r)


def mix1(a, b, v):                              # tracer.rs mix_ptf
    r = (1.0 - v) * a + b * v
    return r if _NOISE is None else r * _NOISE.factor()


ONE3 = (1.0, 1.0, 1.0)
ZERO3 = (0.0, 0.0, 0.0)


class Margin:
    """The smallest relative branch margin seen.  rel(a, b): |a - b| / max(|a|, |b|) of a comparison of a with b; of(x, s): |x| / s
    of a comparison of x with 0 whose operands had magnitude s.  NaN operands are deterministic and record nothing.  Two places
    record the same measure for a quantity that is not compared but divided by (a pole: eval_spec_refraction's half-vector
    denominator) or that magnifies direction rounding (the checker near the horizon): there, as at a branch, f32 and f64 may part."""
    __slots__ = ("m",)

    def __init__(self):
        self.m = INF

    def rel(self, a, b):
        d = abs(a - b)
        if d == d:
            s = max(abs(a), abs(b))
            r = d / s if s > 0.0 else 0.0
            if r < self.m:
                self.m = r

    def range(self, *xs):
        """An intermediate outside f32's normal range (it overflows, or loses precision as a subnormal, in f32): nothing f32
        computes from here on need resemble the double result, so it counts as a tie."""
        for x in xs:
            a = abs(x)
            if a > F_MAX or 0.0 < a < F32_TINY:
                self.m = 0.0

    def of(self, x, s):
        if x == x and s == s:
            r = abs(x) / s if s > 0.0 else (INF if x != 0.0 else 0.0)
            if r < self.m:
                self.m = r


# ---- Material (material.rs) -------------------------------------------------------------------------------------------------
class Material:
    __slots__ = ("rgb", "emission", "anisotropic", "metallic", "roughness", "subsurface", "specular_tint", "sheen", "sheen_tint",
                 "clearcoat", "clearcoat_gloss", "clearcoat_roughness", "spec_trans", "ior", "ax", "ay")

    def __init__(self, rgb_default=1.5):
        """Material::new, material.rs:82-114 (rgb 1.5: quirk Q12)."""
        c = f32(rgb_default)
        self.rgb = (c, c, c)
        self.emission = ZERO3
        self.anisotropic = 0.0
        self.metallic = 0.0
        self.roughness = f32(0.5)
        self.subsurface = 0.0
        self.specular_tint = 0.0
        self.sheen = 0.0
        self.sheen_tint = 0.0
        self.clearcoat = 0.0
        self.clearcoat_gloss = 0.0
        self.clearcoat_roughness = 0.0
        self.spec_trans = 0.0
        self.ior = f32(1.45)
        self.ax = 0.0
        self.ay = 0.0

    def finalize(self):
        """Material::finalize, material.rs:117-131."""
        self.roughness = fmax(self.roughness, f32(0.01))
        self.clearcoat_roughness = mix1(f32(0.1), f32(0.001), self.clearcoat_gloss)
        aspect = sqrt(1.0 - self.anisotropic * f32(0.9))
        self.ax = fmax(dv(self.roughness, aspect), f32(0.001))
        self.ay = fmax(self.roughness * aspect, f32(0.001))
        return self

    FIELDS17 = ("rgb", "emission", "anisotropic", "metallic", "roughness", "subsurface", "specular_tint", "sheen", "sheen_tint",
                "clearcoat", "clearcoat_gloss", "spec_trans", "ior")

    @classmethod
    def from17(cls, m):
        """The 17 user-set floats of the oracle's and the probes' records (rgb, emission, anisotropic ... ior)."""
        mat = cls()
        m = [float(x) for x in m]
        mat.rgb, mat.emission = tuple(m[0:3]), tuple(m[3:6])
        (mat.anisotropic, mat.metallic, mat.roughness, mat.subsurface, mat.specular_tint, mat.sheen, mat.sheen_tint, mat.clearcoat,
         mat.clearcoat_gloss, mat.spec_trans, mat.ior) = m[6:17]
        return mat


# ---- BSDF helpers (tracer.rs:222-439) ---------------------------------------------------------------------------------------
def power_heuristic(a, b, mut):                 # tracer.rs:223-226
    if "balance_heuristic" in mut:
        return dv(a, a + b)
    t = a * a
    return dv(t, b * b + t)


def gtr1(ndoth, a, mut, M):                     # tracer.rs:233-240 (Q5: log2)
    M.rel(a, 1.0)
    if a >= 1.0:
        return INV_PI
    a2 = a * a
    t = 1.0 + (a2 - 1.0) * ndoth * ndoth
    lg = ln(a2) if "Q5_ln" in mut else log2(a2)
    return dv(a2 - 1.0, PI * lg * t)


def sample_gtr1(rgh, r1, r2, mut):              # tracer.rs:242-254 (Q6: r2 unused)
    a = fmax(f32(0.001), rgh)
    a2 = a * a
    phi = (r2 if "Q6_r2" in mut else r1) * TWO_PI
    cos_theta = sqrt(dv(1.0 - powf(a2, 1.0 - r1), 1.0 - a2))
    sin_theta = clamp(sqrt(1.0 - cos_theta * cos_theta), 0.0, 1.0)
    return (sin_theta * cos(phi), sin_theta * sin(phi), cos_theta)


def sample_ggxvndf(v, ax, ay, r1, r2, M):       # tracer.rs:256-274
    vh = normalize((ax * v[0], ay * v[1], v[2]))
    lensq = vh[0] * vh[0] + vh[1] * vh[1]
    M.of(lensq, 1.0)
    if lensq > 0.0:
        s = dv(1.0, sqrt(lensq))
        t_1 = (-vh[1] * s, vh[0] * s, 0.0 * s)
    else:
        t_1 = (1.0, 0.0, 0.0)
    t_2 = cross(vh, t_1)
    r = sqrt(r1)
    phi = 2.0 * PI * r2
    t1 = r * cos(phi)
    t2 = r * sin(phi)
    s = 0.5 * (1.0 + vh[2])
    t2 = (1.0 - s) * sqrt(1.0 - t1 * t1) + s * t2
    w = sqrt(fmax(0.0, 1.0 - t1 * t1 - t2 * t2))
    nh = add(add(scale(t1, t_1), scale(t2, t_2)), scale(w, vh))
    return normalize((ax * nh[0], ay * nh[1], fmax(0.0, nh[2])))


def smithg(ndotv, alphag):                      # tracer.rs:276-280
    a = alphag * alphag
    b = ndotv * ndotv
    return dv(2.0 * ndotv, ndotv + sqrt(a + b - a * b))


LUM = (f32(0.212671), f32(0.715160), f32(0.072169))


def luminance(c):                               # tracer.rs:284-286
    return LUM[0] * c[0] + LUM[1] * c[1] + LUM[2] * c[2]


def schlick_fresnel(u):                         # tracer.rs:288-292
    m = clamp(1.0 - u, 0.0, 1.0)
    m2 = m * m
    return m2 * m2 * m


def gtr2aniso(ndoth, hdotx, hdoty, ax, ay):     # tracer.rs:294-299
    a = dv(hdotx, ax)
    b = dv(hdoty, ay)
    c = a * a + b * b + ndoth * ndoth
    return dv(1.0, PI * ax * ay * c * c)


def smithganiso(ndotv, vdotx, vdoty, ax, ay):   # tracer.rs:301-306
    a = vdotx * ax
    b = vdoty * ay
    c = ndotv
    return dv(2.0 * ndotv, ndotv + sqrt(a * a + b * b + c * c))


def dielectric_fresnel(cos_theta_i, eta, M):    # tracer.rs:308-322
    sin_theta_tsq = eta * eta * (1.0 - cos_theta_i * cos_theta_i)
    M.rel(sin_theta_tsq, 1.0)
    if sin_theta_tsq > 1.0:
        return 1.0
    cos_theta_t = sqrt(fmax(1.0 - sin_theta_tsq, 0.0))
    rs = dv(eta * cos_theta_t - cos_theta_i, eta * cos_theta_t + cos_theta_i)
    rp = dv(eta * cos_theta_i - cos_theta_t, eta * cos_theta_i + cos_theta_t)
    return 0.5 * (rs * rs + rp * rp)


def cosine_sample_hemisphere(r1, r2):           # tracer.rs:324-333
    r = sqrt(r1)
    phi = TWO_PI * r2
    x = r * cos(phi)
    y = r * sin(phi)
    return (x, y, sqrt(fmax(0.0, 1.0 - x * x - y * y)))


def spec_color(mat, eta, M):                    # tracer.rs:335-341
    lum = luminance(mat.rgb)
    M.of(lum, max(mat.rgb) if max(mat.rgb) > 0 else 1.0)
    ctint = div3(mat.rgb, (lum, lum, lum)) if lum > 0.0 else ONE3
    f0 = dv(1.0 - eta, 1.0 + eta)
    spec = mix3(scale(f0 * f0, mix3(ONE3, ctint, mat.specular_tint)), mat.rgb, mat.metallic)
    sheen = mix3(ONE3, ctint, mat.sheen_tint)
    return spec, sheen


def eval_diffuse(mat, c_sheen, v, l, h, M):     # tracer.rs:343-366
    M.of(l[2], 1.0)
    if l[2] <= 0.0:
        return ZERO3, 0.0
    fl = schlick_fresnel(l[2])
    fv = schlick_fresnel(v[2])
    ldh = dot(l, h)
    fh = schlick_fresnel(ldh)
    fd90 = 0.5 + 2.0 * ldh * ldh * mat.roughness
    fd = mix1(1.0, fd90, fl) * mix1(1.0, fd90, fv)
    fss90 = ldh * ldh * mat.roughness
    fss = mix1(1.0, fss90, fl) * mix1(1.0, fss90, fv)
    ss = 1.25 * (fss * (dv(1.0, l[2] + v[2]) - 0.5) + 0.5)
    fsheen = scale(fh * mat.sheen, c_sheen)
    k = (1.0 - mat.metallic) * (1.0 - mat.spec_trans)
    return scale(k, add(scale(INV_PI * mix1(fd, ss, mat.subsurface), mat.rgb), fsheen)), l[2] * INV_PI


def disney_fresnel(mat, eta, ldoth, vdoth, M):  # tracer.rs:435-439
    metallic_fresnel = schlick_fresnel(ldoth)
    dielectric = dielectric_fresnel(abs(vdoth), eta, M)
    return mix1(dielectric, metallic_fresnel, mat.metallic)


def eval_spec_reflection(mat, eta, spec_col, v, l, h, M):     # tracer.rs:368-382
    M.of(l[2], 1.0)
    if l[2] <= 0.0:
        return ZERO3, 0.0
    fm = disney_fresnel(mat, eta, dot(l, h), dot(v, h), M)
    f = mix3(spec_col, ONE3, fm)
    d = gtr2aniso(h[2], h[0], h[1], mat.ax, mat.ay)
    g1 = smithganiso(abs(v[2]), v[0], v[1], mat.ax, mat.ay)
    g2 = g1 * smithganiso(abs(l[2]), l[0], l[1], mat.ax, mat.ay)
    pdf = dv(g1 * d, 4.0 * v[2])
    den = 4.0 * l[2] * v[2]
    M.range(d, g1 * d, pdf, den, d * g2)
    return div3(scale(d * g2, f), (den, den, den)), pdf


def eval_spec_refraction(mat, eta, v, l, h, M):                # tracer.rs:384-402
    M.of(l[2], 1.0)
    if l[2] >= 0.0:
        return ZERO3, 0.0
    vdh = dot(v, h)
    ldh = dot(l, h)
    f = dielectric_fresnel(abs(vdh), eta, M)
    d = gtr2aniso(h[2], h[0], h[1], mat.ax, mat.ay)
    g1 = smithganiso(abs(v[2]), v[0], v[1], mat.ax, mat.ay)
    g2 = g1 * smithganiso(abs(l[2]), l[0], l[1], mat.ax, mat.ay)
    denom = ldh + vdh * eta
    M.of(denom, abs(ldh) + abs(vdh * eta))          # (not a branch: a pole the quotient below sits near, eta = 1 straight through)
    denom *= denom
    eta2 = eta * eta
    jacobian = dv(abs(ldh), denom)
    M.range(d, denom, jacobian, d * jacobian)
    M.of(vdh, 1.0)
    pdf = dv(g1 * fmax(0.0, vdh) * d * jacobian, v[2])
    k = dv((1.0 - mat.metallic) * mat.spec_trans * (1.0 - f) * d * g2 * abs(vdh) * jacobian * eta2, abs(l[2] * v[2]))
    return scale(k, tuple(powf(c, 0.5) for c in mat.rgb)), pdf


def eval_clearcoat(mat, v, l, h, mut, M):      # tracer.rs:404-419
    M.of(l[2], 1.0)
    if l[2] <= 0.0:
        return ZERO3, 0.0
    vdh = dot(v, h)
    fh = dielectric_fresnel(vdh, float(np.float32(1.0) / np.float32(1.5)), M)
    f = mix1(f32(0.04), 1.0, fh)
    d = gtr1(h[2], mat.clearcoat_roughness, mut, M)
    g = smithg(l[2], 0.25) * smithg(v[2], 0.25)
    jacobian = dv(1.0, 4.0 * vdh)
    k = dv(mat.clearcoat * f * d * g, 4.0 * l[2] * v[2])
    M.range(d, jacobian, 4.0 * l[2] * v[2], k)
    return (k * 0.25, k * 0.25, k * 0.25), d * h[2] * jacobian


def lobe_probabilities(mat, spec_col, approx_fresnel):         # tracer.rs:421-433
    lum = luminance(mat.rgb)
    dw = lum * (1.0 - mat.metallic) * (1.0 - mat.spec_trans)
    srw = luminance(mix3(spec_col, ONE3, approx_fresnel))
    stw = (1.0 - approx_fresnel) * (1.0 - mat.metallic) * mat.spec_trans * lum
    cw = 0.25 * mat.clearcoat * (1.0 - mat.metallic)
    total = dw + srw + stw + cw
    return dv(dw, total), dv(srw, total), dv(stw, total), dv(cw, total)


def onb(n, M):                                  # tracer.rs:184-189, 449-454, 559-564 (all three alike)
    M.rel(abs(n[2]), f32(0.999))
    up = (0.0, 0.0, 1.0) if abs(n[2]) < f32(0.999) else (1.0, 0.0, 0.0)
    t = normalize(cross(up, n))
    return t, cross(n, t)


def to_local(t, b, n, v):
    return (dot(v, t), dot(v, b), dot(v, n))


def to_world(t, b, n, v):
    return add(add(scale(v[0], t), scale(v[1], b)), scale(v[2], n))


def reflect(i, n):                              # tracer.rs:464-466
    d = dot(n, i)
    return sub(i, (2.0 * n[0] * d, 2.0 * n[1] * d, 2.0 * n[2] * d))


def refract(i, n, eta, M):                      # tracer.rs:468-475
    d = dot(n, i)
    k = 1.0 - eta * eta * (1.0 - d * d)
    M.of(k, 1.0)
    if k < 0.0:
        return ZERO3
    return sub(scale(eta, i), scale(eta * d + sqrt(k), n))


def disney_sample(mat, eta, v, n, l_stale, draw, mut=(), M=None):
    """tracer.rs:441-553 -> (f, l, pdf).  l_stale: scatter_sample.l as the previous bounce left it (zeros on bounce 0): the
    specular arm's Fresnel reads it (Q4).  draw(): the next draw."""
    M = M or Margin()
    r1 = draw()
    r2 = draw()
    t, b = onb(n, M)
    v = to_local(t, b, n, v)
    spec_col, sheen_col = spec_color(mat, eta, M)
    approx_fresnel = disney_fresnel(mat, eta, v[2], v[2], M)
    dw, srw, stw, cw = lobe_probabilities(mat, spec_col, approx_fresnel)
    cdf0 = dw
    cdf1 = cdf0 + cw
    M.rel(r1, cdf0)
    M.rel(r1, cdf1)
    if r1 < cdf0:
        r1 = dv(r1, cdf0)
        l = cosine_sample_hemisphere(r1, r2)
        h = normalize(add(l, v))
        f, pdf = eval_diffuse(mat, sheen_col, v, l, h, M)
        pdf *= dw
    elif r1 < cdf1:
        r1 = dv(r1 - cdf0, cdf1 - cdf0)
        h = sample_gtr1(mat.clearcoat_roughness, r1, r2, mut)
        M.of(h[2], 1.0)
        if h[2] < 0.0:
            h = neg(h)
        l = normalize(reflect(neg(v), h))
        f, pdf = eval_clearcoat(mat, v, l, h, mut, M)
        pdf *= cw
    else:
        r1 = dv(r1 - cdf1, 1.0 - cdf1)
        h = sample_ggxvndf(v, mat.ax, mat.ay, r1, r2, M)
        M.of(h[2], 1.0)
        if h[2] < 0.0:
            h = neg(h)
        lf = normalize(reflect(neg(v), h)) if "Q4_fresh_l" in mut else l_stale
        fresnel = disney_fresnel(mat, eta, dot(lf, h), dot(v, h), M)
        ff = 1.0 - ((1.0 - fresnel) * mat.spec_trans * (1.0 - mat.metallic))
        rand = draw()
        M.rel(rand, ff)
        if rand < ff:
            l = normalize(reflect(neg(v), h))
            f, pdf = eval_spec_reflection(mat, eta, spec_col, v, l, h, M)
            pdf *= ff
        else:
            l = normalize(refract(neg(v), h, eta, M))
            f, pdf = eval_spec_refraction(mat, eta, v, l, h, M)
            pdf *= 1.0 - ff
        pdf *= srw + stw
    l = to_world(t, b, n, l)
    return scale(abs(dot(n, l)), f), l, pdf


def disney_eval(mat, eta, v, n, l, mut=(), M=None):
    """tracer.rs:555-626 -> (f, pdf)."""
    M = M or Margin()
    t, b = onb(n, M)
    v = to_local(t, b, n, v)
    l = to_local(t, b, n, l)
    M.of(l[2], 1.0)
    h = normalize(add(l, v)) if l[2] > 0.0 else normalize(add(l, scale(eta, v)))
    M.of(h[2], 1.0)
    if h[2] < 0.0:
        h = neg(h)
    spec_col, sheen_col = spec_color(mat, eta, M)
    fresnel = disney_fresnel(mat, eta, dot(l, h), dot(v, h), M)
    dw, srw, stw, cw = lobe_probabilities(mat, spec_col, fresnel)
    M.of(v[2], 1.0)
    f = ZERO3
    pdf = 0.0
    if dw > 0.0 and l[2] > 0.0:
        ff, p = eval_diffuse(mat, sheen_col, v, l, h, M)
        f = add(f, ff)
        pdf += p * dw
    if srw > 0.0 and l[2] > 0.0 and v[2] > 0.0:
        ff, p = eval_spec_reflection(mat, eta, spec_col, v, l, h, M)
        f = add(f, ff)
        pdf += p * srw
    if stw > 0.0 and l[2] < 0.0:
        ff, p = eval_spec_refraction(mat, eta, v, l, h, M)
        f = add(f, ff)
        pdf += p * stw
    if cw > 0.0 and l[2] > 0.0 and v[2] > 0.0:
        ff, p = eval_clearcoat(mat, v, l, h, mut, M)
        f = add(f, ff)
        pdf += p * cw
    return scale(abs(l[2]), f), pdf


# ---- geometry ---------------------------------------------------------------------------------------------------------------
def sphere(o, d, c, r, mut=(), M=None):
    """analytical.rs:166-190 (= scene.rs:39-63) -> t or None.  Q9: from inside, the far root."""
    lx, ly, lz = c[0] - o[0], c[1] - o[1], c[2] - o[2]
    tca = lx * d[0] + ly * d[1] + lz * d[2]
    ll = lx * lx + ly * ly + lz * lz
    d2 = ll - tca * tca
    radius2 = r * r
    if M is not None:
        M.of(d2 - radius2, max(ll, radius2))
    if d2 > radius2:
        return None
    thc = sqrt(radius2 - d2)
    t0 = tca - thc
    t1 = tca + thc
    if t0 > t1:
        t0, t1 = t1, t0
    if M is not None:
        s = max(abs(tca), thc)
        M.of(t0, s)
    if t0 < 0.0:
        if M is not None:
            M.of(t1, s)
        if "Q9_near_root" in mut and t1 >= 0.0:
            return t0
        t0 = t1
        if t0 < 0.0:
            return None
    return t0


def plane(o, d, normal, point, min_denom, max_t=0.0, M=None):
    """analytical.rs:193-204 with the plane as data (include/rpt.h rpt_plane) -> t or None."""
    denom = dot(normal, d)
    if M is not None:
        M.rel(abs(denom), min_denom)
    if abs(denom) > min_denom:
        num = dot(sub(point, o), normal)
        t = dv(num, denom)
        if M is not None:
            M.of(num, abs(dot(point, normal)) + abs(dot(o, normal)))
            if max_t > 0.0:
                M.rel(t, max_t)
        if t >= 0.0 and (not max_t > 0.0 or t <= max_t):
            return t
    return None


def gen_ray(cam, p, offset, width, height):
    """Pinhole::gen_ray, camera/pinhole.rs:38-60.  cam = (origin, center, fov_deg)."""
    origin, center, fov = cam
    ratio = width / height
    psx, psy = 1.0 / width, 1.0 / height
    half_width = math.tan(fov * DEG * 0.5)
    half_height = half_width / ratio
    w = normalize(sub(origin, center))
    u = cross((0.0, 1.0, 0.0), w)
    v = cross(w, u)
    lower_left = sub(sub(sub(origin, scale(half_width, u)), scale(half_height, v)), w)
    horizontal = scale(half_width * 2.0, u)
    vertical = scale(half_height * 2.0, v)
    rd = sub(lower_left, origin)
    rd = add(rd, scale(psx * offset[0] + p[0], horizontal))
    rd = add(rd, scale(psy * offset[1] + p[1], vertical))
    return origin, normalize(rd)


def checker(x, y, M, cond=(1.0, 1.0)):        # analytical.rs:107-111
    """cond: how strongly x and y amplify a perturbation of the ray direction (scale / |dir.y|-style factors; 1: not at all)."""
    M.of(x - round(x), max(abs(x), 1.0, cond[0]))
    M.of(y - round(y), max(abs(y), 1.0, cond[1]))
    x1 = math.fmod(math.floor(x), 2.0) if math.isfinite(x) else NAN
    y1 = math.fmod(math.floor(y), 2.0) if math.isfinite(y) else NAN
    return math.fmod(x1 + y1, 2.0) < 1.0 if (x1 == x1 and y1 == y1) else False


# ---- scenes -----------------------------------------------------------------------------------------------------------------
class DescScene:
    """An rpt_scene_desc read field by field (include/rpt.h) — spheres, planes, lights, material patches, camera, background."""
    BITS = [(MAT_ANISOTROPIC, "anisotropic"), (MAT_METALLIC, "metallic"), (MAT_ROUGHNESS, "roughness"), (MAT_SUBSURFACE, "subsurface"),
            (MAT_SPECULAR_TINT, "specular_tint"), (MAT_SHEEN, "sheen"), (MAT_SHEEN_TINT, "sheen_tint"), (MAT_CLEARCOAT, "clearcoat"),
            (MAT_CLEARCOAT_GLOSS, "clearcoat_gloss"), (MAT_SPEC_TRANS, "spec_trans"), (MAT_IOR, "ior")]

    MEDIA_AND_SDF = False                           # tests/media_sdf_f64.py's scene class restates them; this one does not

    def __init__(self, desc):
        v3 = lambda a: (float(a[0]), float(a[1]), float(a[2]))              # noqa: E731
        if not self.MEDIA_AND_SDF and (int(desc.flags) & SCENE_MEDIA or int(desc.sdf.n_prims) > 0):
            raise ValueError("a description with RPT_SCENE_MEDIA or an SDF object: restate it with media_sdf_f64.MediaSdfDescScene")
        self.flags = int(desc.flags)
        self.cam = (v3(desc.camera.origin), v3(desc.camera.center), float(desc.camera.fov_deg))
        bg = desc.background
        self.bg = (int(bg.kind), v3(bg.colour_a), v3(bg.colour_b), float(bg.gamma), float(bg.scale))
        self.eps = float(desc.eps)
        self.depth = int(desc.max_depth)
        self.spheres = [(v3(s.center), float(s.radius), int(s.material)) for s in desc.spheres[:desc.n_spheres]]
        self.planes = [(v3(p.normal), v3(p.point), float(p.min_denom), int(p.material), float(p.max_t)) for p in desc.planes[:desc.n_planes]]
        self.lights = [(int(L.type), v3(L.position), v3(L.emission), v3(L.u), v3(L.v), float(L.radius), float(L.area))
                       for L in desc.lights[:desc.n_lights]]
        self.materials = []
        for m in desc.materials[:desc.n_materials]:
            self.materials.append((int(m.mask), int(m.proc_kind), v3(m.rgb), v3(m.emission),
                                   dict(anisotropic=float(m.anisotropic), metallic=float(m.metallic), roughness=float(m.roughness),
                                        subsurface=float(m.subsurface), specular_tint=float(m.specular_tint), sheen=float(m.sheen),
                                        sheen_tint=float(m.sheen_tint), clearcoat=float(m.clearcoat), clearcoat_gloss=float(m.clearcoat_gloss),
                                        spec_trans=float(m.spec_trans), ior=float(m.ior)),
                                   tuple(float(x) for x in m.proc_params)))
        self.large = None
        if len(self.spheres) > 64:                  # brute force over the sphere table with numpy
            self.large = (np.array([s[0] for s in self.spheres]), np.array([s[1] for s in self.spheres]))

    def background(self, d):                    # analytical.rs:28-32, to_linear scene.rs:32-34
        kind, a, b, gamma, sc = self.bg
        if kind == BG_CONSTANT:
            return scale(sc, a)
        t = 0.5 * (d[1] + 1.0)
        c = add(scale(1.0 - t, a), scale(t, b))
        return scale(sc, (powf(c[0], gamma), powf(c[1], gamma), powf(c[2], gamma)))

    def patch(self, k, d, hp, mat, mut, M):
        """The material writes of analytical.rs:56-58 / 82-85 / 115-116 as an rpt_material patch."""
        mask, proc_kind, rgb, emission, fields, pp = self.materials[k]
        if mask & MAT_RGB:
            mat.rgb = rgb
        if mask & MAT_EMISSION:
            mat.emission = emission
        for bit, name in self.BITS:
            if mask & bit:
                setattr(mat, name, fields[name])
        if proc_kind == PROC_CHECKER_DIR:
            s, o = pp[0], pp[1]
            if "Q7_checker_by_hit_point" in mut:
                x, y = hp[0] * s + o, hp[2] * s + o
                cond = (1.0, 1.0)
            else:
                qx, qz = dv(d[0], d[1]) * s, dv(d[2], d[1]) * s
                x, y = qx + o, qz + o
                # a unit direction carries absolute rounding ~ulp(1) per component: the quotients move by (|q| + |s|) / |dir.y|
                # times that, which near the horizon is more than the checker's cells
                cond = (dv(abs(qx) + abs(s), abs(d[1])), dv(abs(qz) + abs(s), abs(d[1])))
            c = pp[2] if checker(x, y, M, cond) else pp[3]
            mat.rgb = (c, c, c)

    def closest_hit(self, o, d, st, ls, mut, M):
        """analytical.rs:36-127 over the descriptor's primitives, then Scene::sample_lights (scene.rs:36-86)."""
        dist = F_MAX
        hit = False
        first = True
        if self.large is not None:
            for k, t in self._large_hits(o, d, M):
                if first or t < dist:
                    hp = add(o, scale(t, d))
                    c = self.spheres[k][0]
                    st.hit_dist, st.normal = t, normalize(sub(hp, c))
                    self.patch(self.spheres[k][2], d, hp, st.material, mut, M)
                    hit, dist = True, t
                first = False
        else:
            for c, r, m in self.spheres:
                t = sphere(o, d, c, r, mut, M)
                if t is not None:
                    if not first:
                        M.rel(t, dist)
                    if first or t < dist:
                        hp = add(o, scale(t, d))
                        st.hit_dist, st.normal = t, normalize(sub(hp, c))
                        self.patch(m, d, hp, st.material, mut, M)
                        hit, dist = True, t
                first = False
        for n, p, md, m, mt in self.planes:
            t = plane(o, d, n, p, md, mt, M)
            if t is not None:
                if not first:
                    M.rel(t, dist)
                if first or t < dist:
                    st.hit_dist, st.normal = t, n
                    self.patch(m, d, add(o, scale(t, d)), st.material, mut, M)
                    hit, dist = True, t
            first = False
        if self.sample_lights(o, d, st, ls, mut, M):
            hit = True
        return hit

    def _large_hits(self, o, d, M):
        """Every sphere the ray hits, in table order, as (index, t) — only those a running `t < dist` could accept."""
        cs, rs = self.large
        lv = cs - np.array(o)
        tca = lv @ np.array(d)
        ll = (lv * lv).sum(axis=1)
        d2 = ll - tca * tca
        r2 = rs * rs
        with np.errstate(invalid="ignore", divide="ignore"):
            M.m = min(M.m, float(np.min(np.abs(d2 - r2) / np.maximum(ll, r2))))
            ok = d2 <= r2
            thc = np.sqrt(np.where(ok, r2 - d2, 0.0))
            t0, t1 = tca - thc, tca + thc
            s = np.maximum(np.abs(tca), thc)
            mt0 = np.abs(t0[ok]) / s[ok]
            M.m = min(M.m, float(mt0.min()) if mt0.size else INF)
            t = np.where(t0 < 0.0, t1, t0)
            inside = ok & (t0 < 0.0)
            if inside.any():
                M.m = min(M.m, float((np.abs(t1[inside]) / s[inside]).min()))
            ok &= t >= 0.0
        idx = np.nonzero(ok)[0]
        if idx.size == 0:
            return []
        tv = t[idx]
        prev = np.concatenate(([INF], np.minimum.accumulate(tv)[:-1]))
        keep = (tv < prev) | (idx == 0)
        if idx.size > 1:
            srt = np.sort(tv)
            M.rel(float(srt[0]), float(srt[1]))
        return [(int(k), float(x)) for k, x in zip(idx[keep], tv[keep])]

    def sample_lights(self, o, d, st, ls, mut, M):
        """scene.rs:36-86: starts from state.hit_dist as it stands (Q1)."""
        hit = False
        dist = st.hit_dist
        for typ, pos, em, u, v, radius, area in self.lights:
            if typ == LIGHT_SPHERICAL:
                t = sphere(o, d, pos, radius, mut, M)
                if t is not None:
                    M.rel(t, dist)
                    if t < dist:
                        dist = t
                        hp = add(o, scale(t, d))
                        cos_theta = dot(neg(d), normalize(sub(hp, pos)))
                        ls.pdf = dv(dist * dist, area * cos_theta * 0.5)
                        ls.emission = em
                        st.is_emitter = True
                        st.hit_dist = t
                        hit = True
            elif typ == LIGHT_RECTANGULAR and self.flags & SCENE_SAMPLE_ALL_LIGHT_TYPES:
                n = normalize(cross(u, v))
                dn = dot(n, d)
                M.of(dn, 1.0)
                if dn > 0.0:
                    continue
                t = dv(dot(n, pos) - dot(n, o), dn)
                if not t >= 0.0:
                    continue
                vi = sub(add(o, scale(t, d)), pos)
                a1 = dv(dot(u, vi), dot(u, u))
                a2 = dv(dot(v, vi), dot(v, v))
                for a in (a1, a2):
                    M.of(a, 1.0)
                    M.rel(a, 1.0)
                if 0.0 <= a1 <= 1.0 and 0.0 <= a2 <= 1.0:
                    M.rel(t, dist)
                    if t < dist:
                        dist = t
                        ls.pdf = dv(dist * dist, area * dot(neg(d), n))
                        ls.emission = em
                        st.is_emitter = True
                        st.hit_dist = t
                        hit = True
        return hit

    def any_hit(self, o, d, max_dist, mut, M):
        """analytical.rs:130-145 (Q3: max_dist ignored unless the scene says otherwise)."""
        use_max = bool(self.flags & SCENE_ANYHIT_USES_MAX_DIST) or "Q3_honoured" in mut
        if self.large is not None:
            hits = self._large_hits_all(o, d, M)
            for t in hits:
                if use_max:
                    M.rel(t, max_dist)
                if not use_max or t < max_dist:
                    return True
        else:
            for c, r, m in self.spheres:
                t = sphere(o, d, c, r, mut, M)
                if t is not None:
                    if use_max:
                        M.rel(t, max_dist)
                    if not use_max or t < max_dist:
                        return True
        for n, p, md, m, mt in self.planes:
            t = plane(o, d, n, p, md, mt, M)
            if t is not None:
                if use_max:
                    M.rel(t, max_dist)
                if not use_max or t < max_dist:
                    return True
        return False

    def _large_hits_all(self, o, d, M):
        cs, rs = self.large
        lv = cs - np.array(o)
        tca = lv @ np.array(d)
        ll = (lv * lv).sum(axis=1)
        d2 = ll - tca * tca
        r2 = rs * rs
        with np.errstate(invalid="ignore", divide="ignore"):
            M.m = min(M.m, float(np.min(np.abs(d2 - r2) / np.maximum(ll, r2))))
            ok = d2 <= r2
            thc = np.sqrt(np.where(ok, r2 - d2, 0.0))
            t0, t1 = tca - thc, tca + thc
            s = np.maximum(np.abs(tca), thc)
            if ok.any():
                M.m = min(M.m, float((np.abs(t0[ok]) / s[ok]).min()))
            t = np.where(t0 < 0.0, t1, t0)
            ok &= t >= 0.0
        return [float(x) for x in t[ok]]


def AnalyticalRef():
    """renderer/src/analytical.rs written out with no descriptor: its two spheres and their material writes (:41-58, :70-85), the
    plane y = -1 with |denom| > 0.0001 and the direction checker (:101-116, :193-204), one spherical light (3, 2, 2), r 1,
    emission 3 (:15-16; area 4 PI r^2, light.rs:22), the Pinhole defaults (pinhole.rs:14-25), eps 0.005 (tracer.rs:16), depth 4
    (scene.rs:28-30), the sky gradient (:28-32)."""
    s = DescScene.__new__(DescScene)
    s.flags = 0
    s.cam = ((0.0, 0.0, 3.0), (0.0, 0.0, 0.0), 80.0)
    s.bg = (BG_GRADIENT_Y, ONE3, (0.5, f32(0.7), 1.0), f32(2.2), 0.5)
    s.eps = f32(0.005)
    s.depth = 4
    s.spheres = [((f32(-1.1), 0.0, 0.0), 1.0, 0), ((f32(1.1), 0.0, 0.0), 1.0, 1)]
    s.planes = [((0.0, 1.0, 0.0), (0.0, -1.0, 0.0), f32(0.0001), 2, 0.0)]
    area = float(np.float32(4.0) * np.float32(math.pi) * np.float32(1.0) * np.float32(1.0))
    s.lights = [(LIGHT_SPHERICAL, (3.0, 2.0, 2.0), (3.0, 3.0, 3.0), ZERO3, ZERO3, 1.0, area)]
    z = dict(anisotropic=0.0, metallic=0.0, roughness=0.0, subsurface=0.0, specular_tint=0.0, sheen=0.0, sheen_tint=0.0, clearcoat=0.0,
             clearcoat_gloss=0.0, spec_trans=0.0, ior=0.0)
    s.materials = [
        (MAT_RGB | MAT_ROUGHNESS | MAT_METALLIC, 0, ONE3, ZERO3, dict(z, roughness=f32(0.05), metallic=1.0), (0.0,) * 4),
        (MAT_RGB | MAT_CLEARCOAT | MAT_CLEARCOAT_GLOSS | MAT_ROUGHNESS, 0, (1.0, f32(0.186), 0.0), ZERO3,
         dict(z, clearcoat=1.0, clearcoat_gloss=1.0, roughness=f32(0.1)), (0.0,) * 4),
        (MAT_ROUGHNESS, PROC_CHECKER_DIR, ZERO3, ZERO3, dict(z, roughness=1.0), (0.5, 100.0, 0.25, f32(0.1))),
    ]
    s.large = None
    return s


# ---- the tracer -------------------------------------------------------------------------------------------------------------
class State:                                    # globals.rs:18-41 (State::new)
    __slots__ = ("eta", "hit_dist", "fhp", "normal", "ffnormal", "is_emitter", "material")

    def __init__(self):
        self.eta = 0.0
        self.hit_dist = -1.0
        self.fhp = ZERO3
        self.normal = ZERO3
        self.ffnormal = ZERO3
        self.is_emitter = False
        self.material = None


class LightSampleRec:                           # globals.rs:100-121
    __slots__ = ("normal", "emission", "direction", "dist", "pdf")

    def __init__(self):
        self.normal = ZERO3
        self.emission = ZERO3
        self.direction = ZERO3
        self.dist = 0.0
        self.pdf = 0.0


def sample_light(scene, light, scatter_pos, draw, M=None):
    """tracer.rs:173-220 (spherical) + include/rpt.h's rectangular / distant lights under RPT_SCENE_SAMPLE_ALL_LIGHT_TYPES."""
    M = M or Margin()
    typ, pos, em, u, v, radius, area = light
    ls = LightSampleRec()
    nl = float(len(scene.lights))
    if typ == LIGHT_SPHERICAL:
        r1 = draw()
        r2 = draw()
        sctc = sub(scatter_pos, pos)
        dist_c = length(sctc)
        r = sqrt(fmax(0.0, 1.0 - r1 * r1))              # uniform_sample_hemisphere, :178-182
        phi = TWO_PI * r2
        sd = (r * cos(phi), r * sin(phi), r1)
        sctc = div3(sctc, (dist_c, dist_c, dist_c))
        t, b = onb(sctc, M)
        sd = add(add(scale(sd[0], t), scale(sd[1], b)), scale(sd[2], sctc))
        lsp = add(pos, scale(radius, sd))
        direction = sub(lsp, scatter_pos)
        ls.dist = length(direction)
        dist_sq = ls.dist * ls.dist
        ls.direction = div3(direction, (ls.dist, ls.dist, ls.dist))
        ls.normal = normalize(sub(lsp, pos))
        ls.emission = scale(nl, em)
        ls.pdf = dv(dist_sq, area * 0.5 * abs(dot(ls.normal, ls.direction)))
    elif scene.flags & SCENE_SAMPLE_ALL_LIGHT_TYPES:
        if typ == LIGHT_RECTANGULAR:
            r1 = draw()
            r2 = draw()
            lsp = add(add(pos, scale(r1, u)), scale(r2, v))
            direction = sub(lsp, scatter_pos)
            ls.dist = length(direction)
            dist_sq = ls.dist * ls.dist
            ls.direction = div3(direction, (ls.dist, ls.dist, ls.dist))
            ls.normal = normalize(cross(u, v))
            ls.emission = scale(nl, em)
            ls.pdf = dv(dist_sq, area * abs(dot(ls.normal, ls.direction)))
        else:
            ls.direction = normalize(pos)
            ls.normal = normalize(sub(scatter_pos, pos))
            ls.emission = scale(nl, em)
            ls.dist = INF
            ls.pdf = 1.0
    return ls


class Path:
    """One pixel-sample: Tracer::render's closure body (tracer.rs:33-105) up to `color`."""

    def __init__(self, scene, mut=(), roulette=False):
        for m in mut:
            assert m in MUTANTS, m
        self.scene = scene
        self.mut = frozenset(mut)
        self.roulette = roulette
        self.eps = f32(0.001) if "eps_0.001" in self.mut else scene.eps

    def direct_light(self, d, st, draw, M, rays):      # tracer.rs:126-170
        sc, mut = self.scene, self.mut
        ld = ZERO3
        scatter_pos = add(st.fhp, scale(self.eps, st.ffnormal))
        n = len(sc.lights)
        if n > 0:
            random = draw() * float(n)
            k = round(random)
            if 1 <= k <= n - 1:
                M.rel(random, float(k))                      # the light index's boundaries (Q14)
            index = min(int(random), n - 1)               # `as usize`; index n (f32 rounding only) is taken as n - 1
            light = sc.lights[index]
            ls = sample_light(sc, light, scatter_pos, draw, M)
            li = ls.emission
            fac = dot(ls.direction, ls.normal)
            M.of(fac, 1.0)
            if fac < 0.0:
                max_dist = ls.dist - self.eps
                rays.append(scatter_pos + ls.direction + (max_dist,))
                if not sc.any_hit(scatter_pos, ls.direction, max_dist, mut, M):
                    f, pdf = disney_eval(st.material, st.eta, neg(d), st.ffnormal, ls.direction, mut, M)
                    mis = 1.0
                    if light[6] > 0.0:
                        mis = power_heuristic(ls.pdf, pdf, mut)
                    if pdf > 0.0:
                        ld = add(ld, scale(mis, mul(li, div3(f, (ls.pdf, ls.pdf, ls.pdf)))))
        return ld

    def sample(self, col, row, width, height, draws):
        """-> (radiance, rays, margin).  col, row: the pixel in the top-down buffer; draws: the path's stream (enough of it)."""
        sc, mut = self.scene, self.mut
        M = Margin()
        rays = []
        it = iter(draws)
        draw = lambda: float(next(it))                   # noqa: E731
        # tracer.rs:29-40: par_rchunks_exact_mut hands out rows from the END of the buffer: chunk j = 0 is the last row
        j = height - 1 - row
        x = float(col)
        y = float(height) - float(j)
        xx = x / width
        yy = y / height
        a = draw()
        b = draw()
        cam_offset = (b, a) if "jitter_swapped" in mut else (a, b)
        coord = (xx, yy if "image_not_flipped" in mut else 1.0 - yy)
        o, d = gen_ray(sc.cam, coord, cam_offset, float(width), float(height))
        radiance = ZERO3
        throughput = ONE3
        st = State()
        ls = LightSampleRec()
        ss_l, ss_pdf = ZERO3, 0.0                        # ScatterSampleRec::new
        depth = sc.depth                                 # state.depth = recursion_depth(), constant (Q2)
        for bounce in range(depth):
            st.material = Material(1.0 if "Q12_rgb_one" in mut else 1.5)
            if "Q1_hit_dist_reset" in mut:
                st.hit_dist = F_MAX
            rays.append(o + d + (-1.0,))
            if not sc.closest_hit(o, d, st, ls, mut, M):
                radiance = add(radiance, mul(sc.background(d), throughput))
                break
            # State::finalize, globals.rs:50-62
            st.fhp = add(o, scale(st.hit_dist, d))
            nd = dot(st.normal, d)
            M.of(nd, 1.0)
            st.ffnormal = st.normal if nd <= 0.0 else neg(st.normal)
            st.material.finalize()
            st.eta = dv(1.0, st.material.ior) if nd < 0.0 else st.material.ior
            radiance = add(radiance, mul(st.material.emission, throughput))
            if st.is_emitter:
                mis = 1.0
                if (bounce > 0) if "Q2_mis_past_bounce0" in mut else (depth > 0):
                    mis = power_heuristic(ss_pdf, ls.pdf, mut)
                radiance = add(radiance, mul(scale(mis, ls.emission), throughput))
                break
            radiance = add(radiance, mul(self.direct_light(d, st, draw, M, rays), throughput))
            f, ss_l, ss_pdf = disney_sample(st.material, st.eta, neg(d), st.ffnormal, ss_l, draw, mut, M)
            if ss_pdf > 0.0:
                throughput = mul(throughput, div3(f, (ss_pdf, ss_pdf, ss_pdf)))
            else:
                break
            d = ss_l
            o = add(st.fhp, scale(self.eps, st.ffnormal if "Q8_offset_ffnormal" in mut else d))
            if self.roulette and 2 <= bounce + 1 < depth:      # include/rpt.h, RPT_RENDER_RUSSIAN_ROULETTE
                q = clamp(fmax(fmax(throughput[0], throughput[1]), throughput[2]), f32(0.05), 1.0)
                r = draw()
                M.rel(r, q)
                if r >= q:
                    break
                throughput = div3(throughput, (q, q, q))
        return radiance, rays, M.m


def sample_many(scene, oracle, seed, items, width, height, mut=(), roulette=False, n_draws=96):
    """items: (col, row, frame) triples -> (radiance [n, 3], margins [n], rays list).  Draws from oracle.rng_f32."""
    path = Path(scene, mut, roulette)
    out = np.zeros((len(items), 3))
    marg = np.zeros(len(items))
    rays = []
    for k, (c, r, f) in enumerate(items):
        dr = oracle.rng_f32(seed, int(f), int(r) * width + int(c), n_draws)
        noise_begin(seed, int(f), int(r) * width + int(c))
        rad, ry, m = path.sample(int(c), int(r), width, height, dr)
        out[k] = rad
        marg[k] = m
        rays.append(ry)
    return out, marg, rays
