"""The mesh features of include/rpt.h ("smooth mesh shading" to "mesh normal maps") restated once in float64, and their composition.

First the statements, each as ONE function that every float64 restatement of a mesh feature calls — the single-feature classes of
tests/test_gpu_mesh_{light,env,texture,cutout,normal_map}_f64.py and the composed class below alike: the texture decode and lookup with
its NEAREST margins (decode_texture_f64, tex_axis, tex_lookup), the cut test as the last line of the triangle test (cut_test), the
normal map's decode and the bend (decode_normal_map_f64, bend), the mesh-light table and sampler and the hit-side weight
(bind_mesh_lights, sample_mesh_light, hit_weight), the environment's lookup, sampler, pdf and miss-side weight (bind_environment,
env_lookup, sample_env, env_pdf, miss), direct_light over the pickable lights and the path loop (direct_light, trace).  The smooth
normal stays where it was (test_gpu_mesh_smooth_f64.SmoothMeshDescScene.barycentrics / interpolated_normal).

Then ComposedMeshDescScene and ComposedPath: one pixel-sample with every feature active at once, written from include/rpt.h's wording.
Per mesh FLAT or SMOOTH, OFF or ON, a texture or none, a cutout or none, a normal map or none; per scene an environment or none.  The
arguments are the very dicts Tracer.set_mesh_textures / set_mesh_cutouts / set_mesh_normal_maps take, so a test hands one value to
both sides.  The composition rules, each where the code applies it:

  * shading normal (shading_normal): flat or smooth per mesh, then the bend if the mesh has a map; the bend's N is that normal, e1, e2
    and the UVs are the triangle's                                                              ("mesh normal maps": Bend, "N is the
    normal the hit would have had without the map"; "bends the SHADING normal — the flat one, or smooth mesh shading's")
  * mesh-light sampler and hit-side weight: the flat normal of the triangle, whatever the shading normal is
                                                                                                ("mesh lights": "sampling and lp use
    the flat normal, shading the normal the mesh's mode says"; "mesh normal maps": "Unchanged: ... the mesh-light sampler and hit
    weight (which use the flat normal)")
  * cut test (_triangles): inside closest_hit and any_hit alike, for meshes with a cutout only, through the TEXTURE's UVs and wrap and
    the MASK's own W x H, always NEAREST; a shadow ray toward the environment has max_dist = inf - eps, so a triangle occludes it
    unless the ray passes a hole                                                                ("mesh cutouts": Cut test, "closest_hit
    and any_hit are unchanged in wording: they use the triangle test"; "environment lighting": dist = +inf)
  * base colour (patch): rgb = material.rgb * tex on textured meshes only, emission untouched   ("mesh textures": Scope)
  * pick count (ComposedPath.picks): N = n_lights + ON meshes + (1 if SAMPLED), the environment last; every pick's emission is
    scaled by that N                                                                            ("environment lighting": Pickable lights)
  * margins: the union of what the single-feature restatements record — texel borders for NEAREST (textures, masks, NEAREST maps),
    the sign of D, dot(B, B0), both l2 guards of the bend, the smooth l2, the CDF picks, the environment's folds and borders, the
    sampler's `c > 0`, the hit side's c, and the facing test.

Faults a device could have in exactly one interaction are planted by keyword arguments, as fault= / no_hit_weight= are in the
single-feature files; tests/test_gpu_mesh_compose_f64.py holds each to the draws that must see it.  Three subtle ones, wrong in the
second or third digit, are held to the samples' own f32 tolerances there (tests/f32_spread.py): ComposedPath's mesh_light_pdf_scale,
the scene attribute env_pdf_from_next_row and this module's BILINEAR_SHIFT.

Under pt_f64's noise mode the outputs computed here outside pt_f64's helpers, which the device computes in f32, carry the same
noise: interp_uv's (s, t), the BILINEAR blends of tex_lookup (a NEAREST value is a table entry and is not perturbed), the bend's T,
B and result, env_pdf, the mesh-light sampler's barycentrics, and the textured rgb; the triangle test's t, u and v term by term
(test_gpu_mesh_f64.MeshDescScene.noisy_tuv).  With the mode off every function returns the bits it returned before."""
import bisect
import math

import numpy as np

import pt_f64 as P
from test_gpu_mesh_smooth_f64 import SmoothMeshDescScene
from test_mesh_env_host import restate_table as restate_env_table
from test_mesh_light_host import restate_table as restate_light_table

REPEAT, CLAMP, NEAREST, BILINEAR = 0, 1, 0, 1
WRAPS = {"repeat": REPEAT, "clamp": CLAMP}
FILTERS = {"nearest": NEAREST, "bilinear": BILINEAR}
N_DRAWS = 128
BILINEAR_SHIFT = 0.0                                                  # a planted fault: the BILINEAR lookup shifted by this many texels


# ---- the triangle's own quantities ------------------------------------------------------------------------------------------------
def flat_normal(sc, k):
    """normalize(cross(e1, e2)) of triangle k's row."""
    return P.normalize(tuple(float(x) for x in np.cross(sc.e1[k], sc.e2[k])))


def interp_uv(sc, k, u, v):
    """include/rpt.h, "mesh textures", lookup at the hit: (s, t) from the corners' UVs and the triangle test's u and v."""
    ua, ub, uc = (sc.uv[j] for j in sc.corner[k])
    s, t = ((1.0 - u) - v) * ua + u * ub + v * uc
    return P.noisy(float(s)), P.noisy(float(t))


# ---- mesh textures ------------------------------------------------------------------------------------------------------------------
def decode_texture_f64(rgba, gamma):
    """include/rpt.h's decode in float64: [h, w, 3]."""
    table = np.array([0.0 if k == 0 else 1.0 if k == 255 else P.powf(k / 255.0, gamma) for k in range(256)])
    if gamma == 1.0:
        table = np.arange(256) / 255.0
    return table[np.asarray(rgba, np.uint8)[..., :3]]


def tex_axis(s, n, wrap, filt, M):
    """One axis of tex_wrap and the filter's index -> (i, None, None) for NEAREST, (i0, i1, f) for BILINEAR.  NEAREST records the
    distance of x * n to the next integer where the coordinate is not clamped; BILINEAR is continuous and records nothing."""
    x = min(max(s, 0.0), 1.0) if wrap == CLAMP else s - np.floor(s)
    p = x * n
    if filt == NEAREST:
        if wrap == REPEAT or 0.0 < s < 1.0:
            M.of(p - np.round(p), 1.0)
        i = int(np.floor(p))
        return (min(i, n - 1) if wrap == CLAMP else i % n), None, None
    p -= 0.5 - BILINEAR_SHIFT
    f0 = np.floor(p)
    i0, i1 = int(f0), int(f0) + 1
    if wrap == CLAMP:
        return min(max(i0, 0), n - 1), min(max(i1, 0), n - 1), p - f0
    return i0 % n, i1 % n, p - f0


def tex_lookup(texels, s, t, wrap, filt, M):
    """tex_lookup over [h, w, c] float64 texels (a decoded texture or a decoded normal map)."""
    h, w = texels.shape[:2]
    i0, i1, fx = tex_axis(s, w, wrap, filt, M)
    j0, j1, fy = tex_axis(t, h, wrap, filt, M)
    if filt == NEAREST:
        return texels[j0, i0]                                         # (a table value: never perturbed)
    top = P.noisy_array((1.0 - fx) * texels[j0, i0] + fx * texels[j0, i1])
    bot = P.noisy_array((1.0 - fx) * texels[j1, i0] + fx * texels[j1, i1])
    return P.noisy_array((1.0 - fy) * top + fy * bot)


# ---- mesh cutouts -------------------------------------------------------------------------------------------------------------------
def cut_test(sc, hit, o, d, M, cut_of, swap=False):
    """include/rpt.h, "cut test": the triangle test's last line, applied in place to `hit` — a triangle that passes everything else
    misses where its mesh's mask has a hole.  cut_of(k) -> (opaque bits [H, W], the texture's wrap), or None for a triangle whose
    mesh has no cutout.  The mask is a step function: the NEAREST margins of both axes are recorded for every such triangle."""
    for k in np.nonzero(hit)[0]:
        cut = cut_of(int(k))
        if cut is None:
            continue
        bits, wrap = cut
        s, t = interp_uv(sc, k, *sc.barycentrics(k, o, d))
        if swap:
            s, t = t, s
        h, w = bits.shape
        i = tex_axis(s, w, wrap, NEAREST, M)[0]
        j = tex_axis(t, h, wrap, NEAREST, M)[0]
        if not bits[j, i]:
            hit[k] = False
    return hit


# ---- mesh normal maps ---------------------------------------------------------------------------------------------------------------
def decode_normal_map_f64(rgba, strength=1.0, flip_green=False):
    """include/rpt.h's decode in float64: [h, w, 3] = {sx c(R), sy c(G), c(B)}, c(k) = max((k - 128) / 127, -1)."""
    c = np.maximum((np.asarray(rgba, np.uint8)[..., :3].astype(np.float64) - 128.0) / 127.0, -1.0)
    sx = float(np.float32(strength))
    c[..., 0] *= sx
    c[..., 1] *= -sx if flip_green else sx
    return c


def bend(N, e1, e2, ua, ub, uc, xyz, M, swap=False):
    """include/rpt.h, "Bend": N the normal the hit would have had without the map (a float64 array), e1, e2 the triangle row's,
    ua, ub, uc the corners' UVs, xyz the map's value -> the bent normal as a tuple.  Records the sign of D, the sign of dot(B, B0)
    and both `l2 > 0` guards.  swap: T and B change places (a planted fault)."""
    x, y, z = xyz
    if x == 0.0 and y == 0.0:
        return tuple(float(c) for c in N)
    (du1, dv1), (du2, dv2) = ub - ua, uc - ua
    D = du1 * dv2 - du2 * dv1
    M.of(D, abs(du1 * dv2) + abs(du2 * dv1))
    if not (D < 0.0 or D > 0.0):
        return tuple(float(c) for c in N)
    g = 1.0 if D > 0.0 else -1.0
    T0, B0 = g * (e1 * dv2 - e2 * dv1), g * (e2 * du1 - e1 * du2)
    T1 = T0 - N * float((N * T0).sum())
    l2 = float((T1 * T1).sum())
    M.of(l2, float((T0 * T0).sum()))
    if not l2 > 0.0:
        return tuple(float(c) for c in N)
    T = P.noisy_array(T1 / np.sqrt(l2))
    B = P.noisy_array(np.cross(N, T))
    side = float((B * B0).sum())
    M.of(side, float(np.sqrt((B0 * B0).sum())))
    if side < 0.0:
        B = -B
    if swap:
        T, B = B, T
    m = x * T + y * B + z * N
    l2 = float((m * m).sum())
    M.of(l2, x * x + y * y + z * z)
    if not l2 > 0.0:
        return tuple(float(c) for c in N)
    return tuple(float(c) for c in P.noisy_array(m / np.sqrt(l2)))


# ---- mesh lights --------------------------------------------------------------------------------------------------------------------
def bind_mesh_lights(sc, desc, scene, on):
    """Gives the scene restatement `sc` the ON meshes' tables: tri_ord (triangle -> ordinal of its ON mesh, or -1) and mesh_lights,
    ordinal -> (cdf list, Q, A_tot, corners f64 [n, 3, 3], emission, first flattened triangle).  The INTEGER table is
    tests/test_mesh_light_host.py's restatement: the integers are the device's by construction."""
    sc.tri_ord = np.concatenate([np.full(len(t), sorted(on).index(m) if m in on else -1) for m, (_, t, _) in enumerate(scene.meshes)])
    first = np.cumsum([0] + [len(t) for _, t, _ in scene.meshes])
    sc.mesh_lights = []
    for m in sorted(on):
        v, t, mat = scene.meshes[m]
        cdf, _, a_tot = restate_light_table(v, t)
        tri = np.asarray(v, np.float32)[np.asarray(t, np.int64)].astype(np.float64)
        em = tuple(float(x) for x in desc.materials[mat].emission)
        sc.mesh_lights.append(([int(c) for c in cdf], int(cdf[-1]) if len(cdf) else 0, float(a_tot), tri, em, int(first[m])))
    sc.won = None


def sample_mesh_light(sc, ordinal, n_f, scatter_pos, draw, M, normal_of=None, pdf_scale=1.0):
    """include/rpt.h, "sampling an ON mesh" -> (LightSampleRec, light.area).  n_f: N_f, the number of pickable lights.  normal_of
    (a planted fault): (flattened triangle, bu, bv) -> the normal to use where the flat one belongs; pdf_scale (another): the pdf times it."""
    cdf, q_all, a_tot, tri, em, first = sc.mesh_lights[ordinal]
    r0a, r0b, r1, r2 = draw(), draw(), draw(), draw()
    ls = P.LightSampleRec()
    if not a_tot > 0.0:
        return ls, 0.0
    j = (int(r0a * 16777216.0) << 24) | int(r0b * 16777216.0)
    t = (j * q_all) >> 48
    k = bisect.bisect_right(cdf, t)                                   # the first index with C_k > T
    below = cdf[k - 1] if k else 0
    M.of(min(t - below + 1, cdf[k] - t) / float(cdf[k] - below), 1.0)         # the pick: integer steps to the neighbours, over q_k
    a, b, c = (tuple(float(x) for x in p) for p in tri[k])
    e1, e2 = P.sub(b, a), P.sub(c, a)
    su = P.sqrt(r1)
    bu = P.noisy(1.0 - su)
    bv = P.noisy(r2 * su)
    p = P.add(P.add(a, P.scale(bu, e1)), P.scale(bv, e2))
    direction = P.sub(p, scatter_pos)
    ls.dist = P.length(direction)
    dist_sq = ls.dist * ls.dist
    ls.direction = P.div3(direction, (ls.dist, ls.dist, ls.dist))
    n = P.normalize(P.cross(e1, e2)) if normal_of is None else normal_of(first + k, bu, bv)
    cs = P.dot(n, ls.direction)
    M.of(cs, 1.0)                                                     # the `c > 0` turn
    ls.normal = P.neg(n) if cs > 0.0 else n
    ls.emission = P.scale(n_f, em)
    ls.pdf = P.dv(dist_sq, a_tot * abs(cs))
    if pdf_scale != 1.0:
        ls.pdf *= pdf_scale
    return ls, a_tot


def hit_weight(sc, bounce, d, st, ss_pdf, mut, M, normal=None):
    """include/rpt.h, "hit side": the weight of the hit's emission term.  normal (a planted fault): used where n_flat belongs."""
    if bounce == 0 or sc.won is None or sc.tri_ord[sc.won] < 0:
        return 1.0
    a_tot = sc.mesh_lights[int(sc.tri_ord[sc.won])][2]
    if not a_tot > 0.0:
        return 1.0
    cs = abs(P.dot(d, flat_normal(sc, sc.won) if normal is None else normal))
    M.of(cs, 1.0)
    if not cs > 0.0:
        return 1.0
    lp = P.dv(st.hit_dist * st.hit_dist, a_tot * cs)
    return P.power_heuristic(ss_pdf, lp, mut)


# ---- environment lighting -----------------------------------------------------------------------------------------------------------
def _sgn(x):
    return 1.0 if x >= 0.0 else -1.0


def bind_environment(sc, image, scale=1.0, sampled=True):
    """Gives the scene restatement `sc` the environment: the f32 texels as float64 and the INTEGER table (tests/test_mesh_env_host.py's
    restatement: the integers are the device's by construction).  image None: no environment is set."""
    sc.env_set = image is not None
    if image is None:
        sc.env_size, sc.env_rgb, sc.env_cdf, sc.env_q, sc.env_scale, sc.env_sampled = 0, [], [], 0, 0.0, False
        return
    texels, cdf, _ = restate_env_table(image, sampled)
    sc.env_size = int(np.asarray(image).shape[0])
    sc.env_rgb = [tuple(float(x) for x in c[:3]) for c in texels]
    sc.env_cdf = [int(c) for c in cdf]
    sc.env_q = sc.env_cdf[-1] if sampled else 0
    sc.env_scale = float(np.float32(scale))
    sc.env_sampled = bool(sampled)


def env_quantum(sc, k):
    return sc.env_cdf[k] - (sc.env_cdf[k - 1] if k else 0)


def env_pdf(sc, k, p):
    s_f = float(sc.env_size)
    l2 = P.dot(p, p)
    ln = P.sqrt(l2)
    if getattr(sc, "env_pdf_from_next_row", False):                  # a planted fault: the neighbouring texel row's quantum
        k = k + sc.env_size if k + sc.env_size < sc.env_size * sc.env_size else k - sc.env_size
    sel = P.dv(float(env_quantum(sc, k)), float(sc.env_q))
    return P.noisy((sel * ((s_f * s_f) * 0.25)) * (l2 * ln)), ln


def env_lookup(sc, d, M):
    """include/rpt.h, "lookup of a direction" -> (k or None, radiance, p before the fold)."""
    size, s_f = sc.env_size, float(sc.env_size)
    l1 = (abs(d[0]) + abs(d[1])) + abs(d[2])
    if not (l1 > 0.0 and l1 <= 3.40282347e+38):
        return None, P.ZERO3, P.ZERO3
    px, pz = d[0] / l1, d[2] / l1
    p = (px, d[1] / l1, pz)
    M.of(p[1], 1.0)                                                   # the fold: d.y < 0
    if d[1] < 0.0:
        px, pz = (1.0 - abs(pz)) * _sgn(px), (1.0 - abs(px)) * _sgn(pz)
    idx = []
    for x in (px * 0.5 + 0.5, pz * 0.5 + 0.5):
        xs = x * s_f
        border = round(xs)
        if 1 <= border <= size - 1:
            M.of(xs - border, 1.0)                                    # a texel border
        idx.append(min(int(math.floor(xs)), size - 1))
    k = idx[1] * size + idx[0]
    return k, P.scale(sc.env_scale, sc.env_rgb[k]), p


def sample_env(sc, n_f, draw, M):
    """include/rpt.h, "sampling from scatter_pos" -> (LightSampleRec, light.area).  n_f: N_f, the number of pickable lights."""
    r0a, r0b, r1, r2 = draw(), draw(), draw(), draw()
    ls = P.LightSampleRec()
    if sc.env_q == 0:
        return ls, 1.0
    size, s_f = sc.env_size, float(sc.env_size)
    j = (int(r0a * 16777216.0) << 24) | int(r0b * 16777216.0)
    t = (j * sc.env_q) >> 48
    k = bisect.bisect_right(sc.env_cdf, t)                            # the first index with C_k > T
    below = sc.env_cdf[k - 1] if k else 0
    M.of(min(t - below + 1, sc.env_cdf[k] - t) / float(sc.env_cdf[k] - below), 1.0)
    s, tt = (float(k % size) + r1) / s_f, (float(k // size) + r2) / s_f
    px, pz = s * 2.0 - 1.0, tt * 2.0 - 1.0
    py = (1.0 - abs(px)) - abs(pz)
    M.of(py, 1.0)                                                     # the sampler's fold
    if py < 0.0:
        px, pz = (1.0 - abs(pz)) * _sgn(px), (1.0 - abs(px)) * _sgn(pz)
    p = (px, py, pz)
    ls.pdf, ln = env_pdf(sc, k, p)
    ls.direction = P.div3(p, (ln, ln, ln))
    ls.normal = P.neg(ls.direction)
    ls.dist = P.INF
    ls.emission = P.scale(n_f, P.scale(sc.env_scale, sc.env_rgb[k]))
    return ls, 1.0


def miss(sc, bounce, d, ss_pdf, mut, M, no_weight=False):
    """include/rpt.h, "miss side": w * radiance(d).  no_weight: a planted fault."""
    k, rad, p = env_lookup(sc, d, M)
    w = 1.0
    if not (no_weight or bounce == 0 or k is None or sc.env_q == 0 or env_quantum(sc, k) == 0):
        lp, _ = env_pdf(sc, k, p)
        if lp != 0.0:
            w = P.power_heuristic(ss_pdf, lp, mut)
    return P.scale(w, rad)


# ---- the integrator over the pickable lights --------------------------------------------------------------------------------------
def direct_light(path, d, st, draw, M, rays):
    """tracer.rs:126-170 over path.picks(), the N pickable lights in index order: ("light", rpt_light), ("mesh", ordinal) or
    ("env", None).  N_f takes the place of n_lights as F for every kind of pick (include/rpt.h, "pickable lights")."""
    sc, mut = path.scene, path.mut
    ld = P.ZERO3
    scatter_pos = P.add(st.fhp, P.scale(path.eps, st.ffnormal))
    picks = path.picks()
    n = len(picks)
    if n > 0:
        random = draw() * float(n)
        k = round(random)
        if 1 <= k <= n - 1:
            M.rel(random, float(k))
        index = min(int(random), n - 1)
        kind, what = picks[index]
        if kind == "light":
            ls = P.sample_light(sc, what, scatter_pos, draw, M)
            if what[0] == P.LIGHT_SPHERICAL or sc.flags & P.SCENE_SAMPLE_ALL_LIGHT_TYPES:
                ls.emission = P.scale(float(n), what[2])               # N_f takes the place of n_lights as F
            area = what[6]
        elif kind == "mesh":
            ls, area = path.sample_mesh_light(what, scatter_pos, draw, M)
        else:
            ls, area = path.sample_env(draw, M)
        li = ls.emission
        fac = P.dot(ls.direction, ls.normal)
        M.of(fac, 1.0)                                                # the facing test
        if fac < 0.0:
            max_dist = ls.dist - path.eps                             # (the environment's: inf - eps)
            rays.append(scatter_pos + ls.direction + (max_dist,))
            if not sc.any_hit(scatter_pos, ls.direction, max_dist, mut, M):
                f, pdf = P.disney_eval(st.material, st.eta, P.neg(d), st.ffnormal, ls.direction, mut, M)
                mis = 1.0
                if area > 0.0:
                    mis = P.power_heuristic(ls.pdf, pdf, mut)
                if pdf > 0.0:
                    ld = P.add(ld, P.scale(mis, P.mul(li, P.div3(f, (ls.pdf, ls.pdf, ls.pdf)))))
    return ld


def trace(path, col, row, width, height, draws):
    """pt_f64.Path.sample (its mutants left out) with the hit-side weight on the emission term (path.hit_weight), what a miss adds
    (path.miss) and next-event estimation over the pickable lights (path.direct_light) -> (radiance, rays, margin)."""
    assert not path.mut and not path.roulette
    sc, mut = path.scene, path.mut
    M = P.Margin()
    rays = []
    it = iter(draws)
    draw = lambda: float(next(it))                                    # noqa: E731
    j = height - 1 - row
    x = float(col)
    y = float(height) - float(j)
    a = draw()
    b = draw()
    o, d = P.gen_ray(sc.cam, (x / width, 1.0 - y / height), (a, b), float(width), float(height))
    radiance = P.ZERO3
    throughput = P.ONE3
    st = P.State()
    ls = P.LightSampleRec()
    ss_l, ss_pdf = P.ZERO3, 0.0
    depth = sc.depth
    for bounce in range(depth):
        st.material = P.Material(1.5)
        rays.append(o + d + (-1.0,))
        if not sc.closest_hit(o, d, st, ls, mut, M):
            radiance = P.add(radiance, P.mul(path.miss(bounce, d, ss_pdf, M), throughput))
            break
        st.fhp = P.add(o, P.scale(st.hit_dist, d))
        nd = P.dot(st.normal, d)
        M.of(nd, 1.0)
        st.ffnormal = st.normal if nd <= 0.0 else P.neg(st.normal)
        st.material.finalize()
        st.eta = P.dv(1.0, st.material.ior) if nd < 0.0 else st.material.ior
        w = path.hit_weight(bounce, d, st, ss_pdf, M)
        radiance = P.add(radiance, P.mul(P.scale(w, st.material.emission), throughput))
        if st.is_emitter:
            mis = P.power_heuristic(ss_pdf, ls.pdf, mut) if depth > 0 else 1.0
            radiance = P.add(radiance, P.mul(P.scale(mis, ls.emission), throughput))
            break
        radiance = P.add(radiance, P.mul(path.direct_light(d, st, draw, M, rays), throughput))
        f, ss_l, ss_pdf = P.disney_sample(st.material, st.eta, P.neg(d), st.ffnormal, ss_l, draw, mut, M)
        if ss_pdf > 0.0:
            throughput = P.mul(throughput, P.div3(f, (ss_pdf, ss_pdf, ss_pdf)))
        else:
            break
        d = ss_l
        o = P.add(st.fhp, P.scale(path.eps, d))
    return radiance, rays, M.m


def sample_pixels(path, oracle, seed, pixels, w, h, frame=0):
    """One sample of each of `pixels` [(col, row)] through `path`, of frame `frame` -> (radiance [n, 3], margins [n]).  The oracle
    only supplies the random draws (rng_f32)."""
    out, marg = np.zeros((len(pixels), 3)), np.zeros(len(pixels))
    for k, (c, r) in enumerate(pixels):
        dr = oracle.rng_f32(seed, frame, int(r) * w + int(c), N_DRAWS)
        P.noise_begin(seed, frame, int(r) * w + int(c))
        out[k], _, marg[k] = path.sample(int(c), int(r), w, h, dr)
    return out, marg


# ---- every feature at once ----------------------------------------------------------------------------------------------------------
class ComposedMeshDescScene(SmoothMeshDescScene):
    """The scene with the meshes `smooth` SMOOTH and the meshes `on` ON; `textures`, `cutouts` and `normal_maps` as
    Tracer.set_mesh_textures / set_mesh_cutouts / set_mesh_normal_maps take them ({mesh: dict or array}); `environment` None or
    dict(image=, scale=, sampled=) as Tracer.set_environment's arguments.

    Planted faults, each in one interaction: bend_from_flat (the bend starts from the flat normal on a SMOOTH mesh), map_wrap_clamp
    (the map is looked up with CLAMP where the texture's wrap belongs), no_cut_in_any_hit (the cut test is applied in closest_hit
    but not in any_hit), no_texture_under_env (the texture is dropped while an environment is set)."""

    def __init__(self, desc, scene, smooth=(), on=(), textures=None, cutouts=None, normal_maps=None, environment=None,
                 bend_from_flat=False, map_wrap_clamp=False, no_cut_in_any_hit=False, no_texture_under_env=False):
        super().__init__(desc, scene)
        self.bend_from_flat, self.map_wrap_clamp = bend_from_flat, map_wrap_clamp
        self.no_cut_in_any_hit, self.no_texture_under_env = no_cut_in_any_hit, no_texture_under_env
        textures, cutouts, normal_maps = textures or {}, cutouts or {}, normal_maps or {}
        meshes = list(enumerate(scene.meshes))
        self.tri_mesh = np.concatenate([np.full(len(t), m) for m, (_, t, _) in meshes])
        self.smooth_tri = np.concatenate([np.full(len(t), m in smooth) for m, (_, t, _) in meshes])
        bind_mesh_lights(self, desc, scene, on)
        bind_environment(self, **(environment or dict(image=None)))
        # one UV per vertex, flattened like self.vn (an untextured mesh's are never read)
        self.uv = np.concatenate([np.asarray(textures[m]["uvs"], np.float32).reshape(-1, 2) if m in textures else np.zeros((len(v), 2))
                                  for m, (v, _, _) in meshes]).astype(np.float64)
        self.tex, self.cut, self.maps = {}, {}, {}
        for m, tex in textures.items():
            wrap, filt = WRAPS[tex.get("wrap", "repeat")], FILTERS[tex.get("filter", "bilinear")]
            self.tex[m] = (decode_texture_f64(tex["texels"], float(tex.get("gamma", 1.0))), wrap, filt)
        for m, cut in cutouts.items():
            assert m in self.tex, "a cutout needs the mesh's UVs (include/rpt.h, \"mesh cutouts\": Composition)"
            assert m not in on, "a cutout mesh cannot be a mesh light (include/rpt.h, \"mesh cutouts\": Composition)"
            alpha, threshold = (cut["alpha"], cut.get("threshold", 128)) if isinstance(cut, dict) else (cut, 128)
            self.cut[m] = np.asarray(alpha, np.uint8) >= threshold     # bit k = alpha[k] >= threshold: OPAQUE
        for m, nm in normal_maps.items():
            assert m in self.tex, "a normal map needs the mesh's UVs (include/rpt.h, \"mesh normal maps\": Composition)"
            nm = nm if isinstance(nm, dict) else {"texels": nm}
            self.maps[m] = (decode_normal_map_f64(nm["texels"], nm.get("strength", 1.0), nm.get("flip_green", False)),
                            FILTERS[nm.get("filter", "bilinear")])
        self._won = None
        self._in_any_hit = False

    # "mesh cutouts": the triangle test gains one last line, in both walks; the TEXTURE's wrap, the MASK's own size
    def _cut_of(self, k):
        m = int(self.tri_mesh[k])
        return (self.cut[m], self.tex[m][1]) if m in self.cut else None

    def _triangles(self, o, d, M):
        hit, t = super()._triangles(o, d, M)
        if self.cut and not (self._in_any_hit and self.no_cut_in_any_hit):
            cut_test(self, hit, o, d, M, self._cut_of)
        return hit, t

    def any_hit(self, o, d, max_dist, mut, M):
        self._in_any_hit = True
        try:
            return super().any_hit(o, d, max_dist, mut, M)
        finally:
            self._in_any_hit = False

    def closest_hit(self, o, d, st, ls, mut, M):
        self.won = self._won = None
        return super().closest_hit(o, d, st, ls, mut, M)

    # "smooth mesh shading", then "mesh normal maps": N is the normal the hit would have had without the map
    def shading_normal(self, k, u, v, M):
        flat = flat_normal(self, k)
        N = self.interpolated_normal(k, u, v, M) if self.smooth_tri[k] else flat
        m = int(self.tri_mesh[k])
        if m in self.maps:
            texels, filt = self.maps[m]
            wrap = CLAMP if self.map_wrap_clamp else self.tex[m][1]    # the TEXTURE's wrap, the MAP's own filter and size
            xyz = tex_lookup(texels, *interp_uv(self, k, u, v), wrap, filt, M)
            ua, ub, uc = (self.uv[j] for j in self.corner[k])
            N = bend(np.array(flat if self.bend_from_flat else N), self.e1[k], self.e2[k], ua, ub, uc, xyz, M)
        return N

    def triangle_normal(self, k, o, d, M):
        u, v = self.barycentrics(k, o, d)
        self.won, self._won = k, (k, u, v)
        return self.shading_normal(k, u, v, M)

    # "mesh textures": at a winning triangle of a textured mesh only mat.rgb changes; emission is never textured
    def patch(self, m, d, hp, mat, mut, M):
        super().patch(m, d, hp, mat, mut, M)
        won, self._won = self._won, None                             # (set by the triangle that has just won, and by nothing else)
        if won is not None:
            k, u, v = won
            mesh = int(self.tri_mesh[k])
            if mesh in self.tex and not (self.no_texture_under_env and self.env_set):
                texels, wrap, filt = self.tex[mesh]
                tex = tex_lookup(texels, *interp_uv(self, k, u, v), wrap, filt, M)
                mat.rgb = tuple(P.noisy(float(c) * float(x)) for c, x in zip(mat.rgb, tex))


class ComposedPath(P.Path):
    """pt_f64.Path for a ComposedMeshDescScene.  Planted faults: light_uses_shading_normal (the mesh-light sampler and the hit-side
    weight use the shading normal — smooth, bent — where the flat one belongs) and n_without_on_meshes_under_env (N leaves the ON
    meshes out while an environment is SAMPLED: they are never picked, and every pick is scaled by the smaller N)."""

    def __init__(self, scene, light_uses_shading_normal=False, n_without_on_meshes_under_env=False, mesh_light_pdf_scale=1.0):
        super().__init__(scene)
        self.light_uses_shading_normal, self.n_without_on_meshes_under_env = light_uses_shading_normal, n_without_on_meshes_under_env
        self.mesh_light_pdf_scale = mesh_light_pdf_scale             # (a subtle planted fault: 0.98)

    def picks(self):
        """include/rpt.h, "pickable lights": the rpt_lights, the ON meshes in ascending mesh index, the SAMPLED environment last."""
        sc = self.scene
        picks = [("light", light) for light in sc.lights]
        if not (self.n_without_on_meshes_under_env and sc.env_sampled):
            picks += [("mesh", j) for j in range(len(sc.mesh_lights))]
        if sc.env_sampled:
            picks.append(("env", None))
        return picks

    def sample_mesh_light(self, ordinal, scatter_pos, draw, M):
        shading = (lambda k, bu, bv: self.scene.shading_normal(k, bu, bv, M)) if self.light_uses_shading_normal else None
        return sample_mesh_light(self.scene, ordinal, float(len(self.picks())), scatter_pos, draw, M, normal_of=shading,
                                 pdf_scale=self.mesh_light_pdf_scale)

    def sample_env(self, draw, M):
        return sample_env(self.scene, float(len(self.picks())), draw, M)

    def hit_weight(self, bounce, d, st, ss_pdf, M):
        return hit_weight(self.scene, bounce, d, st, ss_pdf, self.mut, M, normal=st.normal if self.light_uses_shading_normal else None)

    def miss(self, bounce, d, ss_pdf, M):
        """An environment replaces rpt_background at a miss (include/rpt.h, "environment lighting")."""
        sc = self.scene
        return miss(sc, bounce, d, ss_pdf, self.mut, M) if sc.env_set else sc.background(d)

    def direct_light(self, d, st, draw, M, rays):
        return direct_light(self, d, st, draw, M, rays)

    def sample(self, col, row, width, height, draws):
        return trace(self, col, row, width, height, draws)
