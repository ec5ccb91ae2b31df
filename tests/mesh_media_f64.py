"""Mesh media restated in float64 (include/rpt.h, "mesh media"): MediaMeshDescScene and MediaMeshPath, written from that section's
wording on top of the composed mesh restatement (tests/mesh_compose_f64.py: ComposedMeshDescScene, ComposedPath) and of the media
restatement (tests/media_sdf_f64.py), whose phase_hg, sample_hg, transmittance and medium_segment are CALLED here, not copied: step
2 of the bounce loop is MediaSdfPath.medium_segment itself, run over this path's direct_light.

The section's rules, each where the code applies it:

  * which medium a hit carries (MediaMeshDescScene.hit_medium): the winning triangle's mesh's, if it has one that is not NONE; a
    sphere or a plane carries none and leaves in_medium and state.medium as they are
  * step 4 (MediaMeshPath.sample): in_medium = dot(new direction, G) < 0 with G the FLAT normal of the winning triangle, whatever
    smooth shading or a normal map made of state.normal; the sign's margin is recorded
  * step 1 at a miss: ComposedPath.miss, unattenuated, reading scatter_sample.pdf — after a medium scatter the phase pdf
  * steps 2 and 3 (MediaMeshPath.direct_light): the mesh scenes' pick (ComposedPath.picks); at a scatter point scatter_pos is the
    point itself and the phase function stands for f, pdf and the MIS weight; `li` is multiplied by the transmittance over
    light_sample.dist only when that distance is finite; the pick's margins are recorded as the composed restatement records them
  * `d < seg` (medium_segment): M.rel(flight, seg), as media_sdf_f64 records it
  * shadow rays: the scene's any_hit, cutouts included; a hole is no hit, so nothing changes at one

Faults a device could have in the join are planted by keyword arguments; tests/test_mesh_media_f64.py holds each to draws that must
see it."""
import numpy as np

import media_sdf_f64 as MS
import pt_f64 as P
from mesh_compose_f64 import ComposedMeshDescScene, ComposedPath, N_DRAWS, flat_normal
from test_gpu_mesh_smooth_f64 import SmoothMeshDescScene

TYPES = {None: MS.MEDIUM_NONE, "absorb": MS.MEDIUM_ABSORB, "scatter": MS.MEDIUM_SCATTER, "emissive": MS.MEDIUM_EMISSIVE}


class MediaMeshDescScene(ComposedMeshDescScene):
    """ComposedMeshDescScene with `media` as Tracer.set_mesh_media takes them: {mesh: None or dict(type=, density=, color=,
    anisotropy=0.0)}.  The anisotropy is clamped to [-0.9, 0.9] as the setter clamps it (in float32: the context holds that value).

    Planted fault: hole_leaves_medium — a cutout hole passed on the way to the hit toggles in_medium (the scene records the holes a
    closest_hit passed; the path applies them)."""

    def __init__(self, desc, scene, media=None, hole_leaves_medium=False, **composed):
        super().__init__(desc, scene, **composed)
        self.hole_leaves_medium = hole_leaves_medium
        self.mesh_medium = {}
        for m, md in (media or {}).items():
            if md is None or TYPES[md.get("type")] == MS.MEDIUM_NONE:
                continue
            g = float(np.clip(np.float32(md.get("anisotropy", 0.0)), np.float32(-0.9), np.float32(0.9)))
            color = tuple(float(np.float32(c)) for c in md.get("color", (1.0, 1.0, 1.0)))
            self.mesh_medium[int(m)] = MS.Medium(TYPES[md["type"]], float(np.float32(md.get("density", 0.0))), color, g, g)
        self.holes_passed = []

    def hit_medium(self):
        """-> (the medium the last closest_hit's hit carries or None, its winning triangle or None)."""
        k = self.won
        if k is None:
            return None, None
        return self.mesh_medium.get(int(self.tri_mesh[k])), k

    def _triangles(self, o, d, M):
        hit, t = super()._triangles(o, d, M)
        if self.hole_leaves_medium and self.cut and not self._in_any_hit:
            solid, ts = SmoothMeshDescScene._triangles(self, o, d, P.Margin())
            self.holes_passed = [(int(k), float(ts[k])) for k in np.nonzero(solid & ~hit)[0]]
        return hit, t


class MediaMeshPath(ComposedPath):
    """ComposedPath for a MediaMeshDescScene.  Planted faults, each one line of the join: side_uses_shading_normal (step 4 reads
    state.normal — smooth, bent — where G belongs), env_sample_attenuated (a light sample of infinite distance is attenuated too),
    no_light_attenuation_inside (no light sample is), scatter_nee_offset_by_eps (the light estimate at a scatter point starts at
    p + eps * the last surface's facing normal), medium_from_sphere_hit (a sphere or plane hit inside a medium clears in_medium)."""

    def __init__(self, scene, side_uses_shading_normal=False, env_sample_attenuated=False, no_light_attenuation_inside=False,
                 scatter_nee_offset_by_eps=False, medium_from_sphere_hit=False, **composed):
        super().__init__(scene, **composed)
        self.side_uses_shading_normal, self.env_sample_attenuated = side_uses_shading_normal, env_sample_attenuated
        self.no_light_attenuation_inside, self.scatter_nee_offset_by_eps = no_light_attenuation_inside, scatter_nee_offset_by_eps
        self.medium_from_sphere_hit = medium_from_sphere_hit
        self.mut = frozenset()                                       # (what medium_segment asks for its own planted faults: none)

    medium_segment = MS.MediaSdfPath.medium_segment                  # step 2, as it is

    def direct_light(self, d, st, draw, M, rays, phase=None, inside=None):
        """mesh_compose_f64.direct_light — tracer.rs:126-170 over the pickable lights — with "mesh media"'s two additions: at a
        scatter point (phase: the medium) scatter_pos is the point and the phase function stands in place of the BSDF; inside a
        medium (inside: it) a light sample of finite distance is attenuated over that distance."""
        sc, mut = self.scene, self.mut
        ld = P.ZERO3
        if phase is not None and not self.scatter_nee_offset_by_eps:
            scatter_pos = st.fhp
        else:
            scatter_pos = P.add(st.fhp, P.scale(self.eps, st.ffnormal))
        picks = self.picks()
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
                    ls.emission = P.scale(float(n), what[2])
                area = what[6]
            elif kind == "mesh":
                ls, area = self.sample_mesh_light(what, scatter_pos, draw, M)
            else:
                ls, area = self.sample_env(draw, M)
            li = ls.emission
            fac = P.dot(ls.direction, ls.normal)
            M.of(fac, 1.0)                                            # the facing test, unchanged
            if fac < 0.0:
                max_dist = ls.dist - self.eps
                rays.append(scatter_pos + ls.direction + (max_dist,))
                if not sc.any_hit(scatter_pos, ls.direction, max_dist, mut, M):
                    if inside is not None and not self.no_light_attenuation_inside and (ls.dist <= P.F_MAX or self.env_sample_attenuated):
                        li = P.mul(li, MS.transmittance(inside, ls.dist))
                    if phase is not None:
                        pdf = MS.phase_hg(P.dot(P.neg(d), ls.direction), phase.g)
                        f = (pdf, pdf, pdf)
                    else:
                        f, pdf = P.disney_eval(st.material, st.eta, P.neg(d), st.ffnormal, ls.direction, mut, M)
                    mis = 1.0
                    if area > 0.0:
                        mis = P.power_heuristic(ls.pdf, pdf, mut)
                    if pdf > 0.0:
                        ld = P.add(ld, P.scale(mis, P.mul(li, P.div3(f, (ls.pdf, ls.pdf, ls.pdf)))))
        return ld

    def sample(self, col, row, width, height, draws):
        """mesh_compose_f64.trace with steps 2 and 4 of "participating media" as "mesh media" reads them -> (radiance, rays, margin).
        With no medium on any mesh every line below that mesh_compose_f64.trace lacks is skipped, and the operations that remain are
        its own in its order."""
        assert not self.roulette
        sc, mut = self.scene, self.mut
        M = P.Margin()
        rays = []
        it = iter(draws)
        draw = lambda: float(next(it))                                # noqa: E731
        j = height - 1 - row
        x = float(col)
        y = float(height) - float(j)
        a = draw()
        b = draw()
        ps = MS.PathState()
        ps.o, ps.d = P.gen_ray(sc.cam, (x / width, 1.0 - y / height), (a, b), float(width), float(height))
        st = P.State()
        ls = P.LightSampleRec()
        depth = sc.depth
        for bounce in range(depth):
            st.material = P.Material(1.5)
            st.is_emitter = False                                     # step 1 (a path can go on after an emitter hit: a scatter before it)
            rays.append(ps.o + ps.d + (-1.0,))
            if not sc.closest_hit(ps.o, ps.d, st, ls, mut, M):
                ps.radiance = P.add(ps.radiance, P.mul(self.miss(bounce, ps.d, ps.ss_pdf, M), ps.throughput))      # unattenuated
                break
            if sc.hole_leaves_medium:
                for k, t in sc.holes_passed:
                    md = sc.mesh_medium.get(int(sc.tri_mesh[k]))
                    if t < st.hit_dist and md is not None:
                        ps.in_medium = not ps.in_medium
                        ps.medium = md if ps.in_medium else ps.medium
            if ps.in_medium and self.medium_segment(ps, st, draw, M, rays):      # step 2
                continue
            o, d = ps.o, ps.d
            st.fhp = P.add(o, P.scale(st.hit_dist, d))
            nd = P.dot(st.normal, d)
            M.of(nd, 1.0)
            st.ffnormal = st.normal if nd <= 0.0 else P.neg(st.normal)
            st.material.finalize()
            st.eta = P.dv(1.0, st.material.ior) if nd < 0.0 else st.material.ior
            w = self.hit_weight(bounce, d, st, ps.ss_pdf, M)
            ps.radiance = P.add(ps.radiance, P.mul(P.scale(w, st.material.emission), ps.throughput))
            if st.is_emitter:
                mis = P.power_heuristic(ps.ss_pdf, ls.pdf, mut) if depth > 0 else 1.0
                ps.radiance = P.add(ps.radiance, P.mul(P.scale(mis, ls.emission), ps.throughput))
                break
            carried, won = sc.hit_medium()                            # (before direct_light: its shadow rays run other walks)
            inside = ps.medium if ps.in_medium else None
            ps.radiance = P.add(ps.radiance, P.mul(self.direct_light(d, st, draw, M, rays, inside=inside), ps.throughput))
            f, ps.ss_l, ps.ss_pdf = P.disney_sample(st.material, st.eta, P.neg(d), st.ffnormal, ps.ss_l, draw, mut, M)
            if ps.ss_pdf > 0.0:
                ps.throughput = P.mul(ps.throughput, P.div3(f, (ps.ss_pdf, ps.ss_pdf, ps.ss_pdf)))
            else:
                break
            ps.d = ps.ss_l
            ps.o = P.add(st.fhp, P.scale(self.eps, ps.d))
            if carried is not None:                                   # step 4
                G = st.normal if self.side_uses_shading_normal else flat_normal(sc, won)
                side = P.dot(ps.d, G)
                M.of(side, 1.0)
                ps.in_medium = side < 0.0
                if ps.in_medium:
                    ps.medium = carried
            elif won is None and self.medium_from_sphere_hit:
                ps.in_medium = False
        return ps.radiance, rays, M.m


__all__ = ["MediaMeshDescScene", "MediaMeshPath", "N_DRAWS"]
