"""Mesh emission maps (include/rpt.h, "mesh emission maps") in float64, over the material-mapped restatement of
tests/mesh_mmap_f64.py: EmapMeshDescScene is MmapMeshDescScene with one more step at a winning triangle — after the base's patch
(which has written the material's emission), emission.c *= E.c, E looked up through the TEXTURE's UVs and wrap with the MAP's own
filter and size by the same tex_lookup, NEAREST margins included.  The emitter exit reads the same patched material, so the one step
covers it.  EmapPath is ComposedPath whose mesh-light sampler, for an ON mesh with a map, hands out N_f * (m.emission * E(bu, bv)):
the normal_of hook of mesh_compose_f64.sample_mesh_light hands out (triangle, bu, bv), and returns the very normal the sampler
would have computed, so everything but the emission line keeps its bits.  The decode is "mesh textures"'.

`emission_maps` is the very dict Tracer.set_mesh_emission_maps takes.  Three planted faults: sampler_ignores_map (the sampler hands
out the unmapped emission), sampler_swaps_uv (the sampler looks up at (bv, bu)) and hit_ignores_map (the hit side, and with it the
emitter exit, leaves the emission unmapped).  The scene and the maps the float64 tests use are here as well, so the GPU file and the
CPU file hand both sides one value."""
import numpy as np

import mesh_mmap_f64 as MM
import pt_f64 as P
from mesh_compose_f64 import FILTERS, ComposedPath, decode_texture_f64, interp_uv, sample_mesh_light, tex_lookup

OBJECT_EMISSION = (0.35, 0.12, 0.06)


class EmapMeshDescScene(MM.MmapMeshDescScene):
    def __init__(self, desc, scene, emission_maps=None, hit_ignores_map=False, **mapped):
        super().__init__(desc, scene, **mapped)
        self.hit_ignores_map = hit_ignores_map
        self.emaps = {}
        for m, em in (emission_maps or {}).items():
            assert m in self.tex, "an emission map needs the mesh's UVs (include/rpt.h, \"mesh emission maps\": Scope)"
            em = em if isinstance(em, dict) else {"texels": em}
            self.emaps[m] = (decode_texture_f64(em["texels"], float(em.get("gamma", 1.0))), FILTERS[em.get("filter", "bilinear")])

    def emission_factor(self, k, u, v, M):
        """E at barycentrics (u, v) of flattened triangle k, or None when its mesh has no map."""
        mesh = int(self.tri_mesh[k])
        if mesh not in self.emaps:
            return None
        texels, filt = self.emaps[mesh]
        return tuple(float(x) for x in tex_lookup(texels, *interp_uv(self, k, u, v), self.tex[mesh][1], filt, M))

    def patch(self, m, d, hp, mat, mut, M):
        won = self._won                                               # (the base's patch consumes it)
        super().patch(m, d, hp, mat, mut, M)
        if won is None or self.hit_ignores_map:
            return
        E = self.emission_factor(*won, M)
        if E is not None:
            mat.emission = tuple(P.noisy(float(e) * x) for e, x in zip(mat.emission, E))


class EmapPath(ComposedPath):
    def __init__(self, scene, sampler_ignores_map=False, sampler_swaps_uv=False, **composed):
        super().__init__(scene, **composed)
        self.sampler_ignores_map, self.sampler_swaps_uv = sampler_ignores_map, sampler_swaps_uv

    def sample_mesh_light(self, ordinal, scatter_pos, draw, M):
        sc = self.scene
        n_f = float(len(self.picks()))
        _, _, _, tri, em, first = sc.mesh_lights[ordinal]
        picked = []

        def normal_of(k, bu, bv):
            picked.append((k, bu, bv))
            if self.light_uses_shading_normal:
                return sc.shading_normal(k, bu, bv, M)
            a, b, c = (tuple(float(x) for x in p) for p in tri[k - first])      # the sampler's own normal, by its own operations
            return P.normalize(P.cross(P.sub(b, a), P.sub(c, a)))

        ls, area = sample_mesh_light(sc, ordinal, n_f, scatter_pos, draw, M, normal_of=normal_of)
        if picked and not self.sampler_ignores_map:
            k, bu, bv = picked[0]
            E = sc.emission_factor(k, bv, bu, M) if self.sampler_swaps_uv else sc.emission_factor(k, bu, bv, M)
            if E is not None:
                ls.emission = P.scale(n_f, tuple(P.noisy(float(e) * x) for e, x in zip(em, E)))
        return ls, area


def scene():
    """mesh_mmap_f64's scene with an object that emits a little: the hit side's map acts on both meshes, the sampler's on the lamp."""
    from rust_pathtracer_amd import scenes
    s = MM.scene()
    s.materials[0] = scenes.full_material(rgb=(0.8, 0.3, 0.25), roughness=0.9, metallic=MM.OBJECT_METALLIC, emission=OBJECT_EMISSION)
    return s


def emission_maps(identity=False):
    """The maps of the float64 cases: mesh 0 (the object) NEAREST over a 5 x 3 noise map at gamma 2.2, mesh 1 (the lamp) BILINEAR
    over a 16 x 16 one whose left half is dimmed, so that (bu, bv) and (bv, bu) see different light.  identity: all-255 maps of the
    same sizes, filters and gammas."""
    a, b = MM.noise_map(5, 3, 87), MM.noise_map(16, 16, 88)
    b[:, :8, :3] //= 6
    if identity:
        a, b = np.full_like(a, 255), np.full_like(b, 255)
    return {0: dict(texels=a, filter="nearest", gamma=2.2), 1: dict(texels=b, filter="bilinear", gamma=1.0)}
