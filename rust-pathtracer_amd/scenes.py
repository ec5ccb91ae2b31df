"""Project-defined benchmark scenes (BASELINE.json configs 4-5; the reference has only AnalyticalScene).

Everything is generated from the project's PCG hash so the scenes are reproducible in any
language: u(i) = (pcg(seed + i) >> 8) * 2^-24."""
from . import _abi
from .api import AnalyticalLight, Material, Pinhole, Scene

_DEFAULTS = dict(rgb=(1.5, 1.5, 1.5), emission=(0.0, 0.0, 0.0), anisotropic=0.0, metallic=0.0, roughness=0.5,
                 subsurface=0.0, specular_tint=0.0, sheen=0.0, sheen_tint=0.0, clearcoat=0.0, clearcoat_gloss=0.0,
                 spec_trans=0.0, ior=1.45)                      # Material::new, material.rs:82-114


def full_material(medium=None, **fields):
    """A patch that sets every field (mask == RPT_MAT_ALL): what large scenes require for spheres.  `medium`: also the
    Medium (large scenes with media need it on every sphere material; dict(type="none") for none)."""
    d = dict(_DEFAULTS)
    d.update(fields)
    return Material(medium=medium, **d)


def pcg_hash(v):
    state = (v * 747796405 + 2891336453) & 0xFFFFFFFF
    word = (((state >> ((state >> 28) + 4)) ^ state) * 277803737) & 0xFFFFFFFF
    return ((word >> 22) ^ word) & 0xFFFFFFFF


class _U:
    def __init__(self, seed):
        self.seed, self.i = seed & 0xFFFFFFFF, 0

    def __call__(self, lo=0.0, hi=1.0):
        u = (pcg_hash((self.seed + self.i) & 0xFFFFFFFF) >> 8) * 2.0 ** -24
        self.i += 1
        return lo + (hi - lo) * u


def media_scene():
    """Participating media (project-defined, include/rpt.h) in the reference's scene: the left sphere becomes a glass ball
    full of forward-scattering fog, the right one a ball of absorbing amber, a third small one glows (an emissive medium), and
    a small light sits inside the fog (visible from inside it: any_hit honours max_dist)."""
    from .api import AnalyticalScene
    s = AnalyticalScene()
    s.media = True
    s.any_hit_uses_max_dist = True
    s.max_depth = 12
    s.materials[0] = Material(rgb=(1.0, 1.0, 1.0), roughness=0.05, spec_trans=1.0, ior=1.2,
                              medium=dict(type="scatter", density=1.6, color=(0.95, 0.9, 0.8), anisotropy=0.6))
    s.materials[1] = Material(rgb=(1.0, 0.9, 0.7), roughness=0.1, spec_trans=1.0, ior=1.33,
                              medium=dict(type="absorb", density=1.2, color=(0.9, 0.55, 0.1)))
    s.materials.append(Material(rgb=(1.0, 1.0, 1.0), roughness=0.02, spec_trans=1.0, ior=1.05,
                                medium=dict(type="emissive", density=0.8, color=(0.2, 0.6, 1.0), anisotropy=2.0)))
    s.spheres.append(((0.0, -0.6, 1.2), 0.4, 3))
    s.lights.append(AnalyticalLight.spherical((-1.1, 0.0, 0.0), 0.12, (12.0, 12.0, 12.0)))
    return s


def random_spheres_scene(n_spheres=10000, n_lights=16, seed=0x5EED0005, n_palette=64, media=False):
    """spheres uniform in [-60,60]x[0,12]x[-120,0], radii U[0.3,1.2], a
    palette of full materials (rgb U[.05,1]^3, roughness U[.02,1], metallic 1 with p=.3, clearcoat 1
    with p=.2), a checker plane y=-1, spherical lights (r=1, emission 5) on a grid at y=15."""
    u = _U(seed)
    s = Scene()
    s.camera = Pinhole((0.0, 6.0, 14.0), (0.0, 2.0, -40.0), 70.0)
    s.background = dict(kind=_abi.RPT_BG_GRADIENT_Y, colour_a=(1.0, 1.0, 1.0), colour_b=(0.5, 0.7, 1.0), gamma=2.2, scale=0.5)
    s.any_hit_uses_max_dist = True
    s.media = media
    s.materials = []
    for _ in range(n_palette):
        rgb = (u(0.05, 1.0), u(0.05, 1.0), u(0.05, 1.0))
        rough = u(0.02, 1.0)
        metallic = 1.0 if u() < 0.3 else 0.0
        coat = 1.0 if u() < 0.2 else 0.0
        medium = None
        if media:                                     # a third of the palette: glass full of fog / coloured absorber / glow
            kind = (len(s.materials) % 6)
            medium = (dict(type="scatter", density=0.9, color=rgb, anisotropy=0.5), dict(type="absorb", density=1.5, color=rgb),
                      dict(type="emissive", density=0.3, color=rgb), dict(type="none"), dict(type="none"), dict(type="none"))[kind]
            if kind < 3:
                s.materials.append(full_material(medium=medium, rgb=(1.0, 1.0, 1.0), roughness=0.05, spec_trans=1.0, ior=1.3))
                continue
        s.materials.append(full_material(medium=medium, rgb=rgb, roughness=rough, metallic=metallic, clearcoat=coat, clearcoat_gloss=coat))
    s.materials.append(Material(roughness=1.0, checker_dir=(0.5, 100.0, 0.25, 0.1)))     # the reference's floor
    floor = len(s.materials) - 1
    s.spheres = []
    for _ in range(n_spheres):
        c = (u(-60.0, 60.0), u(0.0, 12.0), u(-120.0, 0.0))
        r = u(0.3, 1.2)
        s.spheres.append((c, r, int(u() * n_palette) % n_palette))
    # The floor reaches 400 units along a ray: beyond that the f32 ray/sphere test of the reference is
    # noise (d2 = l.l - tca^2 cancels), which would force brute-force tests for rays that start there.
    s.planes = [((0.0, 1.0, 0.0), (0.0, -1.0, 0.0), 0.0001, floor, 400.0)]
    side = max(1, int(round(n_lights ** 0.5)))
    s.lights = []
    for i in range(n_lights):
        gx, gz = i % side, i // side
        x = -45.0 + 90.0 * (gx + 0.5) / side
        z = -105.0 + 90.0 * (gz + 0.5) / side
        s.lights.append(AnalyticalLight.spherical((x, 15.0, z), 1.0, (5.0, 5.0, 5.0)))
    return s


def six_primitive_scene():
    """Five spheres with whole materials on the reference's checker floor: a small scene of more than four primitives — what
    bench.py's `six_primitives` leg renders (the material table by class of accepted set, csrc/launch.h MatClassMap) and
    tests/test_gpu_dispatch.py checks against the oracle ("five spheres on a floor")."""
    from .api import AnalyticalScene
    s = AnalyticalScene()
    s.materials = [full_material(rgb=(0.9, 0.3, 0.2), clearcoat=1.0, clearcoat_gloss=0.7, roughness=0.4),
                   full_material(rgb=(0.8, 0.8, 0.9), roughness=0.15, metallic=1.0, anisotropic=0.6),
                   full_material(rgb=(0.95, 0.95, 1.0), roughness=0.05, spec_trans=1.0, ior=1.5),
                   full_material(rgb=(0.2, 0.7, 0.3), roughness=0.6, sheen=0.8, subsurface=0.4),
                   full_material(rgb=(0.9, 0.8, 0.1), roughness=0.3, metallic=1.0),
                   Material(roughness=1.0, checker_dir=(0.5, 100.0, 0.25, 0.1))]
    s.spheres = [((0.2, 0.0, -0.6), 1.0, 0), ((-1.3, -0.3, 0.4), 0.7, 1), ((1.4, -0.4, 0.5), 0.6, 2), ((-0.4, -0.6, 1.1), 0.4, 3), ((0.6, -0.65, 1.3), 0.35, 4)]
    s.planes = [((0.0, 1.0, 0.0), (0.0, -1.0, 0.0), 0.0001, 5)]
    return s


def sdf_scene():
    """BASELINE.json configs[3] (project-defined; the reference has no SDF scene, Readme.md:18): a
    sphere-marched blob — the polynomial smooth union of two spheres and a torus — over the reference's
    checker plane, next to one analytical clearcoat sphere, lit by the reference's spherical light."""
    s = Scene()
    s.camera = Pinhole((0.0, 0.6, 3.6), (0.0, 0.0, 0.0), 70.0)
    s.background = dict(kind=_abi.RPT_BG_GRADIENT_Y, colour_a=(1.0, 1.0, 1.0), colour_b=(0.5, 0.7, 1.0), gamma=2.2, scale=0.5)
    s.lights = [AnalyticalLight.spherical((3.0, 2.0, 2.0), 1.0, (3.0, 3.0, 3.0))]
    s.materials = [
        Material(rgb=(0.2, 0.55, 0.9), roughness=0.35, clearcoat=1.0, clearcoat_gloss=0.8),      # the blob
        Material(rgb=(1.0, 0.186, 0.0), clearcoat=1.0, clearcoat_gloss=1.0, roughness=0.1),      # analytical sphere
        Material(roughness=1.0, checker_dir=(0.5, 100.0, 0.25, 0.1)),                           # floor
    ]
    s.spheres = [((1.9, -0.4, -0.3), 0.6, 1)]
    s.planes = [((0.0, 1.0, 0.0), (0.0, -1.0, 0.0), 0.0001, 2)]
    s.sdf = dict(prims=[(_abi.RPT_SDF_SPHERE, (-0.9, -0.2, 0.0), (0.8, 0.0)),
                        (_abi.RPT_SDF_SPHERE, (0.1, 0.15, 0.2), (0.55, 0.0)),
                        (_abi.RPT_SDF_TORUS_Y, (-0.3, -0.55, 0.1), (1.25, 0.22))],
                 material=0, smooth_k=0.35, max_steps=128, hit_eps=1e-3, max_t=60.0, normal_eps=1e-3)
    return s


def icosphere(subdivisions=3, center=(0.0, 0.0, 0.0), radius=1.0):
    """-> (vertices [N, 3] f32, indices [M, 3] u32): the icosahedron, each triangle cut into four `subdivisions` times, the vertices
    pushed out to the sphere (20 * 4^subdivisions triangles, shared vertices)."""
    import numpy as np
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = np.array([[-1, t, 0], [1, t, 0], [-1, -t, 0], [1, -t, 0], [0, -1, t], [0, 1, t], [0, -1, -t], [0, 1, -t],
                  [t, 0, -1], [t, 0, 1], [-t, 0, -1], [-t, 0, 1]], dtype=np.float64)
    f = np.array([[0, 11, 5], [0, 5, 1], [0, 1, 7], [0, 7, 10], [0, 10, 11], [1, 5, 9], [5, 11, 4], [11, 10, 2], [10, 7, 6],
                  [7, 1, 8], [3, 9, 4], [3, 4, 2], [3, 2, 6], [3, 6, 8], [3, 8, 9], [4, 9, 5], [2, 4, 11], [6, 2, 10], [8, 6, 7],
                  [9, 8, 1]])
    tri = v[f]
    tri /= np.linalg.norm(tri, axis=2, keepdims=True)
    for _ in range(subdivisions):
        a, b, c = tri[:, 0], tri[:, 1], tri[:, 2]
        ab, bc, ca = (a + b) * 0.5, (b + c) * 0.5, (c + a) * 0.5
        ab, bc, ca = (x / np.linalg.norm(x, axis=1, keepdims=True) for x in (ab, bc, ca))
        tri = np.stack([np.stack([a, ab, ca], 1), np.stack([ab, b, bc], 1), np.stack([ca, bc, c], 1), np.stack([ab, bc, ca], 1)], 1).reshape(-1, 3, 3)
    pts = (tri.reshape(-1, 3) * radius + np.asarray(center, dtype=np.float64)).astype(np.float32)
    verts, inv = np.unique(pts, axis=0, return_inverse=True)
    return verts, inv.reshape(-1, 3).astype(np.uint32)


def torus(major=0.7, minor=0.3, n_major=128, n_minor=64, center=(0.0, 0.0, 0.0)):
    """-> (vertices, indices): a torus around the z axis (the ring in the xy plane), n_major x n_minor quads as two triangles each."""
    import numpy as np
    u = np.arange(n_major) * (2.0 * np.pi / n_major)
    w = np.arange(n_minor) * (2.0 * np.pi / n_minor)
    uu, ww = np.meshgrid(u, w, indexing="ij")
    ring = major + minor * np.cos(ww)
    pts = np.stack([ring * np.cos(uu), ring * np.sin(uu), minor * np.sin(ww)], -1).reshape(-1, 3) + np.asarray(center)
    i, j = np.meshgrid(np.arange(n_major), np.arange(n_minor), indexing="ij")
    a = i * n_minor + j
    b = ((i + 1) % n_major) * n_minor + j
    c = ((i + 1) % n_major) * n_minor + (j + 1) % n_minor
    d = i * n_minor + (j + 1) % n_minor
    idx = np.concatenate([np.stack([a, b, c], -1).reshape(-1, 3), np.stack([a, c, d], -1).reshape(-1, 3)])
    return pts.astype(np.float32), idx.astype(np.uint32)


def mesh_scene(subdivisions=7, n_major=256, n_minor=128):
    """A triangle-mesh scene (include/rpt.h, "triangle meshes"; the reference's Todo "Implement a mesh based example scene"): the
    reference's scene with its two spheres replaced by meshes — a metal icosphere on the left, a red clearcoat torus on the right —
    over the reference's checker floor, under its light and camera.  Defaults: 327 680 + 65 536 triangles."""
    s = Scene()
    s.camera = Pinhole((0.0, 0.0, 3.0), (0.0, 0.0, 0.0), 80.0)
    s.background = dict(kind=_abi.RPT_BG_GRADIENT_Y, colour_a=(1.0, 1.0, 1.0), colour_b=(0.5, 0.7, 1.0), gamma=2.2, scale=0.5)
    s.lights = [AnalyticalLight.spherical((3.0, 2.0, 2.0), 1.0, (3.0, 3.0, 3.0))]
    s.materials = [
        full_material(rgb=(1.0, 1.0, 1.0), roughness=0.05, metallic=1.0),                        # icosphere
        full_material(rgb=(1.0, 0.186, 0.0), clearcoat=1.0, clearcoat_gloss=1.0, roughness=0.1),  # torus
        Material(roughness=1.0, checker_dir=(0.5, 100.0, 0.25, 0.1)),                            # floor (analytical.rs:107-116)
    ]
    s.planes = [((0.0, 1.0, 0.0), (0.0, -1.0, 0.0), 0.0001, 2)]
    v, t = icosphere(subdivisions, (-1.1, 0.0, 0.0), 1.0)
    s.meshes.append((v, t, 0))
    v, t = torus(0.7, 0.3, n_major, n_minor, (1.1, 0.0, 0.0))
    s.meshes.append((v, t, 1))
    return s


def mesh_light_scene(sphere_light=False, lamp_emission=(40.0, 36.0, 30.0)):
    """A small scene for mesh lights (include/rpt.h, "mesh lights"): a diffuse floor plane, a low-poly diffuse icosphere (mesh 0,
    80 triangles) and above them a small emissive quad, the "lamp" (mesh 1, two triangles, 0.3 x 0.3 around y = 1.4, tilted a
    little so that its triangles' boxes are not flat: a hit on a flat box passes include/rpt.h's point check by rounding alone) — the only light
    unless `sphere_light` adds one spherical rpt_light to the side (then two lights are pickable once the lamp is ON).  A black
    background, so every bit of radiance comes from the lamp (or the light); any_hit_uses_max_dist is set, as mesh lights need."""
    import numpy as np
    s = Scene()
    s.camera = Pinhole((0.0, 0.5, 3.2), (0.0, 0.0, 0.0), 60.0)
    s.any_hit_uses_max_dist = True                                  # (the background stays Scene()'s: constant black)
    # Twelve bounces, not the reference's four: direct_light at a path's LAST bounce sees the lamp over one more segment than any hit
    # of that path can, so with the lamp ON a frame holds one path length more than with it OFF.  Here that tail is far below what
    # the tests that compare the two can resolve (the floor reflects 0.7 and most directions leave into the black background).
    s.max_depth = 12
    s.lights = [AnalyticalLight.spherical((-2.5, 1.5, 1.0), 0.25, (6.0, 6.0, 6.0))] if sphere_light else []
    s.materials = [
        full_material(rgb=(0.8, 0.3, 0.25), roughness=0.9),                                      # the object
        full_material(rgb=(0.6, 0.6, 0.6), roughness=1.0, emission=tuple(lamp_emission)),        # the lamp
        Material(rgb=(0.7, 0.7, 0.7), roughness=1.0),                                            # floor
    ]
    s.planes = [((0.0, 1.0, 0.0), (0.0, -0.6, 0.0), 0.0001, 2)]
    v, t = icosphere(1, (0.0, 0.0, 0.0), 0.6)
    s.meshes.append((v, t, 0))
    h = 0.15
    quad = np.array([[-h, 1.37, -h], [h, 1.43, -h], [h, 1.43, h], [-h, 1.37, h]], dtype=np.float32)
    s.meshes.append((quad, np.array([[0, 1, 2], [0, 2, 3]], dtype=np.uint32), 1))
    return s


def mesh_media_scene(kind="scatter"):
    """-> (scene, media): a small scene for mesh media (include/rpt.h, "mesh media"): mesh_light_scene(sphere_light=True) (82
    triangles) with the icosphere's material made glass (spec_trans 1, ior 1.45, roughness 0.05) so that paths enter it;
    any_hit_uses_max_dist is set, as mesh lights already require.  `media` is what Tracer.set_mesh_media takes after the upload:
    a medium of `kind` ("absorb": a coloured Beer-Lambert glass, "scatter": a forward-scattering fog, "emissive": a dim glow,
    None: the icosphere loses its medium) on mesh 0."""
    s = mesh_light_scene(sphere_light=True)
    s.materials[0] = full_material(rgb=(0.95, 0.95, 0.95), roughness=0.05, spec_trans=1.0, ior=1.45)
    s.any_hit_uses_max_dist = True
    media = {
        None: None,
        "absorb": dict(type="absorb", density=3.0, color=(0.9, 0.45, 0.3)),
        "scatter": dict(type="scatter", density=2.5, color=(0.85, 0.9, 0.95), anisotropy=0.6),
        "emissive": dict(type="emissive", density=0.5, color=(0.2, 0.6, 0.9)),
    }
    if kind not in media:
        raise ValueError("kind must be \"absorb\", \"scatter\", \"emissive\" or None, not %r" % (kind,))
    return s, {0: media[kind]}


def checker_texture(w, h, colour_a=(255, 255, 255), colour_b=(40, 40, 40), cells=8):
    """-> [h, w, 4] uint8 RGBA: a checker of `cells` x `cells` fields over the whole image in two colours, alpha 255; texel (0, 0)
    has colour_a."""
    import numpy as np
    j, i = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    odd = ((i * cells // max(w, 1)) + (j * cells // max(h, 1))) % 2 == 1
    out = np.empty((h, w, 4), np.uint8)
    out[..., :3] = np.where(odd[..., None], np.asarray(colour_b, np.uint8), np.asarray(colour_a, np.uint8))
    out[..., 3] = 255
    return out


def spherical_uvs(vertices, center):
    """-> [N, 2] f32: longitude / latitude UVs of `vertices` about `center`: s = atan2(z, x) / 2 pi + 0.5, t = acos(y / r) / pi.  (A
    triangle that crosses the s = 0 / 1 meridian interpolates the long way round: a seam needs duplicated vertices.)"""
    import numpy as np
    q = np.asarray(vertices, np.float64).reshape(-1, 3) - np.asarray(center, np.float64)
    r = np.sqrt((q * q).sum(1))
    r = np.where(r > 0.0, r, 1.0)
    s = np.arctan2(q[:, 2], q[:, 0]) / (2.0 * np.pi) + 0.5
    t = np.arccos(np.clip(q[:, 1] / r, -1.0, 1.0)) / np.pi
    return np.stack([s, t], 1).astype(np.float32)


def torus_uv(major=0.7, minor=0.3, n_major=128, n_minor=64, center=(0.0, 0.0, 0.0)):
    """-> (vertices, indices, uvs): torus() with its seam rows duplicated — (n_major + 1) x (n_minor + 1) vertices, the last row and
    column repeating the first one's positions — so that s = i / n_major and t = j / n_minor are continuous across every triangle."""
    import numpy as np
    u = np.arange(n_major + 1) * (2.0 * np.pi / n_major)
    w = np.arange(n_minor + 1) * (2.0 * np.pi / n_minor)
    u[-1], w[-1] = 0.0, 0.0                                           # the seam's positions are the first row's, bit for bit
    uu, ww = np.meshgrid(u, w, indexing="ij")
    ring = major + minor * np.cos(ww)
    pts = np.stack([ring * np.cos(uu), ring * np.sin(uu), minor * np.sin(ww)], -1).reshape(-1, 3) + np.asarray(center)
    i, j = np.meshgrid(np.arange(n_major), np.arange(n_minor), indexing="ij")
    row = n_minor + 1
    a, b, c, d = i * row + j, (i + 1) * row + j, (i + 1) * row + j + 1, i * row + j + 1
    idx = np.concatenate([np.stack([a, b, c], -1).reshape(-1, 3), np.stack([a, c, d], -1).reshape(-1, 3)])
    si, tj = np.meshgrid(np.arange(n_major + 1) / n_major, np.arange(n_minor + 1) / n_minor, indexing="ij")
    return pts.astype(np.float32), idx.astype(np.uint32), np.stack([si, tj], -1).reshape(-1, 2).astype(np.float32)


def mesh_texture_scene():
    """-> (scene, uvs): a small scene for mesh textures (include/rpt.h, "mesh textures"): mesh_light_scene()'s floor and icosphere
    (mesh 0, 80 triangles, spherical_uvs) and a two-triangle quad (mesh 1, 1.2 x 1.2, standing behind and beside the icosphere,
    tilted a little) whose UVs run from -1.5 to 2.5, so that both wraps show; one spherical light and a grey constant
    background.  `uvs`: one [n_vertices, 2] f32 array per mesh."""
    import numpy as np
    s = Scene()
    s.camera = Pinhole((0.0, 0.5, 3.2), (0.0, 0.0, 0.0), 60.0)
    s.any_hit_uses_max_dist = True
    s.background = dict(kind=_abi.RPT_BG_CONSTANT, colour_a=(0.6, 0.6, 0.6), colour_b=(0.0, 0.0, 0.0), gamma=2.2, scale=1.0)
    s.lights = [AnalyticalLight.spherical((-2.5, 1.5, 1.0), 0.25, (6.0, 6.0, 6.0))]
    s.materials = [
        full_material(rgb=(0.8, 0.7, 0.6), roughness=0.9),                                       # the object
        full_material(rgb=(0.9, 0.9, 0.9), roughness=0.7),                                       # the quad
        Material(rgb=(0.7, 0.7, 0.7), roughness=1.0),                                            # floor
    ]
    s.planes = [((0.0, 1.0, 0.0), (0.0, -0.6, 0.0), 0.0001, 2)]
    v, t = icosphere(1, (0.0, 0.0, 0.0), 0.6)
    s.meshes.append((v, t, 0))
    quad = np.array([[0.5, -0.5, -0.9], [1.7, -0.5, -0.6], [1.7, 0.7, -0.55], [0.5, 0.7, -0.85]], dtype=np.float32)
    s.meshes.append((quad, np.array([[0, 1, 2], [0, 2, 3]], dtype=np.uint32), 1))
    quad_uv = np.array([[-1.5, -1.5], [2.5, -1.5], [2.5, 2.5], [-1.5, 2.5]], dtype=np.float32)
    return s, [spherical_uvs(v, (0.0, 0.0, 0.0)), quad_uv]


def mesh_emission_scene(sphere_light=False, lamp_emission=(40.0, 36.0, 30.0)):
    """-> (scene, textures, emission_maps): mesh_light_scene() with its lamp (mesh 1) textured — a 1 x 1 white texture over UVs that
    run from 0 to 1 across the quad — and emission-mapped by a small striped image (include/rpt.h, "mesh emission maps"): 8 x 4
    texels, NEAREST, four bright stripes (255, 230, 200) and four dim ones (40, 25, 10) along s.  `textures` and `emission_maps` are
    what Tracer.set_mesh_textures and Tracer.set_mesh_emission_maps take, in this order, after the upload."""
    import numpy as np
    s = mesh_light_scene(sphere_light, lamp_emission)
    uvs = np.array([[0.0, 0.0], [1.0, 0.0], [1.0, 1.0], [0.0, 1.0]], dtype=np.float32)
    stripes = np.empty((4, 8, 4), np.uint8)
    stripes[:, 0::2] = (255, 230, 200, 255)
    stripes[:, 1::2] = (40, 25, 10, 255)
    textures = {1: dict(uvs=uvs, texels=np.full((1, 1, 4), 255, np.uint8), wrap="clamp", filter="nearest")}
    return s, textures, {1: dict(texels=stripes, filter="nearest", gamma=1.0)}


def checker_mask(w, h, cells=8, opaque=255, hole=0):
    """-> [h, w] uint8, an A8 mask for Tracer.set_mesh_cutouts in checker_texture()'s pattern: `cells` x `cells` fields over the whole
    image, alternately `opaque` and `hole`; texel (0, 0) is opaque."""
    import numpy as np
    j, i = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    odd = ((i * cells // max(w, 1)) + (j * cells // max(h, 1))) % 2 == 1
    return np.where(odd, np.uint8(hole), np.uint8(opaque)).astype(np.uint8)


def mesh_cutout_scene(cells=6, size=48):
    """-> (scene, uvs, mask): a small scene for mesh cutouts (include/rpt.h, "mesh cutouts"): mesh_texture_scene()'s content and, in
    front of it, a two-triangle screen (mesh 2, 2.4 x 1.5, tilted a little, UVs over [0, 1]) for which `mask`, a size x size
    checker_mask of `cells` fields, is meant: through its holes the camera sees the icosphere and the quad behind, and the light
    reaches them.  `uvs`: one [n_vertices, 2] f32 array per mesh; give the screen any texture (1 x 1 white is enough) first."""
    import numpy as np
    s, uvs = mesh_texture_scene()
    s.materials.append(full_material(rgb=(0.25, 0.55, 0.3), roughness=0.8))                        # the screen
    screen = np.array([[-1.2, -0.55, 1.0], [1.2, -0.55, 1.1], [1.2, 0.95, 1.15], [-1.2, 0.95, 1.05]], dtype=np.float32)
    s.meshes.append((screen, np.array([[0, 1, 2], [0, 2, 3]], dtype=np.uint32), len(s.materials) - 1))
    screen_uv = np.array([[0.0, 0.0], [1.0, 0.0], [1.0, 1.0], [0.0, 1.0]], dtype=np.float32)
    return s, uvs + [screen_uv], checker_mask(size, size, cells)


def height_to_normal_map(height, scale):
    """-> [h, w, 4] uint8, an RGBA8 tangent-space normal map for Tracer.set_mesh_normal_maps from a [h, w] height field that tiles:
    the normal of texel (i, j) is normalize(-scale * dh/di, -scale * dh/dj, 1) with central differences over the wrapped
    neighbours (per texel, so `scale` is the height range in texels), stored as round(128 + 127 c) per component — the inverse of
    the library's decode — with alpha 255.  A constant field gives (128, 128, 255, 255) everywhere; +y is up (no FLIP_GREEN)."""
    import numpy as np
    h = np.asarray(height, np.float64)
    if h.ndim != 2:
        raise ValueError("height must be a 2-D array (height, width)")
    di = 0.5 * (np.roll(h, -1, 1) - np.roll(h, 1, 1))
    dj = 0.5 * (np.roll(h, -1, 0) - np.roll(h, 1, 0))
    n = np.stack([-float(scale) * di, -float(scale) * dj, np.ones_like(h)], -1)
    n /= np.sqrt((n * n).sum(-1, keepdims=True))
    out = np.full(h.shape + (4,), 255, np.uint8)
    out[..., :3] = np.clip(np.rint(128.0 + 127.0 * n), 0, 255).astype(np.uint8)
    return out


def bump_height(w, h, waves=3):
    """-> [h, w] f64 in [0, 1]: `waves` x `waves` smooth bumps that tile, the height field behind mesh_normal_map_scene()'s map."""
    import numpy as np
    j, i = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    return 0.5 + 0.5 * np.sin(2.0 * np.pi * waves * (i + 0.5) / w) * np.sin(2.0 * np.pi * waves * (j + 0.5) / h)


def mesh_normal_map_scene(size=32, tilt_degrees=15.0):
    """-> (scene, uvs, normal_map): a small scene for mesh normal maps (include/rpt.h, "mesh normal maps"): mesh_texture_scene()
    as it is, and a size x size bump map (height_to_normal_map of bump_height, three waves each way) whose steepest tilt is about
    `tilt_degrees`, meant for either mesh.  `uvs`: one [n_vertices, 2] f32 array per mesh; texture a mesh (1 x 1 white is enough)
    before giving it the map."""
    import numpy as np
    s, uvs = mesh_texture_scene()
    steepest = 0.5 * np.sin(2.0 * np.pi * 3 / size)                  # of bump_height's central differences
    return s, uvs, height_to_normal_map(bump_height(size, size, 3), np.tan(np.radians(tilt_degrees)) / steepest)


def octahedral_directions(size):
    """-> [size, size, 3] f64: the unit direction of every texel centre of a size x size octahedral image (include/rpt.h,
    "environment lighting"): texel (i, j) is row j, column i; +y is the centre, -y the four corners, +x the middle of the right
    edge, +z the middle of the last row."""
    import numpy as np
    c = (np.arange(size) + 0.5) / size * 2.0 - 1.0
    px, pz = np.meshgrid(c, c, indexing="xy")                       # [j, i]
    py = 1.0 - np.abs(px) - np.abs(pz)
    sx, sz = np.where(px >= 0.0, 1.0, -1.0), np.where(pz >= 0.0, 1.0, -1.0)
    fx, fz = (1.0 - np.abs(pz)) * sx, (1.0 - np.abs(px)) * sz
    low = py < 0.0
    p = np.stack([np.where(low, fx, px), py, np.where(low, fz, pz)], -1)
    return p / np.linalg.norm(p, axis=-1, keepdims=True)


def octahedral_from_equirect(image, size):
    """-> [size, size, 3] f32: a latitude-longitude image ([h, w, 3], row 0 at +y, column s = atan2(z, x) / 2 pi + 0.5 as
    spherical_uvs has it) resampled into the octahedral layout Tracer.set_environment takes: the nearest source texel at every texel
    centre's direction.  A convenience in plain numpy with no bit promise; rotate or filter the source first if need be."""
    import numpy as np
    src = np.asarray(image, np.float32)
    h, w = src.shape[0], src.shape[1]
    d = octahedral_directions(size)
    u = np.arctan2(d[..., 2], d[..., 0]) / (2.0 * np.pi) + 0.5
    v = np.arccos(np.clip(d[..., 1], -1.0, 1.0)) / np.pi
    col = np.clip(np.floor(u * w).astype(np.int64), 0, w - 1)
    row = np.clip(np.floor(v * h).astype(np.int64), 0, h - 1)
    return np.ascontiguousarray(src[row, col, :3])


def mesh_env_scene(size=64, sun=(0.35, 0.8, 0.5), sun_radiance=(900.0, 800.0, 650.0), sun_texels=3.0):
    """-> (scene, image): a small scene for environment lighting (include/rpt.h, "environment lighting"): mesh_light_scene()'s
    icosphere on its floor, no lamp and no rpt_light, and a size x size octahedral sky for Tracer.set_environment: dim blue above
    the horizon, dimmer grey below, and a sun `sun_texels` texels wide towards `sun` — nearly all of the image's power in a few
    texels, which is what BSDF sampling alone renders as noise."""
    import numpy as np
    s = mesh_light_scene(lamp_emission=(0.0, 0.0, 0.0))
    s.meshes = s.meshes[:1]                                         # the object; the lamp is gone (its material stays unused)
    d = octahedral_directions(size)
    img = np.where(d[..., 1:2] >= 0.0, np.array([0.10, 0.14, 0.20]), np.array([0.03, 0.03, 0.03]))
    to_sun = np.asarray(sun, np.float64) / np.linalg.norm(np.asarray(sun, np.float64))
    img = np.where((d @ to_sun)[..., None] > np.cos(2.0 * sun_texels / size), np.asarray(sun_radiance, np.float64), img)
    return s, np.ascontiguousarray(img, dtype=np.float32)


def mesh_scene_moved(scene, phase, seed=0x5EED0006):
    """-> new vertex arrays for `scene` (a mesh_scene(): the icosphere, then the torus), one per mesh, for Tracer.update_meshes: a
    radial ripple travelling over the icosphere — amplitude 0.25 * min(phase, 1) of its radius, six waves from pole to pole, a seeded
    phase offset — and the torus turned by `phase` radians about its own axis (z, through its centre).  Meshes beyond the second
    keep their positions.  phase = 0 returns the scene's arrays as they are, bit for bit; 0.05 is a small move, 0.5 a medium one,
    2.0 a large one (tools/mesh_bench.py --update)."""
    import numpy as np
    out = [np.array(v, dtype=np.float32, copy=True) for v, _, _ in scene.meshes]
    if phase == 0:
        return out
    offset = _U(seed)(0.0, 2.0 * np.pi)
    for k, v in enumerate(out[:2]):
        p = v.astype(np.float64)
        c = 0.5 * (p.min(0) + p.max(0))
        q = p - c
        if k == 0:
            r = np.sqrt((q * q).sum(1, keepdims=True))
            r = np.where(r > 0.0, r, 1.0)
            wave = np.sin(6.0 * np.pi * q[:, 1:2] / r + offset + 4.0 * phase)
            q = q * (1.0 + 0.25 * min(phase, 1.0) * wave)
        else:
            cs, sn = np.cos(phase), np.sin(phase)
            q = np.stack([cs * q[:, 0] - sn * q[:, 1], sn * q[:, 0] + cs * q[:, 1], q[:, 2]], 1)
        out[k] = (q + c).astype(np.float32)
    return out
