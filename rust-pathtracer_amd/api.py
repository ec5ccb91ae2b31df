"""Host-side mirror of the reference's API for the render path, over the C ABI.

Names and argument meaning follow the reference so code reads the same:
    reference (Rust)                                   here
    ------------------------------------------------   ---------------------------------
    ColorBuffer::new(w, h)       buffer.rs:18          ColorBuffer(w, h) / DeviceColorBuffer(w, h)
    Tracer::new(scene)           tracer.rs:13          Tracer(scene)
    Tracer::render(&mut buffer)  tracer.rs:22          Tracer.render(buffer)     (1 spp, frames += 1)
    Tracer::scene()              tracer.rs:629         Tracer.scene()
    AnalyticalScene::new()       analytical.rs:13      AnalyticalScene()
    Pinhole::new/set/set_fov     pinhole.rs:14-34      Pinhole(...)
    AnalyticalLight::spherical   light.rs:13           AnalyticalLight.spherical(...)
    buffer.convert_to_u8(frame)  buffer.rs:55          buffer.convert_to_u8()
All computation happens in the HIP library; nothing here falls back to the CPU.
"""
import ctypes as C
import math

import numpy as np

from . import _abi
from ._lib import RptError, check, lib


class Pinhole:
    """camera/pinhole.rs:6-34"""

    def __init__(self, origin=(0.0, 0.0, 3.0), center=(0.0, 0.0, 0.0), fov=80.0):
        self.origin = tuple(origin)
        self.center = tuple(center)
        self.fov = float(fov)

    def set(self, origin, center):
        self.origin = tuple(origin)
        self.center = tuple(center)

    def set_fov(self, fov):
        self.fov = float(fov)


class AnalyticalLight:
    """light.rs:6-28 (globals.rs:76-84 for the fields)"""

    def __init__(self, light_type, position, emission, radius, area, u=(0.0, 0.0, 0.0), v=(0.0, 0.0, 0.0)):
        self.light_type = light_type
        self.position = tuple(position)
        self.emission = tuple(emission)
        self.radius = float(radius)
        self.area = float(area)
        self.u = tuple(u)
        self.v = tuple(v)

    @staticmethod
    def spherical(position, radius, emission):
        r = np.float32(radius)
        area = np.float32(4.0) * np.float32(math.pi) * r * r          # light.rs:22, f32 left to right
        return AnalyticalLight(_abi.RPT_LIGHT_SPHERICAL, position, emission, radius, float(area))

    @staticmethod
    def rectangular(position, u, v, emission):
        """LightType::Rectangular (globals.rs:70): the parallelogram position + a*u + b*v.  The reference declares the type
        and has no constructor or sampling code for it; sampled only in scenes with sample_all_light_types (include/rpt.h)."""
        c = np.cross(np.asarray(u, dtype=np.float64), np.asarray(v, dtype=np.float64))
        return AnalyticalLight(_abi.RPT_LIGHT_RECTANGULAR, position, emission, 0.0, float(np.float32(np.sqrt((c * c).sum()))), u, v)

    @staticmethod
    def distant(position, emission):
        """LightType::Distant (globals.rs:72): light from the direction normalize(position); area 0 = no MIS (tracer.rs:158)."""
        return AnalyticalLight(_abi.RPT_LIGHT_DISTANT, position, emission, 0.0, 0.0)


class Material:
    """A material PATCH: only the fields passed are written over Material::new()
    (material.rs:82-114), the way analytical.rs:56-58 assigns individual fields."""

    _FIELDS = {
        "rgb": _abi.RPT_MAT_RGB, "emission": _abi.RPT_MAT_EMISSION, "anisotropic": _abi.RPT_MAT_ANISOTROPIC,
        "metallic": _abi.RPT_MAT_METALLIC, "roughness": _abi.RPT_MAT_ROUGHNESS, "subsurface": _abi.RPT_MAT_SUBSURFACE,
        "specular_tint": _abi.RPT_MAT_SPECULAR_TINT, "sheen": _abi.RPT_MAT_SHEEN, "sheen_tint": _abi.RPT_MAT_SHEEN_TINT,
        "clearcoat": _abi.RPT_MAT_CLEARCOAT, "clearcoat_gloss": _abi.RPT_MAT_CLEARCOAT_GLOSS,
        "spec_trans": _abi.RPT_MAT_SPEC_TRANS, "ior": _abi.RPT_MAT_IOR,
    }

    MEDIUM_TYPES = {"none": _abi.RPT_MEDIUM_NONE, "absorb": _abi.RPT_MEDIUM_ABSORB, "scatter": _abi.RPT_MEDIUM_SCATTER,
                    "emissive": _abi.RPT_MEDIUM_EMISSIVE}

    def __init__(self, checker_dir=None, medium=None, **fields):
        for k in fields:
            if k not in self._FIELDS:
                raise TypeError("unknown material field %r" % k)
        self.fields = fields
        self.checker_dir = checker_dir       # (scale, offset, colour_a, colour_b) or None
        # Material.medium (material.rs:16-21): dict(type="absorb"|"scatter"|"emissive"|"none", density, color, anisotropy);
        # read only by scenes with `media = True` (project-defined, include/rpt.h)
        self.medium = medium

    def to_c(self):
        m = _abi.rpt_material()
        for k, v in self.fields.items():
            m.mask |= self._FIELDS[k]
            if k in ("rgb", "emission"):
                setattr(m, k, _abi.F3(*v))
            else:
                setattr(m, k, float(v))
        if self.checker_dir is not None:
            m.proc_kind = _abi.RPT_PROC_CHECKER_DIR
            m.proc_params = _abi.F4(*self.checker_dir)
        if self.medium is not None:
            m.mask |= _abi.RPT_MAT_MEDIUM
            t = self.medium.get("type", "none")
            m.medium_type = self.MEDIUM_TYPES[t] if isinstance(t, str) else int(t)
            m.medium_density = float(self.medium.get("density", 0.0))
            m.medium_color = _abi.F3(*self.medium.get("color", (0.0, 0.0, 0.0)))
            m.medium_anisotropy = float(self.medium.get("anisotropy", 0.0))
        return m


class Scene:
    """Data-driven counterpart of trait Scene (scene.rs:5-90): instead of callbacks the
    scene describes itself (spheres, planes, lights, material patches, camera)."""

    def __init__(self):
        self.camera = Pinhole()
        self.spheres = []        # (center, radius, material_index)
        self.planes = []         # (normal, point, min_denom, material_index[, max_t])
        self.lights = []         # AnalyticalLight
        self.materials = []      # Material
        self.background = dict(kind=_abi.RPT_BG_CONSTANT, colour_a=(0.0, 0.0, 0.0), colour_b=(0.0, 0.0, 0.0), gamma=2.2, scale=1.0)
        self.eps = 0.005         # tracer.rs:16
        self.max_depth = 4       # scene.rs:28-30
        self.any_hit_uses_max_dist = False
        self.sample_all_light_types = False   # rectangular / distant lights do something (project-defined; off = the reference)
        self.media = False       # Material.medium is read: participating media (project-defined, include/rpt.h; off = the reference)
        self.sdf = None          # dict(prims=[(kind, center, (p0, p1))], material, smooth_k, max_steps, hit_eps, max_t, normal_eps)
        self.meshes = []         # (vertices [N, 3] f32, indices [M, 3] u32, material_index): triangles after the planes (include/rpt.h)
        self._keep = None

    def recursion_depth(self):
        return self.max_depth

    def number_of_lights(self):
        return len(self.lights)

    def light_at(self, index):
        return self.lights[index]

    def describe(self):
        """-> rpt_scene_desc (keeps the backing arrays alive on self)."""
        d = _abi.rpt_scene_desc()
        d.abi_version = _abi.RPT_ABI_VERSION
        d.flags = (_abi.RPT_SCENE_ANYHIT_USES_MAX_DIST if self.any_hit_uses_max_dist else 0) | \
                  (_abi.RPT_SCENE_SAMPLE_ALL_LIGHT_TYPES if self.sample_all_light_types else 0) | \
                  (_abi.RPT_SCENE_MEDIA if self.media else 0)
        d.camera.origin = _abi.F3(*self.camera.origin)
        d.camera.center = _abi.F3(*self.camera.center)
        d.camera.fov_deg = self.camera.fov
        bg = self.background
        d.background.kind = bg["kind"]
        d.background.colour_a = _abi.F3(*bg["colour_a"])
        d.background.colour_b = _abi.F3(*bg["colour_b"])
        d.background.gamma = bg["gamma"]
        d.background.scale = bg["scale"]
        d.eps = self.eps
        d.max_depth = self.max_depth
        sph = (_abi.rpt_sphere * max(1, len(self.spheres)))()
        for i, (c, r, m) in enumerate(self.spheres):
            sph[i].center = _abi.F3(*c); sph[i].radius = r; sph[i].material = m
        pl = (_abi.rpt_plane * max(1, len(self.planes)))()
        for i, pln in enumerate(self.planes):
            n, p, md, m = pln[:4]
            pl[i].normal = _abi.F3(*n); pl[i].point = _abi.F3(*p); pl[i].min_denom = md; pl[i].material = m
            pl[i].max_t = pln[4] if len(pln) > 4 else 0.0
        li = (_abi.rpt_light * max(1, len(self.lights)))()
        for i, L in enumerate(self.lights):
            li[i].type = L.light_type; li[i].position = _abi.F3(*L.position); li[i].emission = _abi.F3(*L.emission)
            li[i].radius = L.radius; li[i].area = L.area; li[i].u = _abi.F3(*L.u); li[i].v = _abi.F3(*L.v)
        ma = (_abi.rpt_material * max(1, len(self.materials)))()
        for i, M in enumerate(self.materials):
            ma[i] = M.to_c()
        d.n_spheres = len(self.spheres); d.spheres = C.cast(sph, C.POINTER(_abi.rpt_sphere))
        d.n_planes = len(self.planes); d.planes = C.cast(pl, C.POINTER(_abi.rpt_plane))
        d.n_lights = len(self.lights); d.lights = C.cast(li, C.POINTER(_abi.rpt_light))
        d.n_materials = len(self.materials); d.materials = C.cast(ma, C.POINTER(_abi.rpt_material))
        sd = None
        if self.sdf:
            sd = (_abi.rpt_sdf_prim * len(self.sdf["prims"]))()
            for i, (kind, c, prm) in enumerate(self.sdf["prims"]):
                sd[i].kind = kind; sd[i].center = _abi.F3(*c); sd[i].params = (C.c_float * 2)(*prm)
            d.sdf.n_prims = len(self.sdf["prims"]); d.sdf.prims = C.cast(sd, C.POINTER(_abi.rpt_sdf_prim))
            d.sdf.material = self.sdf["material"]; d.sdf.smooth_k = self.sdf.get("smooth_k", 0.5)
            d.sdf.max_steps = self.sdf.get("max_steps", 128); d.sdf.hit_eps = self.sdf.get("hit_eps", 1e-3)
            d.sdf.max_t = self.sdf.get("max_t", 100.0); d.sdf.normal_eps = self.sdf.get("normal_eps", 1e-3)
        me, arrays = None, []
        if self.meshes:
            import numpy as np
            me = (_abi.rpt_mesh * len(self.meshes))()
            for i, (verts, idx, m) in enumerate(self.meshes):
                v = np.ascontiguousarray(verts, dtype=np.float32).reshape(-1, 3)
                t = np.ascontiguousarray(idx, dtype=np.uint32).reshape(-1, 3)
                arrays += [v, t]
                me[i].n_vertices = v.shape[0]; me[i].vertices = v.ctypes.data_as(C.POINTER(C.c_float))
                me[i].n_triangles = t.shape[0]; me[i].indices = t.ctypes.data_as(C.POINTER(C.c_uint32))
                me[i].material = m
            d.n_meshes = len(self.meshes); d.meshes = C.cast(me, C.POINTER(_abi.rpt_mesh))
        self._keep = (sph, pl, li, ma, sd, me, arrays)
        return d


class AnalyticalScene(Scene):
    """renderer/src/analytical.rs:4-205 as data."""

    def __init__(self):
        super().__init__()
        em = 3.0
        self.lights = [AnalyticalLight.spherical((3.0, 2.0, 2.0), 1.0, (em, em, em))]            # analytical.rs:15-16
        self.materials = [
            Material(rgb=(1.0, 1.0, 1.0), roughness=0.05, metallic=1.0),                           # analytical.rs:56-58
            Material(rgb=(1.0, 0.186, 0.0), clearcoat=1.0, clearcoat_gloss=1.0, roughness=0.1),    # analytical.rs:82-85
            Material(roughness=1.0, checker_dir=(0.5, 100.0, 0.25, 0.1)),                          # analytical.rs:107-116
        ]
        self.spheres = [((-1.1, 0.0, 0.0), 1.0, 0), ((1.1, 0.0, 0.0), 1.0, 1)]                     # analytical.rs:41,70
        self.planes = [((0.0, 1.0, 0.0), (0.0, -1.0, 0.0), 0.0001, 2)]                             # analytical.rs:194-198
        self.background = dict(kind=_abi.RPT_BG_GRADIENT_Y, colour_a=(1.0, 1.0, 1.0), colour_b=(0.5, 0.7, 1.0), gamma=2.2, scale=0.5)


class ColorBuffer:
    """buffer.rs:6-32: host RGBA f32 buffer, row 0 = top, plus the frame counter."""

    def __init__(self, width, height):
        self.width = int(width)
        self.height = int(height)
        self.pixels = np.zeros(self.width * self.height * 4, dtype=np.float32)
        self.frames = 0

    def at(self, x, y):                                            # buffer.rs:29-32
        i = y * self.width * 4 + x * 4
        return [float(v) for v in self.pixels[i:i + 4]]

    def image(self):
        return self.pixels.reshape(self.height, self.width, 4)

    def convert_to_u8(self, frame=None):                           # buffer.rs:55-64, on the device
        import torch
        dev = torch.from_numpy(self.pixels).to("cuda")
        out = _convert_to_u8_tensor(dev, self.width, self.height)
        res = out.cpu().numpy().reshape(-1)
        if frame is not None:
            frame[:] = res
        return res

    def to_u8_vec(self):                                           # buffer.rs:37-52 (same arithmetic)
        return self.convert_to_u8()

    def denoise(self, iterations=3, edge_k=2.0, device=0):
        """A denoised copy (project-defined, include/rpt.h "denoiser"; the reference lists one as a Todo): a new ColorBuffer."""
        out = ColorBuffer(self.width, self.height)
        ctx = _ctx_for(device)
        check(lib().rpt_denoise(ctx, self.pixels.ctypes.data, out.pixels.ctypes.data, self.width, self.height, iterations, edge_k), ctx)
        out.frames = self.frames
        return out

    def denoise_guided(self, guides, iterations=4, edge_k=0.25, normal_k=4.0, plane_k=1000.0, device=0):
        """A copy denoised against first-hit guides (include/rpt.h "guided denoiser"): a new ColorBuffer.  `guides`: a float32 numpy
        array [height * width, 16], one rpt_guide per pixel (pack_guides, or Tracer.denoise_guides(...).cpu().numpy())."""
        guides = _host_guides(guides, self.width * self.height)
        out = ColorBuffer(self.width, self.height)
        ctx = _ctx_for(device)
        check(lib().rpt_denoise_guided(ctx, self.pixels.ctypes.data, guides.ctypes.data, out.pixels.ctypes.data, self.width, self.height, iterations,
                                       edge_k, normal_k, plane_k, 0), ctx)
        out.frames = self.frames
        return out


def _host_guides(guides, n):
    if not (isinstance(guides, np.ndarray) and guides.dtype == np.float32 and guides.shape == (n, 16)):
        raise ValueError("guides must be a float32 numpy array [%d, 16]: one rpt_guide per pixel" % n)
    return np.ascontiguousarray(guides)


def pack_guides(rays, hits, surfaces, device=0):
    """One rpt_guide per (ray, hit, surface) record (rpt_denoise_guides*): float32 [n, 16].  Three float32 arrays [n, 8], [n, 8] and
    [n, 16] as the ray queries return them: CUDA tensors go through the device form on torch's current stream and return a tensor,
    numpy arrays go through the host form and return numpy."""
    n = int(rays.shape[0])
    if tuple(rays.shape) != (n, 8) or tuple(hits.shape) != (n, 8) or tuple(surfaces.shape) != (n, 16):
        raise ValueError("rays, hits and surfaces must be [n, 8], [n, 8] and [n, 16]")
    if all(isinstance(a, np.ndarray) for a in (rays, hits, surfaces)):
        if any(a.dtype != np.float32 for a in (rays, hits, surfaces)):
            raise ValueError("rays, hits and surfaces must be float32")
        rays, hits, surfaces = (np.ascontiguousarray(a) for a in (rays, hits, surfaces))
        out = np.empty((n, 16), dtype=np.float32)
        ctx = _ctx_for(device)
        check(lib().rpt_denoise_guides(ctx, rays.ctypes.data, hits.ctypes.data, surfaces.ctypes.data, n, out.ctypes.data), ctx)
        return out
    import torch
    if not all(isinstance(a, torch.Tensor) and a.is_cuda and a.dtype == torch.float32 and a.device == rays.device for a in (rays, hits, surfaces)):
        raise ValueError("rays, hits and surfaces must all be float32 numpy arrays, or all float32 CUDA tensors on one device")
    rays, hits, surfaces = rays.contiguous(), hits.contiguous(), surfaces.contiguous()
    out = torch.empty((n, 16), dtype=torch.float32, device=rays.device)
    ctx = _ctx_for(rays.device.index or 0)
    stream = torch.cuda.current_stream(rays.device).cuda_stream
    check(lib().rpt_denoise_guides_device(ctx, rays.data_ptr(), hits.data_ptr(), surfaces.data_ptr(), n, out.data_ptr(), C.c_void_p(stream)), ctx)
    return out


class DeviceColorBuffer:
    """ColorBuffer whose pixels live in HBM (a torch CUDA tensor): what the render loop
    uses when frames are accumulated on the device and fetched once at the end."""

    def __init__(self, width, height, device="cuda:0"):
        import torch
        self.width = int(width)
        self.height = int(height)
        self.pixels = torch.zeros(self.height, self.width, 4, dtype=torch.float32, device=device)
        self.frames = 0

    def to_host(self):
        b = ColorBuffer(self.width, self.height)
        b.pixels = self.pixels.detach().cpu().numpy().reshape(-1).copy()
        b.frames = self.frames
        return b

    def convert_to_u8(self):
        return _convert_to_u8_tensor(self.pixels, self.width, self.height)

    def denoise(self, iterations=3, edge_k=2.0, out=None):
        """A denoised copy on the device (include/rpt.h "denoiser"): a new DeviceColorBuffer, or `out` (same size)."""
        import torch
        if out is None:
            out = DeviceColorBuffer(self.width, self.height, device=self.pixels.device)
        assert out.width == self.width and out.height == self.height
        ctx = _ctx_for(self.pixels.device.index or 0)
        stream = torch.cuda.current_stream(self.pixels.device).cuda_stream
        check(lib().rpt_denoise_device(ctx, self.pixels.data_ptr(), out.pixels.data_ptr(), self.width, self.height, iterations, edge_k,
                                       C.c_void_p(stream)), ctx)
        out.frames = self.frames
        return out

    def denoise_guided(self, guides, iterations=4, edge_k=0.25, normal_k=4.0, plane_k=1000.0, out=None):
        """A copy denoised against first-hit guides, on the device (include/rpt.h "guided denoiser"): a new DeviceColorBuffer, or
        `out` (same size).  `guides`: a float32 CUDA tensor [height * width, 16] on the buffer's device, one rpt_guide per pixel
        (Tracer.denoise_guides, pack_guides, or the caller's own)."""
        import torch
        n = self.width * self.height
        if not (isinstance(guides, torch.Tensor) and guides.is_cuda and guides.device == self.pixels.device and guides.dtype == torch.float32 and
                tuple(guides.shape) == (n, 16) and guides.is_contiguous()):
            raise ValueError("guides must be a contiguous float32 CUDA tensor [%d, 16] on the buffer's device" % n)
        if out is None:
            out = DeviceColorBuffer(self.width, self.height, device=self.pixels.device)
        assert out.width == self.width and out.height == self.height
        ctx = _ctx_for(self.pixels.device.index or 0)
        stream = torch.cuda.current_stream(self.pixels.device).cuda_stream
        check(lib().rpt_denoise_guided_device(ctx, self.pixels.data_ptr(), guides.data_ptr(), out.pixels.data_ptr(), self.width, self.height, iterations,
                                              edge_k, normal_k, plane_k, 0, C.c_void_p(stream)), ctx)
        out.frames = self.frames
        return out

    def convert_to_u8_at(self, frame, at):
        """buffer.rs:67-89: blit into `frame` (a CUDA uint8 tensor [at[3], at[2], 4]) at offset (at[0], at[1])."""
        import torch
        assert frame.is_cuda and frame.dtype == torch.uint8 and frame.is_contiguous() and frame.numel() == at[2] * at[3] * 4
        ctx = _ctx_for(self.pixels.device.index or 0)
        stream = torch.cuda.current_stream(self.pixels.device).cuda_stream
        check(lib().rpt_convert_to_u8_at_device(ctx, self.pixels.data_ptr(), self.width, self.height, frame.data_ptr(),
                                                at[0], at[1], at[2], at[3], C.c_void_p(stream)), ctx)
        return frame


_default_ctx = {}


def _ctx_for(device_index):
    """A bare context (no scene) for stateless helpers such as convert_to_u8."""
    if device_index not in _default_ctx:
        h = C.c_void_p()
        check(lib().rpt_create(C.byref(h), device_index))
        _default_ctx[device_index] = h
    return _default_ctx[device_index]


def _convert_to_u8_tensor(pixels, width, height):
    import torch
    assert pixels.is_cuda and pixels.dtype == torch.float32 and pixels.is_contiguous()
    idx = pixels.device.index or 0
    out = torch.empty(height, width, 4, dtype=torch.uint8, device=pixels.device)
    ctx = _ctx_for(idx)
    stream = torch.cuda.current_stream(pixels.device).cuda_stream
    check(lib().rpt_convert_to_u8_device(ctx, pixels.data_ptr(), out.data_ptr(), width, height, C.c_void_p(stream)), ctx)
    return out


def _c_camera(camera):
    """An rpt_camera from a Pinhole (or an rpt_camera, returned as it is)."""
    if isinstance(camera, _abi.rpt_camera):
        return camera
    c = _abi.rpt_camera()
    c.origin = _abi.F3(*camera.origin)
    c.center = _abi.F3(*camera.center)
    c.fov_deg = camera.fov
    return c


# The defaults of temporal accumulation ("temporal accumulation", has what was tried)
TEMPORAL_N_MAX, TEMPORAL_NORMAL_MIN, TEMPORAL_PLANE_K = 32.0, 0.9, 1000.0


class TemporalAccumulator:
    """Temporal accumulation on the device (include/rpt.h, "temporal accumulation"): carries a frame's samples into the next one while
    the camera moves.  Owns the two history tensors it swaps, the previous frame's guides and the previous camera.

        acc = TemporalAccumulator(w, h)
        for each redraw:
            buf = DeviceColorBuffer(w, h); tracer.render(buf)          # 1 spp of this camera alone
            shown = acc.accumulate(buf, tracer.denoise_guides(w, h), camera)
    """

    def __init__(self, width, height, device="cuda:0", n_max=TEMPORAL_N_MAX, normal_min=TEMPORAL_NORMAL_MIN, plane_k=TEMPORAL_PLANE_K):
        import torch
        self.width, self.height = int(width), int(height)
        self.device = torch.device(device)
        self.n_max, self.normal_min, self.plane_k = float(n_max), float(normal_min), float(plane_k)
        n = self.width * self.height
        self._history = [torch.zeros((n, 8), dtype=torch.float32, device=self.device) for _ in range(2)]
        self._cur = 0                                              # the history tensor the last call wrote
        self._prev_guides = None
        self._prev_camera = None

    def reset(self):
        """Start over: the next accumulate() is a first frame."""
        self._prev_guides = None
        self._prev_camera = None

    def accumulate(self, buffer, guides, camera, prev_positions=None, out=None):
        """Blend `buffer` (a DeviceColorBuffer holding this frame alone) into the reprojected history, on torch's current stream: a new
        DeviceColorBuffer, or `out` (same size).  `guides`: this frame's rpt_guide records, a contiguous float32 CUDA tensor
        [height * width, 16] (Tracer.denoise_guides); the accumulator keeps the tensor until the next call, so the caller must not
        write into it.  `camera`: the Pinhole the frame was rendered with.  `prev_positions`: [height * width, 4] float32 on the
        device, where each pixel's surface point was in the previous frame, for geometry that moved; None: static geometry."""
        import torch
        n = self.width * self.height
        if not (buffer.width == self.width and buffer.height == self.height and buffer.pixels.device == self.device and buffer.pixels.is_contiguous()):
            raise ValueError("buffer must be a %d x %d DeviceColorBuffer on %s" % (self.width, self.height, self.device))
        if not (isinstance(guides, torch.Tensor) and guides.device == self.device and guides.dtype == torch.float32 and tuple(guides.shape) == (n, 16) and
                guides.is_contiguous()):
            raise ValueError("guides must be a contiguous float32 CUDA tensor [%d, 16] on the accumulator's device" % n)
        if prev_positions is not None and not (isinstance(prev_positions, torch.Tensor) and prev_positions.device == self.device and
                                               prev_positions.dtype == torch.float32 and tuple(prev_positions.shape) == (n, 4) and
                                               prev_positions.is_contiguous()):
            raise ValueError("prev_positions must be a contiguous float32 CUDA tensor [%d, 4] on the accumulator's device" % n)
        if out is None:
            out = DeviceColorBuffer(self.width, self.height, device=self.device)
        assert out.width == self.width and out.height == self.height
        cam = _c_camera(camera)
        first = self._prev_guides is None
        prev_hist, hist = self._history[self._cur], self._history[1 - self._cur]
        ctx = _ctx_for(self.device.index or 0)
        stream = torch.cuda.current_stream(self.device).cuda_stream
        check(lib().rpt_temporal_accumulate_device(
            ctx, buffer.pixels.data_ptr(), guides.data_ptr(), C.addressof(cam), None if first else self._prev_guides.data_ptr(),
            None if first else prev_hist.data_ptr(), None if first else C.addressof(self._prev_camera),
            None if prev_positions is None else prev_positions.data_ptr(), out.pixels.data_ptr(), hist.data_ptr(), self.width, self.height,
            self.n_max, self.normal_min, self.plane_k, 0, C.c_void_p(stream)), ctx)
        self._cur = 1 - self._cur
        self._prev_guides, self._prev_camera = guides, cam
        out.frames = buffer.frames
        return out

    def history(self):
        """The rpt_history records the last accumulate() wrote: float32 [height * width, 8] (rgb, n, m1, m2, 0, 0)."""
        return self._history[self._cur]

    def samples(self):
        """The number of samples behind each pixel after the last accumulate(): float32 [height, width]."""
        return self.history()[:, 3].reshape(self.height, self.width)

    def variance(self):
        """max(m2 - m1^2, 0): the luminance variance of the samples behind each pixel, float32 [height, width]."""
        h = self.history()
        return (h[:, 5] - h[:, 4] * h[:, 4]).clamp_min(0.0).reshape(self.height, self.width)


def temporal_accumulate(pixels, guides, camera, prev_guides=None, prev_history=None, prev_camera=None, prev_positions=None,
                        n_max=TEMPORAL_N_MAX, normal_min=TEMPORAL_NORMAL_MIN, plane_k=TEMPORAL_PLANE_K, device=0):
    """rpt_temporal_accumulate on numpy arrays (the host form; blocks): `pixels` float32 [height, width, 4], `guides` [height * width,
    16], the previous frame's `prev_guides`, `prev_history` [height * width, 8] and `prev_camera` all None (the first frame) or all
    given.  Returns (out [height, width, 4], history [height * width, 8])."""
    if not (isinstance(pixels, np.ndarray) and pixels.dtype == np.float32 and pixels.ndim == 3 and pixels.shape[2] == 4):
        raise ValueError("pixels must be a float32 numpy array [height, width, 4]")
    h, w = pixels.shape[:2]
    n = w * h
    pixels = np.ascontiguousarray(pixels)
    guides = _host_guides(guides, n)
    if sum(x is None for x in (prev_guides, prev_history, prev_camera)) not in (0, 3):
        raise ValueError("prev_guides, prev_history and prev_camera must be all None or all given")
    ptr = lambda a: None if a is None else a.ctypes.data           # noqa: E731
    if prev_guides is not None:
        prev_guides = _host_guides(prev_guides, n)
        if not (isinstance(prev_history, np.ndarray) and prev_history.dtype == np.float32 and prev_history.shape == (n, 8)):
            raise ValueError("prev_history must be a float32 numpy array [%d, 8]" % n)
        prev_history = np.ascontiguousarray(prev_history)
    if prev_positions is not None:
        if not (isinstance(prev_positions, np.ndarray) and prev_positions.dtype == np.float32 and prev_positions.shape == (n, 4)):
            raise ValueError("prev_positions must be a float32 numpy array [%d, 4]" % n)
        prev_positions = np.ascontiguousarray(prev_positions)
    cam = _c_camera(camera)
    pcam = None if prev_camera is None else _c_camera(prev_camera)
    out = np.empty((h, w, 4), np.float32)
    history = np.empty((n, 8), np.float32)
    ctx = _ctx_for(device)
    check(lib().rpt_temporal_accumulate(ctx, pixels.ctypes.data, guides.ctypes.data, C.addressof(cam), ptr(prev_guides), ptr(prev_history),
                                        None if pcam is None else C.addressof(pcam), ptr(prev_positions), out.ctypes.data, history.ctypes.data, w, h,
                                        n_max, normal_min, plane_k, 0), ctx)
    return out, history


def comm_unique_id():
    """128 opaque bytes from rank 0 that every rank passes to Tracer(..., rank=, world=, unique_id=) (ncclGetUniqueId)."""
    uid = _abi.rpt_unique_id()
    check(lib().rpt_comm_unique_id(C.byref(uid)))
    return C.string_at(C.byref(uid), _abi.RPT_UNIQUE_ID_BYTES)


class Tracer:
    """tracer.rs:5-19.  Owns the scene; render() is the boundary into the HIP library.

    Tracer(scene, device=0)                       one GPU
    Tracer(scene, devices=[0, 1, ...])            the GPUs of a node driven by this process: render() fans out over them
                                                  inside the call, where the reference fans out over rayon threads
    Tracer(scene, device=d, rank=r, world=n,      one process per GPU (torch.distributed.run): collective construction;
           unique_id=comm_unique_id() of rank 0)  the resident_* calls are then collective too"""

    def __init__(self, scene, device=0, seed=1, devices=None, rank=None, world=None, unique_id=None):
        self._scene = scene
        self.seed = int(seed)
        self.flags = 0                 # RPT_RENDER_* bits (0 = the strict, bit-exact regenerating kernel)
        self._frame = None             # resident_to_u8's page-locked frame
        self._stale_meshes = set()     # meshes whose scene().meshes arrays a device-source call has left behind (update_meshes_device)
        self._h = C.c_void_p()
        if devices is not None:
            ids = (C.c_int * len(devices))(*devices)
            self.device = int(devices[0])
            check(lib().rpt_create_multi(C.byref(self._h), ids, len(devices)))
        elif world is not None:
            uid = _abi.rpt_unique_id()
            C.memmove(C.byref(uid), unique_id, _abi.RPT_UNIQUE_ID_BYTES)
            self.device = int(device)
            check(lib().rpt_create_rank(C.byref(self._h), self.device, int(rank), int(world), C.byref(uid)))
        else:
            self.device = int(device)
            check(lib().rpt_create(C.byref(self._h), self.device))
        self.upload_scene()

    def world(self):
        """(rank of this context's first device, ranks in all, devices this context drives)"""
        r, w, n = C.c_int(), C.c_int(), C.c_int()
        check(lib().rpt_world(self._h, C.byref(r), C.byref(w), C.byref(n)), self._h)
        return r.value, w.value, n.value

    def set_tile_rows(self, tile_rows):
        check(lib().rpt_set_tile_rows(self._h, int(tile_rows)), self._h)

    def set_dispatch(self, cost_order=1, unit_rounds=12, unit_min_spp=64, unit_slots=0):
        """Scheduling of the launches (include/rpt.h, rpt_set_dispatch): changes when a sample is computed, never its value."""
        check(lib().rpt_set_dispatch(self._h, int(cost_order), int(unit_rounds), int(unit_min_spp), int(unit_slots)), self._h)

    def upload_scene(self):
        """Call after mutating the scene returned by scene()."""
        self._refresh_stale_meshes()
        desc = self._scene.describe()
        check(lib().rpt_upload_scene(self._h, C.byref(desc)), self._h)

    def update_meshes(self, updates):
        """New vertex positions for meshes of the uploaded scene without the upload (include/rpt.h, "moving meshes"): `updates` maps
        a mesh's index in scene().meshes to an array of shape (n_vertices, 3).  The frames are those of upload_scene() of the moved
        scene, bit for bit; the hierarchy is refitted on the device, not rebuilt.  On success the scene's vertex arrays are
        replaced too, so a later upload_scene() uploads the moved scene."""
        self._move_meshes(lib().rpt_update_meshes, updates)

    def rebuild_meshes(self, updates=None):
        """update_meshes, then a new hierarchy over all triangles, built on the device (include/rpt.h, "rebuilding a moved mesh's
        hierarchy"): for meshes whose shape has changed.  The frames are again those of upload_scene() of the moved scene, bit
        for bit.  Without `updates`: a rebuild over the positions the context holds."""
        self._move_meshes(lib().rpt_rebuild_meshes, updates or {})

    def _move_meshes(self, call, updates):
        items = sorted(updates.items())
        arrays = [np.ascontiguousarray(v, dtype=np.float32).reshape(-1, 3) for _, v in items]
        ups = (_abi.rpt_mesh_vertices * max(1, len(items)))()
        for u, (m, _), v in zip(ups, items, arrays):
            u.mesh, u.n_vertices, u.vertices = int(m), v.shape[0], v.ctypes.data_as(C.POINTER(C.c_float))
        self._checked_move(call(self._h, ups, len(items)))
        for (m, _), v in zip(items, arrays):
            _, idx, mat = self._scene.meshes[m]
            self._scene.meshes[m] = (v, idx, mat)
            self._stale_meshes.discard(int(m))

    def _checked_move(self, status):
        """check() for the calls that move meshes: one that failed part-way (RPT_ERR_HIP) has left the context without a scene, so
        there is nothing left to read stale arrays back from — the next upload_scene() uploads the scene as the wrapper has it."""
        if status == _abi.RPT_ERR_HIP:
            self._stale_meshes.clear()
        check(status, self._h)

    def update_meshes_device(self, sources):
        """update_meshes for positions that live in device memory (include/rpt.h, "moving meshes from device memory"): `sources`
        maps a mesh's index to a CUDA float32 contiguous tensor of shape (n_vertices, 3), or to a pair (tensor, transform) —
        `transform` anything np.asarray(..., np.float32).reshape(3, 4) takes, applied on the device while the positions are read.
        The call blocks and has consumed the tensors when it returns.  scene().meshes[m]'s vertex array is stale afterwards;
        mesh_vertices(m) reads the positions the context holds, and upload_scene() refreshes the stale ones first."""
        self._move_meshes_device(lib().rpt_update_meshes_device, sources)

    def rebuild_meshes_device(self, sources=None):
        """rebuild_meshes from device memory: update_meshes_device's arguments.  Without `sources`: a rebuild over the positions
        the context holds."""
        self._move_meshes_device(lib().rpt_rebuild_meshes_device, sources or {})

    def _move_meshes_device(self, call, sources):
        import torch
        items = sorted(sources.items())
        srcs = (_abi.rpt_mesh_source * max(1, len(items)))()
        keep = []
        for s, (m, v) in zip(srcs, items):
            xf = None
            if isinstance(v, (tuple, list)):
                v, xf = v
            if not (isinstance(v, torch.Tensor) and v.is_cuda and v.dtype == torch.float32 and v.is_contiguous() and v.dim() == 2 and
                    v.shape[1] == 3):
                raise ValueError("mesh %d: the source must be a CUDA float32 contiguous tensor of shape (n, 3)" % m)
            s.mesh, s.n_vertices, s.vertices_dev = int(m), v.shape[0], v.data_ptr() if v.shape[0] else None
            if xf is not None:
                xf = np.ascontiguousarray(np.asarray(xf, np.float32).reshape(3, 4))
                s.transform = xf.ctypes.data_as(C.POINTER(C.c_float))
            keep.append((v, xf))
        self._checked_move(call(self._h, srcs, len(items)))
        self._stale_meshes.update(int(m) for m, _ in items)

    def mesh_vertices(self, m):
        """The positions the context holds for mesh `m` (rpt_download_mesh_vertices): a new float32 array of shape (n_vertices, 3)."""
        n = np.asarray(self._scene.meshes[m][0]).reshape(-1, 3).shape[0]
        out = np.empty((n, 3), np.float32)
        check(lib().rpt_download_mesh_vertices(self._h, int(m), out.ctypes.data, n), self._h)
        return out

    def set_mesh_shading(self, modes):
        """Per-mesh shading (include/rpt.h, "smooth mesh shading"): `modes` maps a mesh's index in scene().meshes to "smooth" —
        interpolated vertex normals, which the library computes on the device and keeps current through every call that moves
        the mesh — or "flat".  Meshes not named keep their mode; upload_scene() leaves every mesh flat again, as in C."""
        names = {"flat": _abi.RPT_MESH_SHADING_FLAT, "smooth": _abi.RPT_MESH_SHADING_SMOOTH}
        items = sorted(modes.items())
        its = (_abi.rpt_mesh_shading * max(1, len(items)))()
        for it, (m, mode) in zip(its, items):
            if mode not in names:
                raise ValueError("mesh %d: the mode must be \"smooth\" or \"flat\", not %r" % (m, mode))
            it.mesh, it.mode = int(m), names[mode]
        self._checked_move(lib().rpt_set_mesh_shading(self._h, its, len(items)))

    def mesh_normals(self, m):
        """The vertex normals the context holds for the smooth mesh `m` (rpt_download_mesh_normals): a new float32 array of shape
        (n_vertices, 3)."""
        n = np.asarray(self._scene.meshes[m][0]).reshape(-1, 3).shape[0]
        out = np.empty((n, 3), np.float32)
        check(lib().rpt_download_mesh_normals(self._h, int(m), out.ctypes.data, n), self._h)
        return out

    def set_mesh_lights(self, modes):
        """Mesh lights (include/rpt.h, "mesh lights"): `modes` maps a mesh's index in scene().meshes to True — next-event estimation
        samples the mesh's surface, through a table the library computes on the device and keeps current through every call that
        moves the mesh — or False.  Meshes not named keep their mode; upload_scene() leaves every mesh off again, as in C.  The scene
        needs any_hit_uses_max_dist."""
        items = sorted(modes.items())
        its = (_abi.rpt_mesh_light * max(1, len(items)))()
        for it, (m, on) in zip(its, items):
            if not isinstance(on, (bool, np.bool_)):
                raise ValueError("mesh %d: the mode must be True or False, not %r" % (m, on))
            it.mesh, it.mode = int(m), _abi.RPT_MESH_LIGHT_ON if on else _abi.RPT_MESH_LIGHT_OFF
        self._checked_move(lib().rpt_set_mesh_lights(self._h, its, len(items)))

    def mesh_light_table(self, m):
        """The table the context holds for the mesh light `m` (rpt_download_mesh_light_table): (cdf, exponent, area) — a new uint64
        array with one running sum per triangle of the mesh, the integer E and the float32 A_tot; (zeros, 0, 0.0): the mesh is dark."""
        n = np.asarray(self._scene.meshes[m][1]).reshape(-1, 3).shape[0]
        cdf = np.zeros(n, np.uint64)
        e, area = C.c_int32(0), C.c_float(0.0)
        check(lib().rpt_download_mesh_light_table(self._h, int(m), cdf.ctypes.data, n, C.byref(e), C.byref(area)), self._h)
        return cdf, int(e.value), np.float32(area.value)

    def set_mesh_textures(self, items):
        """Mesh textures (include/rpt.h, "mesh textures"): `items` maps a mesh's index in scene().meshes to None — the mesh loses its
        texture — or to a dict with "uvs" (n_vertices, 2) float32, "texels" (height, width, 4) uint8 RGBA with row 0 at t = 0, and
        optionally "wrap" ("repeat" / "clamp"), "filter" ("bilinear" / "nearest") and "gamma" (1.0: the bytes are linear).  The
        library decodes the image on the device and multiplies it into the mesh material's rgb at every hit.  Meshes not named
        keep their texture; upload_scene() leaves every mesh untextured again, as in C."""
        wraps = {"repeat": _abi.RPT_TEX_WRAP_REPEAT, "clamp": _abi.RPT_TEX_WRAP_CLAMP}
        filters = {"nearest": _abi.RPT_TEX_FILTER_NEAREST, "bilinear": _abi.RPT_TEX_FILTER_BILINEAR}
        items = sorted(items.items())
        its = (_abi.rpt_mesh_texture * max(1, len(items)))()
        keep = []
        for it, (m, tex) in zip(its, items):
            it.mesh = int(m)
            if tex is None:
                continue
            wrap, filt = tex.get("wrap", "repeat"), tex.get("filter", "bilinear")
            if wrap not in wraps or filt not in filters:
                raise ValueError("mesh %d: wrap must be \"repeat\" or \"clamp\" and filter \"nearest\" or \"bilinear\", not %r / %r" % (m, wrap, filt))
            texels = np.ascontiguousarray(tex["texels"], dtype=np.uint8)
            if texels.ndim != 3 or texels.shape[2] != 4:
                raise ValueError("mesh %d: texels must have the shape (height, width, 4)" % m)
            uvs = np.ascontiguousarray(tex["uvs"], dtype=np.float32).reshape(-1, 2)
            keep.append((texels, uvs))
            it.n_vertices, it.uvs = uvs.shape[0], uvs.ctypes.data_as(C.POINTER(C.c_float))
            it.height, it.width, it.texels = texels.shape[0], texels.shape[1], texels.ctypes.data_as(C.POINTER(C.c_uint8))
            it.wrap, it.filter, it.gamma = wraps[wrap], filters[filt], float(tex.get("gamma", 1.0))
        self._checked_move(lib().rpt_set_mesh_textures(self._h, its, len(items)))
        sizes = self.__dict__.setdefault("_texture_sizes", {})
        for it, (m, tex) in zip(its, items):
            sizes[int(m)] = (it.width, it.height)

    def mesh_texture(self, m, width=None, height=None):
        """The decoded texels the context holds for the textured mesh `m` (rpt_download_mesh_texture): a new float32 array of shape
        (height, width, 4), linear values, the fourth 0.  Without a size: the one set_mesh_textures last gave the mesh."""
        if width is None or height is None:
            width, height = self.__dict__.get("_texture_sizes", {}).get(int(m), (0, 0))
        out = np.empty((int(height), int(width), 4), np.float32)
        check(lib().rpt_download_mesh_texture(self._h, int(m), out.ctypes.data, int(width), int(height)), self._h)
        return out

    def set_environment(self, image, scale=1.0, sampled=True):
        """Environment lighting (include/rpt.h, "environment lighting"): `image` is a (size, size, 3) float32 linear RGB image in the
        octahedral layout (scenes.octahedral_from_equirect makes one from a latitude-longitude image) that replaces the background of
        the uploaded mesh scene, times `scale`; with `sampled` it is also one more light of next-event estimation, importance-sampled
        by texel.  None removes it; upload_scene() drops it, as in C."""
        if image is None:
            self._checked_move(lib().rpt_set_environment(self._h, None))
            self.__dict__["_environment_size"] = 0
            return
        texels = np.ascontiguousarray(image, dtype=np.float32)
        if texels.ndim != 3 or texels.shape[2] != 3 or texels.shape[0] != texels.shape[1]:
            raise ValueError("the environment must have the shape (size, size, 3)")
        env = _abi.rpt_environment()
        env.size, env.texels = texels.shape[0], texels.ctypes.data_as(C.POINTER(C.c_float))
        env.scale, env.mode = float(scale), _abi.RPT_ENV_SAMPLED if sampled else _abi.RPT_ENV_BACKGROUND_ONLY
        self._checked_move(lib().rpt_set_environment(self._h, C.byref(env)))
        self.__dict__["_environment_size"] = int(texels.shape[0])

    def download_environment_table(self, size=None):
        """The table the context holds for its sampled environment (rpt_download_environment_table): (cdf, exponent) — a new uint64
        array with one running sum per texel, row 0 first, and the integer E; (zeros, 0): the table is dark.  Without a size: the
        one set_environment last gave."""
        if size is None:
            size = self.__dict__.get("_environment_size", 0)
        cdf = np.zeros(int(size) * int(size), np.uint64)
        e = C.c_int32(0)
        check(lib().rpt_download_environment_table(self._h, cdf.ctypes.data, cdf.size, C.byref(e)), self._h)
        return cdf, int(e.value)

    def set_mesh_cutouts(self, items):
        """Mesh cutouts (include/rpt.h, "mesh cutouts"): `items` maps a mesh's index in scene().meshes to None — the mesh loses its
        cutout — or to a 2-D (height, width) uint8 mask with row 0 at t = 0 (`rgba[..., 3]` of the texture works), or to a dict with
        "alpha" (that array) and optionally "threshold" (1 .. 255, default 128: a texel is opaque when alpha >= threshold).  The mask
        is tested inside the hierarchy walks through the mesh's texture UVs and wrap, so the mesh must be textured.  Meshes not
        named keep their cutout; upload_scene() drops every cutout, as in C."""
        items = sorted(items.items())
        its = (_abi.rpt_mesh_cutout * max(1, len(items)))()
        keep = []
        for it, (m, cut) in zip(its, items):
            it.mesh, it.mode = int(m), _abi.RPT_MESH_CUTOUT_OFF
            if cut is None:
                continue
            threshold = 128
            if isinstance(cut, dict):
                cut, threshold = cut["alpha"], cut.get("threshold", 128)
            alpha = np.asarray(cut)
            if alpha.ndim != 2 or alpha.dtype != np.uint8:
                raise ValueError("mesh %d: the mask must be a 2-D uint8 array (height, width)" % m)
            alpha = np.ascontiguousarray(alpha)
            keep.append(alpha)
            it.mode, it.threshold = _abi.RPT_MESH_CUTOUT_ON, int(threshold)
            it.height, it.width, it.alpha = alpha.shape[0], alpha.shape[1], alpha.ctypes.data_as(C.POINTER(C.c_uint8))
        self._checked_move(lib().rpt_set_mesh_cutouts(self._h, its, len(items)))
        sizes = self.__dict__.setdefault("_cutout_sizes", {})
        for it, (m, cut) in zip(its, items):
            sizes[int(m)] = (it.width, it.height)

    def mesh_cutout(self, m, width=None, height=None):
        """The mask the context holds for the cutout mesh `m` (rpt_download_mesh_cutout): a new bool array of shape (height, width),
        True where the mesh is opaque.  Without a size: the one set_mesh_cutouts last gave the mesh."""
        if width is None or height is None:
            width, height = self.__dict__.get("_cutout_sizes", {}).get(int(m), (0, 0))
        n = int(width) * int(height)
        words = np.zeros((n + 31) // 32, np.uint32)
        check(lib().rpt_download_mesh_cutout(self._h, int(m), words.ctypes.data, words.size), self._h)
        bits = (words[:, None] >> np.arange(32, dtype=np.uint32)[None, :]) & 1
        return bits.reshape(-1)[:n].astype(bool).reshape(int(height), int(width))

    def set_mesh_normal_maps(self, items):
        """Mesh normal maps (include/rpt.h, "mesh normal maps"): `items` maps a mesh's index in scene().meshes to None — the mesh loses
        its map — or to a (height, width, 4) uint8 RGBA tangent-space map with row 0 at t = 0 (scenes.height_to_normal_map makes one),
        or to a dict with "texels" (that array) and optionally "filter" ("bilinear" / "nearest"), "flip_green" (a map authored with
        +y down) and "strength" (0 .. 16, default 1: scales x and y).  The map is looked up through the mesh's texture UVs and wrap at
        every hit and bends the shading normal, so the mesh must be textured.  Meshes not named keep their map; upload_scene()
        drops every map, as in C."""
        filters = {"nearest": _abi.RPT_TEX_FILTER_NEAREST, "bilinear": _abi.RPT_TEX_FILTER_BILINEAR}
        items = sorted(items.items())
        its = (_abi.rpt_mesh_normal_map * max(1, len(items)))()
        keep = []
        for it, (m, nm) in zip(its, items):
            it.mesh, it.mode = int(m), _abi.RPT_MESH_NORMAL_MAP_OFF
            if nm is None:
                continue
            if not isinstance(nm, dict):
                nm = {"texels": nm}
            filt = nm.get("filter", "bilinear")
            if filt not in filters:
                raise ValueError("mesh %d: filter must be \"nearest\" or \"bilinear\", not %r" % (m, filt))
            texels = np.ascontiguousarray(nm["texels"], dtype=np.uint8)
            if texels.ndim != 3 or texels.shape[2] != 4:
                raise ValueError("mesh %d: texels must have the shape (height, width, 4)" % m)
            keep.append(texels)
            it.mode, it.filter = _abi.RPT_MESH_NORMAL_MAP_ON, filters[filt]
            it.flags = _abi.RPT_NORMAL_MAP_FLIP_GREEN if nm.get("flip_green", False) else 0
            it.strength = float(nm.get("strength", 1.0))
            it.height, it.width, it.texels = texels.shape[0], texels.shape[1], texels.ctypes.data_as(C.POINTER(C.c_uint8))
        self._checked_move(lib().rpt_set_mesh_normal_maps(self._h, its, len(items)))
        sizes = self.__dict__.setdefault("_normal_map_sizes", {})
        for it, (m, nm) in zip(its, items):
            sizes[int(m)] = (it.width, it.height)

    def mesh_normal_map(self, m, width=None, height=None):
        """The decoded texels the context holds for the normal-mapped mesh `m` (rpt_download_mesh_normal_map): a new float32 array of
        shape (height, width, 4), {x, y, z, 0}.  Without a size: the one set_mesh_normal_maps last gave the mesh."""
        if width is None or height is None:
            width, height = self.__dict__.get("_normal_map_sizes", {}).get(int(m), (0, 0))
        out = np.empty((int(height), int(width), 4), np.float32)
        check(lib().rpt_download_mesh_normal_map(self._h, int(m), out.ctypes.data, int(width), int(height)), self._h)
        return out

    def set_mesh_material_maps(self, items):
        """Mesh material maps (include/rpt.h, "mesh material maps"): `items` maps a mesh's index in scene().meshes to None — the mesh
        loses its map — or to a (height, width, 4) uint8 RGBA map with row 0 at t = 0, or to a dict with "texels" (that array) and
        optionally "filter" ("bilinear" / "nearest"), "roughness_channel" (0 .. 3 or None, default 1) and "metallic_channel" (default
        2: glTF's metallicRoughness texture).  The map is looked up through the mesh's texture UVs and wrap at every hit and scales
        the material's roughness and metallic, so the mesh must be textured.  Meshes not named keep their map; upload_scene() drops
        every map, as in C."""
        filters = {"nearest": _abi.RPT_TEX_FILTER_NEAREST, "bilinear": _abi.RPT_TEX_FILTER_BILINEAR}
        items = sorted(items.items())
        its = (_abi.rpt_mesh_material_map * max(1, len(items)))()
        keep = []
        for it, (m, mm) in zip(its, items):
            it.mesh, it.mode = int(m), _abi.RPT_MESH_MATERIAL_MAP_OFF
            it.roughness_channel = it.metallic_channel = _abi.RPT_MATERIAL_MAP_CHANNEL_NONE
            if mm is None:
                continue
            if not isinstance(mm, dict):
                mm = {"texels": mm}
            filt = mm.get("filter", "bilinear")
            if filt not in filters:
                raise ValueError("mesh %d: filter must be \"nearest\" or \"bilinear\", not %r" % (m, filt))
            texels = np.ascontiguousarray(mm["texels"], dtype=np.uint8)
            if texels.ndim != 3 or texels.shape[2] != 4:
                raise ValueError("mesh %d: texels must have the shape (height, width, 4)" % m)
            keep.append(texels)
            it.mode, it.filter = _abi.RPT_MESH_MATERIAL_MAP_ON, filters[filt]
            for name, default in (("roughness_channel", 1), ("metallic_channel", 2)):
                c = mm.get(name, default)
                setattr(it, name, _abi.RPT_MATERIAL_MAP_CHANNEL_NONE if c is None else int(c) & 0xFFFFFFFF)
            it.height, it.width, it.texels = texels.shape[0], texels.shape[1], texels.ctypes.data_as(C.POINTER(C.c_uint8))
        self._checked_move(lib().rpt_set_mesh_material_maps(self._h, its, len(items)))
        sizes = self.__dict__.setdefault("_material_map_sizes", {})
        for it, (m, mm) in zip(its, items):
            sizes[int(m)] = (it.width, it.height)

    def mesh_material_map(self, m, width=None, height=None):
        """The decoded texels the context holds for the material-mapped mesh `m` (rpt_download_mesh_material_map): a new float32 array
        of shape (height, width, 4), {fr, fm, 0, 0}.  Without a size: the one set_mesh_material_maps last gave the mesh."""
        if width is None or height is None:
            width, height = self.__dict__.get("_material_map_sizes", {}).get(int(m), (0, 0))
        out = np.empty((int(height), int(width), 4), np.float32)
        check(lib().rpt_download_mesh_material_map(self._h, int(m), out.ctypes.data, int(width), int(height)), self._h)
        return out

    def set_mesh_emission_maps(self, items):
        """Mesh emission maps (include/rpt.h, "mesh emission maps"): `items` maps a mesh's index in scene().meshes to None — the mesh
        loses its map — or to a (height, width, 4) uint8 RGBA map with row 0 at t = 0, or to a dict with "texels" (that array) and
        optionally "filter" ("bilinear" / "nearest") and "gamma" (default 1: the bytes are linear).  The map is looked up through
        the mesh's texture UVs and wrap and scales the material's emission where a path hits the mesh, where the mesh-light sampler
        picks a point on it and at the emitter exit, so the mesh must be textured.  Meshes not named keep their map; upload_scene()
        drops every map, as in C."""
        filters = {"nearest": _abi.RPT_TEX_FILTER_NEAREST, "bilinear": _abi.RPT_TEX_FILTER_BILINEAR}
        items = sorted(items.items())
        its = (_abi.rpt_mesh_emission_map * max(1, len(items)))()
        keep = []
        for it, (m, em) in zip(its, items):
            it.mesh, it.mode, it.gamma = int(m), _abi.RPT_MESH_EMISSION_MAP_OFF, 1.0
            if em is None:
                continue
            if not isinstance(em, dict):
                em = {"texels": em}
            filt = em.get("filter", "bilinear")
            if filt not in filters:
                raise ValueError("mesh %d: filter must be \"nearest\" or \"bilinear\", not %r" % (m, filt))
            texels = np.ascontiguousarray(em["texels"], dtype=np.uint8)
            if texels.ndim != 3 or texels.shape[2] != 4:
                raise ValueError("mesh %d: texels must have the shape (height, width, 4)" % m)
            keep.append(texels)
            it.mode, it.filter, it.gamma = _abi.RPT_MESH_EMISSION_MAP_ON, filters[filt], float(em.get("gamma", 1.0))
            it.height, it.width, it.texels = texels.shape[0], texels.shape[1], texels.ctypes.data_as(C.POINTER(C.c_uint8))
        self._checked_move(lib().rpt_set_mesh_emission_maps(self._h, its, len(items)))
        sizes = self.__dict__.setdefault("_emission_map_sizes", {})
        for it, (m, em) in zip(its, items):
            sizes[int(m)] = (it.width, it.height)

    def download_mesh_emission_map(self, m, width=None, height=None):
        """The decoded texels the context holds for the emission-mapped mesh `m` (rpt_download_mesh_emission_map): a new float32 array
        of shape (height, width, 4), {r, g, b, 0}.  Without a size: the one set_mesh_emission_maps last gave the mesh."""
        if width is None or height is None:
            width, height = self.__dict__.get("_emission_map_sizes", {}).get(int(m), (0, 0))
        out = np.empty((int(height), int(width), 4), np.float32)
        check(lib().rpt_download_mesh_emission_map(self._h, int(m), out.ctypes.data, int(width), int(height)), self._h)
        return out

    def set_mesh_media(self, items):
        """Mesh media (include/rpt.h, "mesh media"): `items` maps a mesh's index in scene().meshes to None — the mesh loses its
        medium — or to a dict with "type" ("absorb", "scatter", "emissive" or None), "density", "color" (three floats) and optionally
        "anisotropy" (default 0; the library clamps it to [-0.9, 0.9]).  The mesh bounds the medium: a path that enters through one
        of its triangles is absorbed, scattered or lit along its way until it leaves through another.  Meshes not named keep their
        medium; upload_scene() drops every medium, as in C."""
        types = {None: _abi.RPT_MEDIUM_NONE, "absorb": _abi.RPT_MEDIUM_ABSORB, "scatter": _abi.RPT_MEDIUM_SCATTER, "emissive": _abi.RPT_MEDIUM_EMISSIVE}
        items = sorted(items.items())
        its = (_abi.rpt_mesh_medium * max(1, len(items)))()
        for it, (m, md) in zip(its, items):
            it.mesh, it.medium_type = int(m), _abi.RPT_MEDIUM_NONE
            if md is None:
                continue
            kind = md.get("type")
            if kind not in types:
                raise ValueError("mesh %d: type must be \"absorb\", \"scatter\", \"emissive\" or None, not %r" % (m, kind))
            color = [float(c) for c in md.get("color", (1.0, 1.0, 1.0))]
            if len(color) != 3:
                raise ValueError("mesh %d: color must have three components" % m)
            it.medium_type, it.density, it.anisotropy = types[kind], float(md.get("density", 0.0)), float(md.get("anisotropy", 0.0))
            it.color[0], it.color[1], it.color[2] = color
        self._checked_move(lib().rpt_set_mesh_media(self._h, its, len(items)))

    def download_mesh_medium(self, m):
        """What the context holds for mesh `m` (rpt_download_mesh_medium): a dict with "type" ("absorb", "scatter", "emissive" or None),
        "density", "color" and "anisotropy" — the clamped value; type None and zeros for a mesh without a medium."""
        names = {_abi.RPT_MEDIUM_NONE: None, _abi.RPT_MEDIUM_ABSORB: "absorb", _abi.RPT_MEDIUM_SCATTER: "scatter", _abi.RPT_MEDIUM_EMISSIVE: "emissive"}
        out = _abi.rpt_mesh_medium()
        check(lib().rpt_download_mesh_medium(self._h, int(m), C.byref(out)), self._h)
        return {"type": names[out.medium_type], "density": np.float32(out.density), "color": tuple(np.float32(c) for c in out.color),
                "anisotropy": np.float32(out.anisotropy)}

    # --- ray queries (include/rpt.h, "ray queries")
    @staticmethod
    def _hit_views(hits, surfaces, as_int):
        """The records as a dict of named views: `hits` [n, 8] and `surfaces` [n, 16] (or None) hold float32 words."""
        out = {"t": hits[:, 0], "kind": as_int(hits[:, 1]), "primitive": as_int(hits[:, 2]), "mesh": as_int(hits[:, 3]),
               "triangle": as_int(hits[:, 4]), "u": hits[:, 5], "v": hits[:, 6]}
        if surfaces is not None:
            out.update(ng=surfaces[:, 0:3], ns=surfaces[:, 3:6], rgb=surfaces[:, 6:9], emission=surfaces[:, 9:12],
                       roughness=surfaces[:, 12], metallic=surfaces[:, 13], material=as_int(surfaces[:, 14]))
        return out

    def _query_rays(self, rays):
        """`rays` checked: ([n, 8] float32, on the device?).  A row is an rpt_ray: origin, max_dist, direction, reserved."""
        if isinstance(rays, np.ndarray):
            if rays.dtype != np.float32 or rays.ndim != 2 or rays.shape[1] != 8:
                raise ValueError("rays must be float32 [n, 8]: origin, max_dist, direction, reserved")
            return np.ascontiguousarray(rays), False
        import torch
        if not (isinstance(rays, torch.Tensor) and rays.is_cuda and rays.dtype == torch.float32 and rays.dim() == 2 and rays.shape[1] == 8):
            raise ValueError("rays must be a float32 [n, 8] numpy array or CUDA tensor: origin, max_dist, direction, reserved")
        if (rays.device.index or 0) != self.device:
            raise ValueError("rays lie on device %s, the tracer on %d" % (rays.device, self.device))
        return rays.contiguous(), True

    def trace(self, rays, surfaces=False):
        """The closest hit of every ray (rpt_trace_rays*): a dict of named views t, kind, primitive, mesh, triangle, u, v and, with
        `surfaces`, ng, ns, rgb, emission, roughness, metallic, material.  A CUDA float32 tensor [n, 8] goes through the device form on
        torch's current stream and returns tensors (the index fields as int32: 0xFFFFFFFF reads -1); a numpy array goes through the host
        form and returns numpy (the index fields as uint32)."""
        rays, on_device = self._query_rays(rays)
        n = int(rays.shape[0])
        if on_device:
            import torch
            hits = torch.empty((n, 8), dtype=torch.float32, device=rays.device)
            surf = torch.empty((n, 16), dtype=torch.float32, device=rays.device) if surfaces else None
            stream = torch.cuda.current_stream(rays.device).cuda_stream
            check(lib().rpt_trace_rays_device(self._h, rays.data_ptr(), n, hits.data_ptr(), surf.data_ptr() if surfaces else None, 0,
                                              C.c_void_p(stream)), self._h)
            return self._hit_views(hits, surf, lambda x: x.view(torch.int32))
        hits = np.empty((n, 8), dtype=np.float32)
        surf = np.empty((n, 16), dtype=np.float32) if surfaces else None
        check(lib().rpt_trace_rays(self._h, rays.ctypes.data, n, hits.ctypes.data, surf.ctypes.data if surfaces else None, 0), self._h)
        return self._hit_views(hits, surf, lambda x: x.view(np.uint32))

    def occluded(self, rays):
        """Whether anything lies along each ray before its max_dist (rpt_occluded*): uint8 [n], a tensor for a CUDA tensor of rays, a
        numpy array for a numpy array."""
        rays, on_device = self._query_rays(rays)
        n = int(rays.shape[0])
        if on_device:
            import torch
            out = torch.empty((n,), dtype=torch.uint8, device=rays.device)
            stream = torch.cuda.current_stream(rays.device).cuda_stream
            check(lib().rpt_occluded_device(self._h, rays.data_ptr(), n, out.data_ptr(), 0, C.c_void_p(stream)), self._h)
            return out
        out = np.empty((n,), dtype=np.uint8)
        check(lib().rpt_occluded(self._h, rays.ctypes.data, n, out.ctypes.data, 0), self._h)
        return out

    def camera_rays(self, width, height):
        """The camera's ray through the centre of every pixel, row 0 on top (rpt_camera_rays_device): a CUDA float32 tensor
        [width * height, 8] on the tracer's device, ready for trace() and occluded()."""
        import torch
        dev = torch.device("cuda", self.device)
        rays = torch.empty((int(width) * int(height), 8), dtype=torch.float32, device=dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
        check(lib().rpt_camera_rays_device(self._h, int(width), int(height), rays.data_ptr(), C.c_void_p(stream)), self._h)
        return rays

    def denoise_guides(self, width, height):
        """First-hit guides of the scene as the camera sees it now (include/rpt.h "guided denoiser"): the camera's rays, traced with
        surfaces, packed — a CUDA float32 tensor [height * width, 16], one rpt_guide per pixel, for DeviceColorBuffer.denoise_guided.
        A static camera packs them once and denoises every progressive frame against them."""
        import torch
        rays = self.camera_rays(width, height)
        n = int(rays.shape[0])
        hits = torch.empty((n, 8), dtype=torch.float32, device=rays.device)
        surf = torch.empty((n, 16), dtype=torch.float32, device=rays.device)
        guides = torch.empty((n, 16), dtype=torch.float32, device=rays.device)
        stream = C.c_void_p(torch.cuda.current_stream(rays.device).cuda_stream)
        check(lib().rpt_trace_rays_device(self._h, rays.data_ptr(), n, hits.data_ptr(), surf.data_ptr(), 0, stream), self._h)
        check(lib().rpt_denoise_guides_device(self._h, rays.data_ptr(), hits.data_ptr(), surf.data_ptr(), n, guides.data_ptr(), stream), self._h)
        return guides

    # --- radiance queries (include/rpt.h, "radiance queries")
    def radiance(self, rays, spp=1, frames_done=0, out=None, first_index=0):
        """The integrator's estimate along every ray (rpt_radiance*): [n, 4] float32, a ColorBuffer pixel per ray — `spp` samples
        blended in as frames `frames_done` ... with the tracer's seed, ray i on the stream of index `first_index` + i.  A CUDA float32
        tensor [n, 8] goes through the device form on torch's current stream and returns a tensor; a numpy array goes through the host
        form and returns numpy.  `out` (same kind, [n, 4] float32, contiguous) accumulates in place; without it the mean starts from zeros."""
        rays, on_device = self._query_rays(rays)
        n = int(rays.shape[0])
        if on_device:
            import torch
            if out is None:
                out = torch.zeros((n, 4), dtype=torch.float32, device=rays.device)
            elif not (isinstance(out, torch.Tensor) and out.is_cuda and out.device == rays.device and out.dtype == torch.float32 and
                      tuple(out.shape) == (n, 4) and out.is_contiguous()):
                raise ValueError("out must be a contiguous float32 [n, 4] CUDA tensor on the rays' device")
            stream = torch.cuda.current_stream(rays.device).cuda_stream
            check(lib().rpt_radiance_device(self._h, rays.data_ptr(), n, out.data_ptr(), int(frames_done), int(spp), self.seed, int(first_index) & 0xFFFFFFFF, 0,
                                            C.c_void_p(stream)), self._h)
            return out
        if out is None:
            out = np.zeros((n, 4), dtype=np.float32)
        elif not (isinstance(out, np.ndarray) and out.dtype == np.float32 and out.shape == (n, 4) and out.flags["C_CONTIGUOUS"]):
            raise ValueError("out must be a C-contiguous float32 [n, 4] numpy array")
        check(lib().rpt_radiance(self._h, rays.ctypes.data, n, out.ctypes.data, int(frames_done), int(spp), self.seed, int(first_index) & 0xFFFFFFFF, 0), self._h)
        return out

    def camera_sample_rays(self, width, height, frame):
        """The rays a render of frame `frame` sends, one per pixel, row 0 on top (rpt_camera_sample_rays_device, the tracer's seed): a
        CUDA float32 tensor [width * height, 8].  radiance() over them with frames_done = frame is that frame's render, word for word."""
        import torch
        dev = torch.device("cuda", self.device)
        rays = torch.empty((int(width) * int(height), 8), dtype=torch.float32, device=dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
        check(lib().rpt_camera_sample_rays_device(self._h, int(width), int(height), int(frame), self.seed, rays.data_ptr(), C.c_void_p(stream)), self._h)
        return rays

    def _refresh_stale_meshes(self):
        """scene().meshes' vertex arrays that a device-source call left stale, read back once (only before an upload)."""
        for m in sorted(self._stale_meshes):
            if m < len(getattr(self._scene, "meshes", ())):
                _, idx, mat = self._scene.meshes[m]
                self._scene.meshes[m] = (self.mesh_vertices(m), idx, mat)
        self._stale_meshes.clear()

    def scene(self):                                               # tracer.rs:629-631
        return self._scene

    def render(self, buffer):
        """Render one frame and accumulate into the pixels buffer (tracer.rs:21-123)."""
        self.render_n(buffer, 1)

    def render_n(self, buffer, spp):
        """`spp` consecutive render() calls folded into one launch; bit-identical to them."""
        if isinstance(buffer, ColorBuffer):
            assert buffer.pixels.dtype == np.float32 and buffer.pixels.size == buffer.width * buffer.height * 4
            check(lib().rpt_render(self._h, buffer.pixels.ctypes.data, buffer.width, buffer.height, buffer.frames,
                                   spp, self.seed, self.flags), self._h)
        else:
            import torch
            px = buffer.pixels
            assert px.is_cuda and px.is_contiguous() and px.dtype == torch.float32
            assert (px.device.index or 0) == self.device
            stream = torch.cuda.current_stream(px.device).cuda_stream
            check(lib().rpt_render_device(self._h, px.data_ptr(), buffer.width, buffer.height, buffer.frames, spp,
                                          self.seed, self.flags, buffer.height, 0, 1, C.c_void_p(stream)), self._h)
        buffer.frames += spp                                       # tracer.rs:121

    # --- resident ColorBuffer: the interactive loop of renderer/src/main.rs:113-124 without the PCIe round trip
    def render_resident(self, width, height, spp=1):
        check(lib().rpt_resident_render(self._h, width, height, spp, self.seed, self.flags), self._h)

    def resident_frames(self):
        f = C.c_uint64(0)
        check(lib().rpt_resident_frames(self._h, C.byref(f)), self._h)
        return f.value

    def resident_to_host(self, width, height):
        """Collective on a multi-process tracer; every rank gets a ColorBuffer, only rank 0's is filled."""
        b = ColorBuffer(width, height)
        check(lib().rpt_resident_download(self._h, b.pixels.ctypes.data), self._h)
        b.frames = self.resident_frames()
        return b

    def resident_to_u8(self, width, height, frame=None):
        """buffer.convert_to_u8(frame) on the device + the 4 B per pixel over PCIe.  `frame`: the caller's uint8 array
        (renderer/src/main.rs:122 passes the window's); None: the tracer's own page-locked frame, REUSED by the next call."""
        if frame is None:
            n = width * height * 4
            if self._frame is None or self._frame.size != n:
                self._drop_frame()
                self._frame = np.zeros(n, dtype=np.uint8)
                check(lib().rpt_host_pin(self._frame.ctypes.data, n))
            frame = self._frame
        assert frame.dtype == np.uint8 and frame.size == width * height * 4
        check(lib().rpt_resident_download_u8(self._h, frame.ctypes.data), self._h)
        return frame

    def _drop_frame(self):
        if getattr(self, "_frame", None) is not None:
            lib().rpt_host_unpin(self._frame.ctypes.data)
            self._frame = None

    def resident_reset(self):
        check(lib().rpt_resident_reset(self._h), self._h)

    def resident_upload(self, buffer):
        """Start the resident buffer from a host ColorBuffer (resume; each rank takes the rows it owns)."""
        assert buffer.pixels.dtype == np.float32 and buffer.pixels.size == buffer.width * buffer.height * 4
        check(lib().rpt_resident_upload(self._h, buffer.pixels.ctypes.data, buffer.width, buffer.height, buffer.frames), self._h)

    def resident_gather(self, image=None):
        """Enqueue the assembly of the resident image on the root device (RCCL gather over xGMI + scatter kernel).
        image: a [h, w, 4] f32 CUDA tensor on rank 0's device, or None (the library's own staging image)."""
        check(lib().rpt_resident_gather_device(self._h, image.data_ptr() if image is not None else None), self._h)

    def resident_sync(self):
        check(lib().rpt_resident_sync(self._h), self._h)

    def resident_kernel_ms(self):
        ms = C.c_float(0.0)
        check(lib().rpt_resident_kernel_ms(self._h, C.byref(ms)), self._h)
        return ms.value

    def render_tile(self, tile_pixels, width, height, frames_done, spp, tile_rows, rank, world):
        """Render this rank's rows of a row-tiled image into its compact tile tensor."""
        import torch
        assert tile_pixels.is_cuda and tile_pixels.is_contiguous() and tile_pixels.dtype == torch.float32
        stream = torch.cuda.current_stream(tile_pixels.device).cuda_stream
        check(lib().rpt_render_device(self._h, tile_pixels.data_ptr(), width, height, frames_done, spp, self.seed, self.flags,
                                      tile_rows, rank, world, C.c_void_p(stream)), self._h)

    def close(self):
        self._drop_frame()
        if self._h:
            lib().rpt_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
