"""The mesh scene (rust_pathtracer_amd.scenes.mesh_scene: ~3.9e5 triangles) at 1920x1080 on one GPU: prints ONE JSON line with
Gsamples/s of the resident render, the triangle and BVH node counts, the BVH's depth and build time (host, inside the upload) and the
whole upload's time.  Loads the test build (its rpt_debug_mesh_stats, include/rpt_test.h).

--update: one JSON line more, for rpt_update_meshes (include/rpt.h, "moving meshes").  For a small, a medium and a large move of the
scene (scenes.mesh_scene_moved, phases 0.05 / 0.5 / 2.0), alternating, `--reps` times each in one process: the wall time of
update_meshes (the host's clock around the blocking call) from the uploaded scene to the moved one; the wall time of upload_scene()
of the same moved scene (the existing path: the yardstick); and the resident render rate after each, from resident_kernel_ms.

--rebuild: one JSON line more, for rpt_rebuild_meshes (include/rpt.h, "rebuilding a moved mesh's hierarchy"), in the same shape.  For
the same three moves, alternating, `--reps` times each (at least 5) in one process: the wall time of rebuild_meshes, of upload_scene()
of the same moved scene on a second context (the unchanged path: the yardstick) and of update_meshes on a third (which refits the
ORIGINAL scene's hierarchy); the resident render rate after each of the three; the rebuilt node count and depth; the context's first
rebuild apart (it allocates); and the rates of the unmoved scene, rebuilt and uploaded.  RPT_BUILD_LEAF (csrc/knobs.h) sets the
leaf target of the run.

--device: one JSON line more, for rpt_update_meshes_device / rpt_rebuild_meshes_device (include/rpt.h, "moving meshes from device
memory").  For the same three moves, alternating, `--reps` times each (at least 5) in one process, one context per column: the wall
time of update_meshes and rebuild_meshes from host arrays (unchanged code: the yardsticks, to be compared with the figures
include/rpt.h records for them); of the two device forms without a transform on the same positions held in CUDA tensors; of the two
device forms moving the torus alone, rigidly, from a rest tensor by a matrix; and each device form's first call apart (it allocates).

--smooth: one JSON line more, for smooth mesh shading (include/rpt.h, "smooth mesh shading"), in one process, the two sides of each
comparison alternating `--reps` times (at least 5): the resident render rate of the scene flat and with both meshes SMOOTH, on two
contexts; the wall time of update_meshes, rebuild_meshes and their device forms for the medium move and back, on a context whose
meshes are SMOOTH against one whose meshes are FLAT (one pair of contexts per call); and the time of rpt_set_mesh_shading itself.

--lights: one JSON line more, for mesh lights (include/rpt.h, "mesh lights"), in the same manner: the resident render rate of the
scene with its torus emissive, every mesh OFF against the torus ON, on two contexts; the wall time of the four move calls on a
context whose torus is ON against one whose meshes are OFF; and the time of rpt_set_mesh_lights itself.

--textures: one JSON line more, for mesh textures (include/rpt.h, "mesh textures"), in the same manner: the resident render rate of
the scene untextured against both meshes under a 1024 x 1024 BILINEAR / REPEAT texture, on two contexts; the wall time of the four
move calls on a textured context against an untextured one; and the time of rpt_set_mesh_textures itself.

--environment: one JSON line more, for environment lighting (include/rpt.h, "environment lighting"): the resident render rate of
the scene without an environment, with a BACKGROUND_ONLY one and with a SAMPLED one (1024 x 1024, a dim sky with a small sun), on
three contexts, alternating; and the time of rpt_set_environment itself, for either mode.

--cutouts: one JSON line more, for mesh cutouts (include/rpt.h, "mesh cutouts"): the resident render rate of the scene textured as
--textures does with no mask ("textured": the textured kernel, unchanged), under a 1024 x 1024 checker mask on both meshes ("checker":
rays pass through holes, so it may be faster or slower) and under an all-opaque mask ("opaque": the pure cost of the test), on three
contexts, alternating; the time of rpt_set_mesh_cutouts itself; and the wall time of the four move calls with and without masks.

--normal-maps: one JSON line more, for mesh normal maps (include/rpt.h, "mesh normal maps"): the resident render rate of the scene
textured as --textures does with no map ("textured": the textured kernel, unchanged), under a flat 1024 x 1024 map on both meshes
("flat": the pure cost of the lookup, the bend returns at its first line) and under a 1024 x 1024 BILINEAR bump map ("bump"), on three
contexts, alternating; the time of rpt_set_mesh_normal_maps itself; and the wall time of the four move calls with and without maps.

--material-maps: one JSON line more, for mesh material maps (include/rpt.h, "mesh material maps"): the resident render rate of the
scene textured as --textures does with no map ("textured": the textured kernel, unchanged), under an all-255 1024 x 1024 map on both
meshes ("ones": the pure cost of the lookup, both factors are exactly 1) and under a 1024 x 1024 BILINEAR noise map ("noise"), on three
contexts, alternating; the time of rpt_set_mesh_material_maps itself; and the wall time of the four move calls with and without maps.

--emission-maps: one JSON line more, for mesh emission maps (include/rpt.h, "mesh emission maps"): the resident render rate of the
scene textured as --textures does, its torus emissive and ON, with no map ("lit": the textured mesh-light kernel, unchanged), under an
all-255 1024 x 1024 map on the torus ("ones": the pure cost of the lookups, every factor is exactly 1) and under a 1024 x 1024 BILINEAR
noise map ("noise"), on three contexts, alternating; the time of rpt_set_mesh_emission_maps itself; and the wall time of the four move
calls with and without maps.

--media: one JSON line more, for mesh media (include/rpt.h, "mesh media"): the resident render rate of the scene with its icosphere made
glass and the shadow rays' flag, with no medium ("none": the mesh kernel the scene always ran, a form below 28), with an ABSORB medium
on the glass mesh ("absorb") and with a SCATTER medium on it ("scatter"), on three contexts, alternating; the time of rpt_set_mesh_media
itself; and the wall time of the four move calls with and without a medium.

--rays: one JSON line more, for ray queries (include/rpt.h, "ray queries"), on the scene as it is: the camera's 1080p rays
(rpt_camera_rays_device: coherent) and as many random rays through the scene's box (a uniform origin in the box of the meshes grown
by a half, a uniform direction: incoherent).  For either set, rays per second of the closest hit, of the closest hit with surfaces
and of occlusion (max_dist = +inf), each timed with device events around 20 launches in a row, medians of `--reps` (at least 5); the
1-spp resident render of the same frame next to them, alternating with the closest hit of the camera's rays, and the ratio of that
rate to the frame's samples per second; the time of rpt_camera_rays_device; and what the camera's rays hit.

--radiance: one JSON line more, for radiance queries (include/rpt.h, "radiance queries"), on scenes.mesh_scene() as it is ("flat": its
render takes form 11, the query the all-tables form over empty tables) and on scenes.mesh_media_scene() with its medium set
("media": render and query run the same arithmetic over the same tables).  Per scene, alternating, medians of `--reps` (at least 5):
Msamples/s of Tracer.radiance over the camera's sample rays of frame 0 at `--spp` samples — the work of a frame — timed with device
events around the call, and of the resident render of that frame (resident_kernel_ms); their ratio; and a probe-style batch, 2 000 000
random rays through the box of the meshes grown by a half at `--spp` samples.

    python tools/mesh_bench.py [--spp 16] [--reps 5] [--update] [--rebuild] [--device] [--smooth] [--lights] [--textures] [--environment]
                               [--cutouts] [--normal-maps] [--material-maps] [--emission-maps] [--media] [--rays] [--radiance]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--update", action="store_true")
    ap.add_argument("--rebuild", action="store_true")
    ap.add_argument("--device", action="store_true")
    ap.add_argument("--smooth", action="store_true")
    ap.add_argument("--lights", action="store_true")
    ap.add_argument("--textures", action="store_true")
    ap.add_argument("--environment", action="store_true")
    ap.add_argument("--cutouts", action="store_true")
    ap.add_argument("--normal-maps", action="store_true")
    ap.add_argument("--material-maps", action="store_true")
    ap.add_argument("--emission-maps", action="store_true")
    ap.add_argument("--media", action="store_true")
    ap.add_argument("--rays", action="store_true")
    ap.add_argument("--radiance", action="store_true")
    a = ap.parse_args()
    os.environ.setdefault("RPT_LIB", os.path.join(ROOT, "rust-pathtracer_amd", "librpt_hip_test.so"))     # (the product has no hooks)
    import __graft_entry__
    pkg = __graft_entry__._load_package()
    from rust_pathtracer_amd import scenes
    s = scenes.mesh_scene()
    n_tris = sum(len(t) for _, t, _ in s.meshes)
    t = pkg.Tracer(pkg.AnalyticalScene(), device=0, seed=1)
    t._scene = s
    t0 = time.perf_counter()
    t.upload_scene()                                                # validation, flattening, BVH build, upload
    upload_s = time.perf_counter() - t0
    nodes, depth, build_ms = C.c_uint32(0), C.c_uint32(0), C.c_float(0.0)
    pkg._lib.check(pkg.lib().rpt_debug_mesh_stats(t._h, C.byref(nodes), C.byref(depth), C.byref(build_ms)), t._h)
    t.render_resident(a.width, a.height, a.spp)                     # warm-up (and the dispatch order's first costs)
    t.resident_sync()
    rates = []
    for _ in range(a.reps):
        t.render_resident(a.width, a.height, a.spp)
        ms = t.resident_kernel_ms()
        rates.append(a.width * a.height * a.spp / (ms * 1e-3) / 1e9)
    update = measure_updates(pkg, t, s, a) if a.update else None
    rebuild = measure_rebuilds(pkg, s, a) if a.rebuild else None
    device = measure_device_sources(pkg, s, a) if a.device else None
    smooth = measure_smooth(pkg, s, a) if a.smooth else None
    lights = measure_lights(pkg, s, a) if a.lights else None
    textures = measure_textures(pkg, s, a) if a.textures else None
    environment = measure_environment(pkg, a) if a.environment else None
    cutouts = measure_cutouts(pkg, s, a) if a.cutouts else None
    normal_maps = measure_normal_maps(pkg, s, a) if a.normal_maps else None
    material_maps = measure_material_maps(pkg, s, a) if a.material_maps else None
    emission_maps = measure_emission_maps(pkg, s, a) if a.emission_maps else None
    media = measure_media(pkg, s, a) if a.media else None
    rays = measure_rays(pkg, s, a) if a.rays else None
    radiance = measure_radiance(pkg, a) if a.radiance else None
    t.close()
    print(json.dumps({"workload": "mesh_scene %dx%d x %d spp, resident" % (a.width, a.height, a.spp), "triangles": n_tris,
                      "gsamples_per_s_median": sorted(rates)[len(rates) // 2], "gsamples_per_s": rates,
                      "bvh_nodes": nodes.value, "bvh_depth": depth.value, "bvh_build_ms": build_ms.value, "upload_s": upload_s}))
    if update:
        print(json.dumps(update))
    if rebuild:
        print(json.dumps(rebuild))
    if device:
        print(json.dumps(device))
    if smooth:
        print(json.dumps(smooth))
    if lights:
        print(json.dumps(lights))
    if textures:
        print(json.dumps(textures))
    if environment:
        print(json.dumps(environment))
    if cutouts:
        print(json.dumps(cutouts))
    if normal_maps:
        print(json.dumps(normal_maps))
    if material_maps:
        print(json.dumps(material_maps))
    if emission_maps:
        print(json.dumps(emission_maps))
    if media:
        print(json.dumps(media))
    if rays:
        print(json.dumps(rays))
    if radiance:
        print(json.dumps(radiance))


def measure_updates(pkg, t, s, a):
    """-> the --update line.  `t` holds `s` uploaded and warmed up; it is never uploaded to again, so every update refits the
    ORIGINAL scene's hierarchy.  The yardstick runs on a second context of the same process."""
    import numpy as np
    from rust_pathtracer_amd import scenes
    original = [np.array(v, np.float32, copy=True) for v, _, _ in s.meshes]

    def rate(tr):
        tr.resident_reset()
        tr.render_resident(a.width, a.height, a.spp)                # the dispatch order's first costs after an upload
        tr.render_resident(a.width, a.height, a.spp)
        return a.width * a.height * a.spp / (tr.resident_kernel_ms() * 1e-3) / 1e9

    def stats(xs):
        xs = sorted(xs)
        return {"median": xs[len(xs) // 2], "min": xs[0], "max": xs[-1]}

    phases = (("small", 0.05), ("medium", 0.5), ("large", 2.0))
    moved = {name: scenes.mesh_scene_moved(s, phase) for name, phase in phases}
    res = {name: {"update_ms": [], "upload_ms": [], "rate_update": [], "rate_upload": []} for name, _ in phases}
    fresh_scene = scenes.mesh_scene()
    fresh = pkg.Tracer(fresh_scene, device=0, seed=1)
    t0 = time.perf_counter()
    t.update_meshes(dict(enumerate(original)))                      # the context's first update: allocates the device's refit tables
    first_ms = (time.perf_counter() - t0) * 1e3
    reps = max(5, a.reps)
    for _ in range(reps):
        for name, _ in phases:
            r = res[name]
            t0 = time.perf_counter()
            t.update_meshes(dict(enumerate(moved[name])))
            r["update_ms"].append((time.perf_counter() - t0) * 1e3)
            r["rate_update"].append(rate(t))
            fresh_scene.meshes = [(v, idx, m) for v, (_, idx, m) in zip(moved[name], fresh_scene.meshes)]
            t0 = time.perf_counter()
            fresh.upload_scene()                                    # the same moved scene through the existing path
            r["upload_ms"].append((time.perf_counter() - t0) * 1e3)
            r["rate_upload"].append(rate(fresh))
    fresh.close()
    out = {"workload": "mesh_scene update %dx%d x %d spp, resident" % (a.width, a.height, a.spp), "reps": reps, "first_update_ms": first_ms}
    for name, phase in phases:
        r = res[name]
        up, full = stats(r["update_ms"]), stats(r["upload_ms"])
        ru, rf = stats(r["rate_update"]), stats(r["rate_upload"])
        out[name] = {"phase": phase, "update_ms": up, "upload_ms": full, "upload_over_update": full["median"] / up["median"],
                     "gsamples_per_s_after_update": ru, "gsamples_per_s_after_upload": rf,
                     "fresh_upload_renders_faster_by_percent": (rf["median"] / ru["median"] - 1.0) * 100.0}
    return out


def measure_rebuilds(pkg, s, a):
    """-> the --rebuild line.  Three contexts of this process over the same scene: one that rebuilds, one that is uploaded to (the
    yardstick), one that only ever updates (every update refits the ORIGINAL hierarchy, as in --update)."""
    import numpy as np
    from rust_pathtracer_amd import scenes
    original = [np.array(v, np.float32, copy=True) for v, _, _ in s.meshes]

    def rate(tr):
        tr.resident_reset()
        tr.render_resident(a.width, a.height, a.spp)                # the dispatch order's first costs
        tr.render_resident(a.width, a.height, a.spp)
        return a.width * a.height * a.spp / (tr.resident_kernel_ms() * 1e-3) / 1e9

    def stats(xs):
        xs = sorted(xs)
        return {"median": xs[len(xs) // 2], "min": xs[0], "max": xs[-1]}

    def mesh_stats(tr):
        nodes, depth, ms = C.c_uint32(0), C.c_uint32(0), C.c_float(0.0)
        pkg._lib.check(pkg.lib().rpt_debug_mesh_stats(tr._h, C.byref(nodes), C.byref(depth), C.byref(ms)), tr._h)
        return nodes.value, depth.value

    phases = (("small", 0.05), ("medium", 0.5), ("large", 2.0))
    moved = {name: scenes.mesh_scene_moved(s, phase) for name, phase in phases}
    keys = ("rebuild_ms", "upload_ms", "update_ms", "rate_rebuild", "rate_upload", "rate_update")
    res = {name: {k: [] for k in keys} for name, _ in phases}
    built = pkg.Tracer(scenes.mesh_scene(), device=0, seed=1)
    fresh_scene = scenes.mesh_scene()
    fresh = pkg.Tracer(fresh_scene, device=0, seed=1)
    refit = pkg.Tracer(scenes.mesh_scene(), device=0, seed=1)
    uploaded_stats = mesh_stats(fresh)
    rate_unmoved_upload = rate(fresh)
    t0 = time.perf_counter()
    built.rebuild_meshes()                                          # the context's first rebuild: allocates the device's tables
    first_ms = (time.perf_counter() - t0) * 1e3
    rate_unmoved_rebuild = rate(built)
    unmoved_stats = mesh_stats(built)
    refit.update_meshes(dict(enumerate(original)))
    reps = max(5, a.reps)
    shape = {}
    for _ in range(reps):
        for name, _ in phases:
            r = res[name]
            t0 = time.perf_counter()
            built.rebuild_meshes(dict(enumerate(moved[name])))
            r["rebuild_ms"].append((time.perf_counter() - t0) * 1e3)
            r["rate_rebuild"].append(rate(built))
            shape[name] = mesh_stats(built)
            fresh_scene.meshes = [(v, idx, m) for v, (_, idx, m) in zip(moved[name], fresh_scene.meshes)]
            t0 = time.perf_counter()
            fresh.upload_scene()
            r["upload_ms"].append((time.perf_counter() - t0) * 1e3)
            r["rate_upload"].append(rate(fresh))
            t0 = time.perf_counter()
            refit.update_meshes(dict(enumerate(moved[name])))
            r["update_ms"].append((time.perf_counter() - t0) * 1e3)
            r["rate_update"].append(rate(refit))
    for tr in (built, fresh, refit):
        tr.close()
    out = {"workload": "mesh_scene rebuild %dx%d x %d spp, resident" % (a.width, a.height, a.spp), "reps": reps,
           "leaf_target": os.environ.get("RPT_BUILD_LEAF", "default"), "first_rebuild_ms": first_ms,
           "unmoved": {"gsamples_per_s_after_rebuild": rate_unmoved_rebuild, "gsamples_per_s_after_upload": rate_unmoved_upload,
                       "rebuild_over_upload_rate": rate_unmoved_rebuild / rate_unmoved_upload,
                       "rebuilt_nodes": unmoved_stats[0], "rebuilt_depth": unmoved_stats[1],
                       "uploaded_nodes": uploaded_stats[0], "uploaded_depth": uploaded_stats[1]}}
    for name, phase in phases:
        r = res[name]
        rb, full, up = stats(r["rebuild_ms"]), stats(r["upload_ms"]), stats(r["update_ms"])
        rr, rf, ru = stats(r["rate_rebuild"]), stats(r["rate_upload"]), stats(r["rate_update"])
        out[name] = {"phase": phase, "rebuild_ms": rb, "upload_ms": full, "update_ms": up, "upload_over_rebuild": full["median"] / rb["median"],
                     "gsamples_per_s_after_rebuild": rr, "gsamples_per_s_after_upload": rf, "gsamples_per_s_after_update": ru,
                     "rebuild_over_upload_rate": rr["median"] / rf["median"], "rebuild_over_update_rate": rr["median"] / ru["median"],
                     "rebuilt_nodes": shape[name][0], "rebuilt_depth": shape[name][1]}
    return out


def measure_device_sources(pkg, s, a):
    """-> the --device line.  Six contexts of this process over the same scene, one per column, so that every column's calls follow
    calls of its own kind; within a repetition the columns alternate."""
    import numpy as np
    import torch
    from rust_pathtracer_amd import scenes
    original = [np.array(v, np.float32, copy=True) for v, _, _ in s.meshes]

    def stats(xs):
        xs = sorted(xs)
        return {"median": xs[len(xs) // 2], "min": xs[0], "max": xs[-1]}

    def timed(call, arg):
        t0 = time.perf_counter()
        call(arg)
        return (time.perf_counter() - t0) * 1e3

    phases = (("small", 0.05), ("medium", 0.5), ("large", 2.0))
    moved = {name: scenes.mesh_scene_moved(s, phase) for name, phase in phases}
    on_device = {name: [torch.from_numpy(np.ascontiguousarray(v, np.float32)).to("cuda:0") for v in moved[name]] for name, _ in phases}
    rest = torch.from_numpy(original[1]).to("cuda:0")               # the torus's rest pose, and a turn about its own axis per move
    centre = 0.5 * (original[1].min(0) + original[1].max(0)).astype(np.float64)
    matrix = {}
    for name, phase in phases:
        c, si = np.cos(phase), np.sin(phase)
        rot = np.array([[c, -si, 0.0], [si, c, 0.0], [0.0, 0.0, 1.0]])
        matrix[name] = np.concatenate([rot, (centre - rot @ centre)[:, None]], axis=1).astype(np.float32)
    torch.cuda.synchronize()
    columns = ("update_host", "rebuild_host", "update_device", "rebuild_device", "update_device_rigid", "rebuild_device_rigid")
    ctx = {c: pkg.Tracer(scenes.mesh_scene(), device=0, seed=1) for c in columns}
    first = {"update_host": timed(ctx["update_host"].update_meshes, dict(enumerate(original))),
             "rebuild_host": timed(ctx["rebuild_host"].rebuild_meshes, dict(enumerate(original))),
             "update_device": timed(ctx["update_device"].update_meshes_device, dict(enumerate(on_device["small"]))),
             "rebuild_device": timed(ctx["rebuild_device"].rebuild_meshes_device, dict(enumerate(on_device["small"]))),
             "update_device_rigid": timed(ctx["update_device_rigid"].update_meshes_device, {1: (rest, matrix["small"])}),
             "rebuild_device_rigid": timed(ctx["rebuild_device_rigid"].rebuild_meshes_device, {1: (rest, matrix["small"])})}
    res = {name: {c: [] for c in columns} for name, _ in phases}
    reps = max(5, a.reps)
    for _ in range(reps):
        for name, _ in phases:
            r = res[name]
            r["update_host"].append(timed(ctx["update_host"].update_meshes, dict(enumerate(moved[name]))))
            r["update_device"].append(timed(ctx["update_device"].update_meshes_device, dict(enumerate(on_device[name]))))
            r["update_device_rigid"].append(timed(ctx["update_device_rigid"].update_meshes_device, {1: (rest, matrix[name])}))
            r["rebuild_host"].append(timed(ctx["rebuild_host"].rebuild_meshes, dict(enumerate(moved[name]))))
            r["rebuild_device"].append(timed(ctx["rebuild_device"].rebuild_meshes_device, dict(enumerate(on_device[name]))))
            r["rebuild_device_rigid"].append(timed(ctx["rebuild_device_rigid"].rebuild_meshes_device, {1: (rest, matrix[name])}))
    # the device forms hold what the host forms hold (the timing ran the same moves)
    same = all(np.array_equal(ctx["update_host"].mesh_vertices(m).view(np.uint32), ctx["update_device"].mesh_vertices(m).view(np.uint32)) and
               np.array_equal(ctx["rebuild_host"].mesh_vertices(m).view(np.uint32), ctx["rebuild_device"].mesh_vertices(m).view(np.uint32))
               for m in range(len(original)))
    for tr in ctx.values():
        tr.close()
    out = {"workload": "mesh_scene device sources, %d vertices" % sum(len(v) for v in original), "reps": reps,
           "first_call_ms": first, "device_forms_hold_the_host_forms_positions": bool(same)}
    for name, phase in phases:
        out[name] = {"phase": phase}
        out[name].update({c + "_ms": stats(res[name][c]) for c in columns})
    return out


def measure_smooth(pkg, s, a):
    """-> the --smooth line.  Two contexts for the frames and two per move call, one FLAT and one with both meshes SMOOTH, so that
    every context's calls follow calls of its own kind; within a repetition the two sides alternate."""
    import numpy as np
    import torch
    from rust_pathtracer_amd import scenes
    original = [np.array(v, np.float32, copy=True) for v, _, _ in s.meshes]
    both = {0: "smooth", 1: "smooth"}

    def stats(xs):
        xs = sorted(xs)
        return {"median": xs[len(xs) // 2], "min": xs[0], "max": xs[-1]}

    def timed(call, arg):
        t0 = time.perf_counter()
        call(arg)
        return (time.perf_counter() - t0) * 1e3

    def rate(tr):
        tr.render_resident(a.width, a.height, a.spp)
        return a.width * a.height * a.spp / (tr.resident_kernel_ms() * 1e-3) / 1e9

    reps = max(5, a.reps)
    # frames
    flat, smooth = pkg.Tracer(scenes.mesh_scene(), device=0, seed=1), pkg.Tracer(scenes.mesh_scene(), device=0, seed=1)
    first_shading_ms = timed(smooth.set_mesh_shading, both)         # brings the refit tables, reads the corners back, builds the lists
    again_ms = [timed(smooth.set_mesh_shading, both) for _ in range(reps)]
    for tr in (flat, smooth):
        rate(tr)                                                    # warm-up (and the dispatch order's first costs)
        rate(tr)
    rates = {"flat": [], "smooth": []}
    for _ in range(reps):
        rates["flat"].append(rate(flat))
        rates["smooth"].append(rate(smooth))
    flat.close()
    smooth.close()
    # moves: the medium move and back, so that every call moves every vertex
    moved = scenes.mesh_scene_moved(s, 0.5)
    dev = lambda arrays: {m: torch.from_numpy(np.ascontiguousarray(v, np.float32)).to("cuda:0") for m, v in enumerate(arrays)}   # noqa: E731
    there, back = {"host": dict(enumerate(moved)), "device": dev(moved)}, {"host": dict(enumerate(original)), "device": dev(original)}
    torch.cuda.synchronize()
    calls = (("update_meshes", "host"), ("rebuild_meshes", "host"), ("update_meshes_device", "device"), ("rebuild_meshes_device", "device"))
    out = {"workload": "mesh_scene smooth shading %dx%d x %d spp, resident" % (a.width, a.height, a.spp), "reps": reps,
           "first_set_mesh_shading_ms": first_shading_ms, "set_mesh_shading_again_ms": stats(again_ms),
           "gsamples_per_s_flat": stats(rates["flat"]), "gsamples_per_s_smooth": stats(rates["smooth"]),
           "smooth_over_flat_rate": stats(rates["smooth"])["median"] / stats(rates["flat"])["median"]}
    for name, where in calls:
        pair = {"flat": pkg.Tracer(scenes.mesh_scene(), device=0, seed=1), "smooth": pkg.Tracer(scenes.mesh_scene(), device=0, seed=1)}
        pair["smooth"].set_mesh_shading(both)
        for tr in pair.values():
            getattr(tr, name)(back[where])                          # the context's first call of its kind: allocates
        ms = {"flat": [], "smooth": []}
        for _ in range(reps):
            for arg in (there[where], back[where]):
                for side in ("flat", "smooth"):
                    ms[side].append(timed(getattr(pair[side], name), arg))
        for tr in pair.values():
            tr.close()
        fl, sm = stats(ms["flat"]), stats(ms["smooth"])
        out[name] = {"flat_ms": fl, "smooth_ms": sm, "smooth_adds_ms": sm["median"] - fl["median"]}
    return out


def measure_lights(pkg, s, a):
    """-> the --lights line.  scenes.mesh_scene() with its torus emissive and the shadow rays' flag (mesh lights need it).  Two
    contexts for the frames and two per move call, one with every mesh OFF and one with the torus ON, so that every context's calls
    follow calls of its own kind; within a repetition the two sides alternate."""
    import numpy as np
    import torch
    from rust_pathtracer_amd import scenes

    def make():
        sc = scenes.mesh_scene()
        sc.any_hit_uses_max_dist = True
        sc.materials[1].fields["emission"] = (4.0, 3.0, 2.0)
        return sc

    original = [np.array(v, np.float32, copy=True) for v, _, _ in s.meshes]
    torus_on = {1: True}

    def stats(xs):
        xs = sorted(xs)
        return {"median": xs[len(xs) // 2], "min": xs[0], "max": xs[-1]}

    def timed(call, arg):
        t0 = time.perf_counter()
        call(arg)
        return (time.perf_counter() - t0) * 1e3

    def rate(tr):
        tr.render_resident(a.width, a.height, a.spp)
        return a.width * a.height * a.spp / (tr.resident_kernel_ms() * 1e-3) / 1e9

    reps = max(5, a.reps)
    # frames
    off, on = pkg.Tracer(make(), device=0, seed=1), pkg.Tracer(make(), device=0, seed=1)
    first_ms = timed(on.set_mesh_lights, torus_on)                  # brings the refit tables, reads the corners back, builds the table
    again_ms = [timed(on.set_mesh_lights, torus_on) for _ in range(reps)]
    for tr in (off, on):
        rate(tr)                                                    # warm-up (and the dispatch order's first costs)
        rate(tr)
    rates = {"off": [], "on": []}
    for _ in range(reps):
        rates["off"].append(rate(off))
        rates["on"].append(rate(on))
    off.close()
    on.close()
    # moves: the medium move and back, so that every call moves every vertex
    moved = scenes.mesh_scene_moved(s, 0.5)
    dev = lambda arrays: {m: torch.from_numpy(np.ascontiguousarray(v, np.float32)).to("cuda:0") for m, v in enumerate(arrays)}   # noqa: E731
    there, back = {"host": dict(enumerate(moved)), "device": dev(moved)}, {"host": dict(enumerate(original)), "device": dev(original)}
    torch.cuda.synchronize()
    calls = (("update_meshes", "host"), ("rebuild_meshes", "host"), ("update_meshes_device", "device"), ("rebuild_meshes_device", "device"))
    out = {"workload": "mesh_scene mesh lights %dx%d x %d spp, resident" % (a.width, a.height, a.spp), "reps": reps,
           "first_set_mesh_lights_ms": first_ms, "set_mesh_lights_again_ms": stats(again_ms),
           "gsamples_per_s_off": stats(rates["off"]), "gsamples_per_s_on": stats(rates["on"]),
           "on_over_off_rate": stats(rates["on"])["median"] / stats(rates["off"])["median"]}
    for name, where in calls:
        pair = {"off": pkg.Tracer(make(), device=0, seed=1), "on": pkg.Tracer(make(), device=0, seed=1)}
        pair["on"].set_mesh_lights(torus_on)
        for tr in pair.values():
            getattr(tr, name)(back[where])                          # the context's first call of its kind: allocates
        ms = {"off": [], "on": []}
        for _ in range(reps):
            for arg in (there[where], back[where]):
                for side in ("off", "on"):
                    ms[side].append(timed(getattr(pair[side], name), arg))
        for tr in pair.values():
            tr.close()
        fo, fn = stats(ms["off"]), stats(ms["on"])
        out[name] = {"off_ms": fo, "on_ms": fn, "on_adds_ms": fn["median"] - fo["median"]}
    return out


def measure_textures(pkg, s, a):
    """-> the --textures line.  scenes.mesh_scene() untextured ("off") against both meshes under a 1024 x 1024 checker, BILINEAR /
    REPEAT, gamma 2.2, over spherical UVs ("on").  Two contexts for the frames and two per move call, so that every context's calls
    follow calls of its own kind; within a repetition the two sides alternate."""
    import numpy as np
    import torch
    from rust_pathtracer_amd import scenes

    original = [np.array(v, np.float32, copy=True) for v, _, _ in s.meshes]
    image = scenes.checker_texture(1024, 1024, (255, 255, 255), (60, 60, 60), cells=32)
    both = {m: dict(uvs=scenes.spherical_uvs(v, 0.5 * (v.min(0).astype(np.float64) + v.max(0))) * np.float32(4.0), texels=image,
                    wrap="repeat", filter="bilinear", gamma=2.2) for m, v in enumerate(original)}

    def stats(xs):
        xs = sorted(xs)
        return {"median": xs[len(xs) // 2], "min": xs[0], "max": xs[-1]}

    def timed(call, arg):
        t0 = time.perf_counter()
        call(arg)
        return (time.perf_counter() - t0) * 1e3

    def rate(tr):
        tr.render_resident(a.width, a.height, a.spp)
        return a.width * a.height * a.spp / (tr.resident_kernel_ms() * 1e-3) / 1e9

    reps = max(5, a.reps)
    # frames
    off, on = pkg.Tracer(scenes.mesh_scene(), device=0, seed=1), pkg.Tracer(scenes.mesh_scene(), device=0, seed=1)
    first_ms = timed(on.set_mesh_textures, both)                    # brings the refit tables, uploads and decodes 2 x 2^20 texels
    again_ms = [timed(on.set_mesh_textures, both) for _ in range(reps)]
    for tr in (off, on):
        rate(tr)                                                    # warm-up (and the dispatch order's first costs)
        rate(tr)
    rates = {"off": [], "on": []}
    for _ in range(reps):
        rates["off"].append(rate(off))
        rates["on"].append(rate(on))
    off.close()
    on.close()
    # moves: the medium move and back, so that every call moves every vertex
    moved = scenes.mesh_scene_moved(s, 0.5)
    dev = lambda arrays: {m: torch.from_numpy(np.ascontiguousarray(v, np.float32)).to("cuda:0") for m, v in enumerate(arrays)}   # noqa: E731
    there, back = {"host": dict(enumerate(moved)), "device": dev(moved)}, {"host": dict(enumerate(original)), "device": dev(original)}
    torch.cuda.synchronize()
    calls = (("update_meshes", "host"), ("rebuild_meshes", "host"), ("update_meshes_device", "device"), ("rebuild_meshes_device", "device"))
    out = {"workload": "mesh_scene mesh textures %dx%d x %d spp, resident" % (a.width, a.height, a.spp), "reps": reps,
           "texture": "2 x 1024x1024 RGBA8, bilinear, repeat",
           "first_set_mesh_textures_ms": first_ms, "set_mesh_textures_again_ms": stats(again_ms),
           "gsamples_per_s_off": stats(rates["off"]), "gsamples_per_s_on": stats(rates["on"]),
           "on_over_off_rate": stats(rates["on"])["median"] / stats(rates["off"])["median"]}
    for name, where in calls:
        pair = {"off": pkg.Tracer(scenes.mesh_scene(), device=0, seed=1), "on": pkg.Tracer(scenes.mesh_scene(), device=0, seed=1)}
        pair["on"].set_mesh_textures(both)
        for tr in pair.values():
            getattr(tr, name)(back[where])                          # the context's first call of its kind: allocates
        ms = {"off": [], "on": []}
        for _ in range(reps):
            for arg in (there[where], back[where]):
                for side in ("off", "on"):
                    ms[side].append(timed(getattr(pair[side], name), arg))
        for tr in pair.values():
            tr.close()
        fo, fn = stats(ms["off"]), stats(ms["on"])
        out[name] = {"off_ms": fo, "on_ms": fn, "on_adds_ms": fn["median"] - fo["median"]}
    return out


def measure_environment(pkg, a):
    """-> the --environment line.  scenes.mesh_scene() without an environment ("none"), under a 1024 x 1024 sky BACKGROUND_ONLY
    ("background") and SAMPLED ("sampled"): three contexts, alternating within a repetition, medians of `reps`; and the set call."""
    import numpy as np
    from rust_pathtracer_amd import scenes

    size = 1024
    d = scenes.octahedral_directions(size)
    image = np.where(d[..., 1:2] >= 0.0, np.array([0.25, 0.35, 0.5]), np.array([0.05, 0.05, 0.05]))
    sun = np.array([0.35, 0.8, 0.5]) / np.linalg.norm([0.35, 0.8, 0.5])
    image = np.ascontiguousarray(np.where((d @ sun)[..., None] > np.cos(0.02), np.array([2000.0, 1800.0, 1500.0]), image), dtype=np.float32)

    def stats(xs):
        xs = sorted(xs)
        return {"median": xs[len(xs) // 2], "min": xs[0], "max": xs[-1]}

    def timed(call, *args, **kw):
        t0 = time.perf_counter()
        call(*args, **kw)
        return (time.perf_counter() - t0) * 1e3

    def rate(tr):
        tr.render_resident(a.width, a.height, a.spp)
        return a.width * a.height * a.spp / (tr.resident_kernel_ms() * 1e-3) / 1e9

    reps = max(5, a.reps)
    sides = ("none", "background", "sampled")
    tr = {k: pkg.Tracer(scenes.mesh_scene(), device=0, seed=1) for k in sides}
    first = {k: timed(tr[k].set_environment, image, sampled=(k == "sampled")) for k in sides[1:]}      # brings the refit tables too
    again = {k: [timed(tr[k].set_environment, image, sampled=(k == "sampled")) for _ in range(reps)] for k in sides[1:]}
    for t in tr.values():
        rate(t)                                                     # warm-up (and the dispatch order's first costs)
        rate(t)
    rates = {k: [] for k in sides}
    for _ in range(reps):
        for k in sides:
            rates[k].append(rate(tr[k]))
    for t in tr.values():
        t.close()
    med = {k: stats(rates[k])["median"] for k in sides}
    return {"workload": "mesh_scene environment %dx%d x %d spp, resident" % (a.width, a.height, a.spp), "reps": reps,
            "environment": "%d x %d f32 RGB" % (size, size),
            "first_set_environment_ms": first, "set_environment_again_ms": {k: stats(v) for k, v in again.items()},
            "gsamples_per_s": {k: stats(rates[k]) for k in sides},
            "background_over_none_rate": med["background"] / med["none"], "sampled_over_none_rate": med["sampled"] / med["none"]}


def measure_cutouts(pkg, s, a):
    """-> the --cutouts line.  scenes.mesh_scene() textured as measure_textures does, with no mask ("textured"), under a 1024 x 1024
    checker mask of 32 x 32 fields on both meshes ("checker") and under an all-opaque mask of that size ("opaque"): three contexts,
    alternating within a repetition, medians of `reps`; the set call; and the four move calls on a "textured" and a "checker"
    context."""
    import numpy as np
    import torch
    from rust_pathtracer_amd import scenes

    original = [np.array(v, np.float32, copy=True) for v, _, _ in s.meshes]
    image = scenes.checker_texture(1024, 1024, (255, 255, 255), (60, 60, 60), cells=32)
    both = {m: dict(uvs=scenes.spherical_uvs(v, 0.5 * (v.min(0).astype(np.float64) + v.max(0))) * np.float32(4.0), texels=image,
                    wrap="repeat", filter="bilinear", gamma=2.2) for m, v in enumerate(original)}
    masks = {"checker": scenes.checker_mask(1024, 1024, cells=32), "opaque": np.full((1024, 1024), 255, np.uint8)}

    def stats(xs):
        xs = sorted(xs)
        return {"median": xs[len(xs) // 2], "min": xs[0], "max": xs[-1]}

    def timed(call, arg):
        t0 = time.perf_counter()
        call(arg)
        return (time.perf_counter() - t0) * 1e3

    def rate(tr):
        tr.render_resident(a.width, a.height, a.spp)
        return a.width * a.height * a.spp / (tr.resident_kernel_ms() * 1e-3) / 1e9

    def context(mask):
        tr = pkg.Tracer(scenes.mesh_scene(), device=0, seed=1)
        tr.set_mesh_textures(both)
        if mask is not None:
            tr.set_mesh_cutouts({m: masks[mask] for m in both})
        return tr

    reps = max(5, a.reps)
    sides = ("textured", "checker", "opaque")
    tr = {"textured": context(None)}
    first, again = {}, {}
    for k in sides[1:]:
        tr[k] = context(None)
        first[k] = timed(tr[k].set_mesh_cutouts, {m: masks[k] for m in both})      # 2 x 2^20 texels: one byte each up, one bit each kept
        again[k] = [timed(tr[k].set_mesh_cutouts, {m: masks[k] for m in both}) for _ in range(reps)]
    for t in tr.values():
        rate(t)                                                     # warm-up (and the dispatch order's first costs)
        rate(t)
    rates = {k: [] for k in sides}
    for _ in range(reps):
        for k in sides:
            rates[k].append(rate(tr[k]))
    for t in tr.values():
        t.close()
    med = {k: stats(rates[k])["median"] for k in sides}
    out = {"workload": "mesh_scene mesh cutouts %dx%d x %d spp, resident" % (a.width, a.height, a.spp), "reps": reps,
           "mask": "2 x 1024x1024 A8 over 2 x 1024x1024 RGBA8, bilinear, repeat",
           "first_set_mesh_cutouts_ms": first, "set_mesh_cutouts_again_ms": {k: stats(v) for k, v in again.items()},
           "gsamples_per_s": {k: stats(rates[k]) for k in sides},
           "checker_over_textured_rate": med["checker"] / med["textured"], "opaque_over_textured_rate": med["opaque"] / med["textured"]}
    # moves: the medium move and back, so that every call moves every vertex
    moved = scenes.mesh_scene_moved(s, 0.5)
    dev = lambda arrays: {m: torch.from_numpy(np.ascontiguousarray(v, np.float32)).to("cuda:0") for m, v in enumerate(arrays)}   # noqa: E731
    there, back = {"host": dict(enumerate(moved)), "device": dev(moved)}, {"host": dict(enumerate(original)), "device": dev(original)}
    torch.cuda.synchronize()
    calls = (("update_meshes", "host"), ("rebuild_meshes", "host"), ("update_meshes_device", "device"), ("rebuild_meshes_device", "device"))
    for name, where in calls:
        pair = {"off": context(None), "on": context("checker")}
        for t in pair.values():
            getattr(t, name)(back[where])                           # the context's first call of its kind: allocates
        ms = {"off": [], "on": []}
        for _ in range(reps):
            for arg in (there[where], back[where]):
                for side in ("off", "on"):
                    ms[side].append(timed(getattr(pair[side], name), arg))
        for t in pair.values():
            t.close()
        fo, fn = stats(ms["off"]), stats(ms["on"])
        out[name] = {"off_ms": fo, "on_ms": fn, "on_adds_ms": fn["median"] - fo["median"]}
    return out


def measure_normal_maps(pkg, s, a):
    """-> the --normal-maps line.  scenes.mesh_scene() textured as measure_textures does, with no map ("textured"), under a flat
    1024 x 1024 map on both meshes ("flat") and under a 1024 x 1024 BILINEAR bump map of 32 x 32 waves ("bump"): three contexts,
    alternating within a repetition, medians of `reps`; the set call; and the four move calls on a "textured" and a "bump"
    context."""
    import numpy as np
    import torch
    from rust_pathtracer_amd import scenes

    original = [np.array(v, np.float32, copy=True) for v, _, _ in s.meshes]
    image = scenes.checker_texture(1024, 1024, (255, 255, 255), (60, 60, 60), cells=32)
    both = {m: dict(uvs=scenes.spherical_uvs(v, 0.5 * (v.min(0).astype(np.float64) + v.max(0))) * np.float32(4.0), texels=image,
                    wrap="repeat", filter="bilinear", gamma=2.2) for m, v in enumerate(original)}
    maps = {"flat": scenes.height_to_normal_map(np.zeros((1024, 1024)), 1.0),
            "bump": scenes.height_to_normal_map(scenes.bump_height(1024, 1024, 32), 8.0)}

    def stats(xs):
        xs = sorted(xs)
        return {"median": xs[len(xs) // 2], "min": xs[0], "max": xs[-1]}

    def timed(call, arg):
        t0 = time.perf_counter()
        call(arg)
        return (time.perf_counter() - t0) * 1e3

    def rate(tr):
        tr.render_resident(a.width, a.height, a.spp)
        return a.width * a.height * a.spp / (tr.resident_kernel_ms() * 1e-3) / 1e9

    def context(which):
        tr = pkg.Tracer(scenes.mesh_scene(), device=0, seed=1)
        tr.set_mesh_textures(both)
        if which is not None:
            tr.set_mesh_normal_maps({m: dict(texels=maps[which], filter="bilinear") for m in both})
        return tr

    reps = max(5, a.reps)
    sides = ("textured", "flat", "bump")
    tr = {"textured": context(None)}
    first, again = {}, {}
    for k in sides[1:]:
        tr[k] = context(None)
        items = {m: dict(texels=maps[k], filter="bilinear") for m in both}
        first[k] = timed(tr[k].set_mesh_normal_maps, items)         # 2 x 2^20 texels: 4 B each up, 16 B each kept
        again[k] = [timed(tr[k].set_mesh_normal_maps, items) for _ in range(reps)]
    for t in tr.values():
        rate(t)                                                     # warm-up (and the dispatch order's first costs)
        rate(t)
    rates = {k: [] for k in sides}
    for _ in range(reps):
        for k in sides:
            rates[k].append(rate(tr[k]))
    for t in tr.values():
        t.close()
    med = {k: stats(rates[k])["median"] for k in sides}
    out = {"workload": "mesh_scene mesh normal maps %dx%d x %d spp, resident" % (a.width, a.height, a.spp), "reps": reps,
           "map": "2 x 1024x1024 RGBA8, bilinear, over 2 x 1024x1024 RGBA8, bilinear, repeat",
           "first_set_mesh_normal_maps_ms": first, "set_mesh_normal_maps_again_ms": {k: stats(v) for k, v in again.items()},
           "gsamples_per_s": {k: stats(rates[k]) for k in sides},
           "flat_over_textured_rate": med["flat"] / med["textured"], "bump_over_textured_rate": med["bump"] / med["textured"]}
    # moves: the medium move and back, so that every call moves every vertex
    moved = scenes.mesh_scene_moved(s, 0.5)
    dev = lambda arrays: {m: torch.from_numpy(np.ascontiguousarray(v, np.float32)).to("cuda:0") for m, v in enumerate(arrays)}   # noqa: E731
    there, back = {"host": dict(enumerate(moved)), "device": dev(moved)}, {"host": dict(enumerate(original)), "device": dev(original)}
    torch.cuda.synchronize()
    calls = (("update_meshes", "host"), ("rebuild_meshes", "host"), ("update_meshes_device", "device"), ("rebuild_meshes_device", "device"))
    for name, where in calls:
        pair = {"off": context(None), "on": context("bump")}
        for t in pair.values():
            getattr(t, name)(back[where])                           # the context's first call of its kind: allocates
        ms = {"off": [], "on": []}
        for _ in range(reps):
            for arg in (there[where], back[where]):
                for side in ("off", "on"):
                    ms[side].append(timed(getattr(pair[side], name), arg))
        for t in pair.values():
            t.close()
        fo, fn = stats(ms["off"]), stats(ms["on"])
        out[name] = {"off_ms": fo, "on_ms": fn, "on_adds_ms": fn["median"] - fo["median"]}
    return out


def measure_material_maps(pkg, s, a):
    """-> the --material-maps line.  scenes.mesh_scene() textured as measure_textures does, with no map ("textured"), under an
    all-255 1024 x 1024 map on both meshes ("ones") and under a 1024 x 1024 BILINEAR noise map, G roughness and B metallic
    ("noise"): three contexts, alternating within a repetition, medians of `reps`; the set call; and the four move calls on a
    "textured" and a "noise" context."""
    import numpy as np
    import torch
    from rust_pathtracer_amd import scenes

    original = [np.array(v, np.float32, copy=True) for v, _, _ in s.meshes]
    image = scenes.checker_texture(1024, 1024, (255, 255, 255), (60, 60, 60), cells=32)
    both = {m: dict(uvs=scenes.spherical_uvs(v, 0.5 * (v.min(0).astype(np.float64) + v.max(0))) * np.float32(4.0), texels=image,
                    wrap="repeat", filter="bilinear", gamma=2.2) for m, v in enumerate(original)}
    maps = {"ones": np.full((1024, 1024, 4), 255, np.uint8),
            "noise": np.random.default_rng(0x5EED0007).integers(0, 256, (1024, 1024, 4), dtype=np.uint8)}

    def stats(xs):
        xs = sorted(xs)
        return {"median": xs[len(xs) // 2], "min": xs[0], "max": xs[-1]}

    def timed(call, arg):
        t0 = time.perf_counter()
        call(arg)
        return (time.perf_counter() - t0) * 1e3

    def rate(tr):
        tr.render_resident(a.width, a.height, a.spp)
        return a.width * a.height * a.spp / (tr.resident_kernel_ms() * 1e-3) / 1e9

    def context(which):
        tr = pkg.Tracer(scenes.mesh_scene(), device=0, seed=1)
        tr.set_mesh_textures(both)
        if which is not None:
            tr.set_mesh_material_maps({m: dict(texels=maps[which], filter="bilinear") for m in both})
        return tr

    reps = max(5, a.reps)
    sides = ("textured", "ones", "noise")
    tr = {"textured": context(None)}
    first, again = {}, {}
    for k in sides[1:]:
        tr[k] = context(None)
        items = {m: dict(texels=maps[k], filter="bilinear") for m in both}
        first[k] = timed(tr[k].set_mesh_material_maps, items)       # 2 x 2^20 texels: 4 B each up, 16 B each kept
        again[k] = [timed(tr[k].set_mesh_material_maps, items) for _ in range(reps)]
    for t in tr.values():
        rate(t)                                                     # warm-up (and the dispatch order's first costs)
        rate(t)
    rates = {k: [] for k in sides}
    for _ in range(reps):
        for k in sides:
            rates[k].append(rate(tr[k]))
    for t in tr.values():
        t.close()
    med = {k: stats(rates[k])["median"] for k in sides}
    out = {"workload": "mesh_scene mesh material maps %dx%d x %d spp, resident" % (a.width, a.height, a.spp), "reps": reps,
           "map": "2 x 1024x1024 RGBA8, bilinear, over 2 x 1024x1024 RGBA8, bilinear, repeat",
           "first_set_mesh_material_maps_ms": first, "set_mesh_material_maps_again_ms": {k: stats(v) for k, v in again.items()},
           "gsamples_per_s": {k: stats(rates[k]) for k in sides},
           "ones_over_textured_rate": med["ones"] / med["textured"], "noise_over_textured_rate": med["noise"] / med["textured"]}
    # moves: the medium move and back, so that every call moves every vertex
    moved = scenes.mesh_scene_moved(s, 0.5)
    dev = lambda arrays: {m: torch.from_numpy(np.ascontiguousarray(v, np.float32)).to("cuda:0") for m, v in enumerate(arrays)}   # noqa: E731
    there, back = {"host": dict(enumerate(moved)), "device": dev(moved)}, {"host": dict(enumerate(original)), "device": dev(original)}
    torch.cuda.synchronize()
    calls = (("update_meshes", "host"), ("rebuild_meshes", "host"), ("update_meshes_device", "device"), ("rebuild_meshes_device", "device"))
    for name, where in calls:
        pair = {"off": context(None), "on": context("noise")}
        for t in pair.values():
            getattr(t, name)(back[where])                           # the context's first call of its kind: allocates
        ms = {"off": [], "on": []}
        for _ in range(reps):
            for arg in (there[where], back[where]):
                for side in ("off", "on"):
                    ms[side].append(timed(getattr(pair[side], name), arg))
        for t in pair.values():
            t.close()
        fo, fn = stats(ms["off"]), stats(ms["on"])
        out[name] = {"off_ms": fo, "on_ms": fn, "on_adds_ms": fn["median"] - fo["median"]}
    return out


def measure_emission_maps(pkg, s, a):
    """-> the --emission-maps line.  scenes.mesh_scene() textured as measure_textures does, with the shadow rays' flag and its torus
    emissive and ON as measure_lights has it: with no map ("lit"), under an all-255 1024 x 1024 map on the torus ("ones") and under a
    1024 x 1024 BILINEAR noise map ("noise"): three contexts, alternating within a repetition, medians of `reps`; the set call; and
    the four move calls on a "lit" and a "noise" context."""
    import numpy as np
    import torch
    from rust_pathtracer_amd import scenes

    def make():
        sc = scenes.mesh_scene()
        sc.any_hit_uses_max_dist = True
        sc.materials[1].fields["emission"] = (4.0, 3.0, 2.0)
        return sc

    original = [np.array(v, np.float32, copy=True) for v, _, _ in s.meshes]
    image = scenes.checker_texture(1024, 1024, (255, 255, 255), (60, 60, 60), cells=32)
    both = {m: dict(uvs=scenes.spherical_uvs(v, 0.5 * (v.min(0).astype(np.float64) + v.max(0))) * np.float32(4.0), texels=image,
                    wrap="repeat", filter="bilinear", gamma=2.2) for m, v in enumerate(original)}
    maps = {"ones": np.full((1024, 1024, 4), 255, np.uint8),
            "noise": np.random.default_rng(0x5EED0008).integers(0, 256, (1024, 1024, 4), dtype=np.uint8)}

    def stats(xs):
        xs = sorted(xs)
        return {"median": xs[len(xs) // 2], "min": xs[0], "max": xs[-1]}

    def timed(call, arg):
        t0 = time.perf_counter()
        call(arg)
        return (time.perf_counter() - t0) * 1e3

    def rate(tr):
        tr.render_resident(a.width, a.height, a.spp)
        return a.width * a.height * a.spp / (tr.resident_kernel_ms() * 1e-3) / 1e9

    def context(which):
        tr = pkg.Tracer(make(), device=0, seed=1)
        tr.set_mesh_textures(both)
        tr.set_mesh_lights({1: True})
        if which is not None:
            tr.set_mesh_emission_maps({1: dict(texels=maps[which], filter="bilinear", gamma=2.2)})
        return tr

    reps = max(5, a.reps)
    sides = ("lit", "ones", "noise")
    tr = {"lit": context(None)}
    first, again = {}, {}
    for k in sides[1:]:
        tr[k] = context(None)
        items = {1: dict(texels=maps[k], filter="bilinear", gamma=2.2)}
        first[k] = timed(tr[k].set_mesh_emission_maps, items)       # 2^20 texels: 4 B each up, 16 B each kept
        again[k] = [timed(tr[k].set_mesh_emission_maps, items) for _ in range(reps)]
    for t in tr.values():
        rate(t)                                                     # warm-up (and the dispatch order's first costs)
        rate(t)
    rates = {k: [] for k in sides}
    for _ in range(reps):
        for k in sides:
            rates[k].append(rate(tr[k]))
    for t in tr.values():
        t.close()
    med = {k: stats(rates[k])["median"] for k in sides}
    out = {"workload": "mesh_scene mesh emission maps %dx%d x %d spp, resident" % (a.width, a.height, a.spp), "reps": reps,
           "map": "1024x1024 RGBA8, bilinear, gamma 2.2, on the ON torus, over 2 x 1024x1024 RGBA8, bilinear, repeat",
           "first_set_mesh_emission_maps_ms": first, "set_mesh_emission_maps_again_ms": {k: stats(v) for k, v in again.items()},
           "gsamples_per_s": {k: stats(rates[k]) for k in sides},
           "ones_over_lit_rate": med["ones"] / med["lit"], "noise_over_lit_rate": med["noise"] / med["lit"]}
    # moves: the medium move and back, so that every call moves every vertex
    moved = scenes.mesh_scene_moved(s, 0.5)
    dev = lambda arrays: {m: torch.from_numpy(np.ascontiguousarray(v, np.float32)).to("cuda:0") for m, v in enumerate(arrays)}   # noqa: E731
    there, back = {"host": dict(enumerate(moved)), "device": dev(moved)}, {"host": dict(enumerate(original)), "device": dev(original)}
    torch.cuda.synchronize()
    calls = (("update_meshes", "host"), ("rebuild_meshes", "host"), ("update_meshes_device", "device"), ("rebuild_meshes_device", "device"))
    for name, where in calls:
        pair = {"off": context(None), "on": context("noise")}
        for t in pair.values():
            getattr(t, name)(back[where])                           # the context's first call of its kind: allocates
        ms = {"off": [], "on": []}
        for _ in range(reps):
            for arg in (there[where], back[where]):
                for side in ("off", "on"):
                    ms[side].append(timed(getattr(pair[side], name), arg))
        for t in pair.values():
            t.close()
        fo, fn = stats(ms["off"]), stats(ms["on"])
        out[name] = {"off_ms": fo, "on_ms": fn, "on_adds_ms": fn["median"] - fo["median"]}
    return out


def measure_media(pkg, s, a):
    """-> the --media line.  scenes.mesh_scene() with its icosphere (mesh 0) made glass and the shadow rays' flag: with no medium
    ("none": the form the scene always ran), with an ABSORB medium on the glass mesh ("absorb") and with a SCATTER medium on it
    ("scatter"): three contexts, alternating within a repetition, medians of `reps`; the set call; and the four move calls on a
    "none" and a "scatter" context."""
    import numpy as np
    import torch
    from rust_pathtracer_amd import scenes

    def make():
        sc = scenes.mesh_scene()
        sc.any_hit_uses_max_dist = True
        sc.materials[sc.meshes[0][2]] = scenes.full_material(rgb=(0.95, 0.95, 0.95), roughness=0.05, spec_trans=1.0, ior=1.45)
        return sc

    original = [np.array(v, np.float32, copy=True) for v, _, _ in s.meshes]
    media = {"absorb": dict(type="absorb", density=3.0, color=(0.9, 0.45, 0.3)),
             "scatter": dict(type="scatter", density=2.5, color=(0.85, 0.9, 0.95), anisotropy=0.6)}

    def stats(xs):
        xs = sorted(xs)
        return {"median": xs[len(xs) // 2], "min": xs[0], "max": xs[-1]}

    def timed(call, arg):
        t0 = time.perf_counter()
        call(arg)
        return (time.perf_counter() - t0) * 1e3

    def rate(tr):
        tr.render_resident(a.width, a.height, a.spp)
        return a.width * a.height * a.spp / (tr.resident_kernel_ms() * 1e-3) / 1e9

    def form(tr):
        f = C.c_uint32(0)
        pkg._lib.check(pkg.lib().rpt_debug_mesh_form(tr._h, C.byref(f)), tr._h)
        return f.value

    def context(which):
        tr = pkg.Tracer(make(), device=0, seed=1)
        if which is not None:
            tr.set_mesh_media({0: media[which]})
        return tr

    reps = max(5, a.reps)
    sides = ("none", "absorb", "scatter")
    tr = {"none": context(None)}
    first, again = {}, {}
    for k in sides[1:]:
        tr[k] = context(None)
        first[k] = timed(tr[k].set_mesh_media, {0: media[k]})       # 32 B per medium, 4 B per triangle of the scene, the empty tables
        again[k] = [timed(tr[k].set_mesh_media, {0: media[k]}) for _ in range(reps)]
    for t in tr.values():
        rate(t)                                                     # warm-up (and the dispatch order's first costs)
        rate(t)
    forms = {k: form(tr[k]) for k in sides}
    assert forms["none"] < 28 <= forms["absorb"] == forms["scatter"], forms
    rates = {k: [] for k in sides}
    for _ in range(reps):
        for k in sides:
            rates[k].append(rate(tr[k]))
    for t in tr.values():
        t.close()
    med = {k: stats(rates[k])["median"] for k in sides}
    out = {"workload": "mesh_scene mesh media %dx%d x %d spp, resident" % (a.width, a.height, a.spp), "reps": reps,
           "media": "on the glass icosphere: ABSORB density 3 colour (0.9, 0.45, 0.3); SCATTER density 2.5 colour (0.85, 0.9, 0.95) g 0.6",
           "mesh_form": forms,
           "first_set_mesh_media_ms": first, "set_mesh_media_again_ms": {k: stats(v) for k, v in again.items()},
           "gsamples_per_s": {k: stats(rates[k]) for k in sides},
           "absorb_over_none_rate": med["absorb"] / med["none"], "scatter_over_none_rate": med["scatter"] / med["none"]}
    # moves: the medium move and back, so that every call moves every vertex
    moved = scenes.mesh_scene_moved(s, 0.5)
    dev = lambda arrays: {m: torch.from_numpy(np.ascontiguousarray(v, np.float32)).to("cuda:0") for m, v in enumerate(arrays)}   # noqa: E731
    there, back = {"host": dict(enumerate(moved)), "device": dev(moved)}, {"host": dict(enumerate(original)), "device": dev(original)}
    torch.cuda.synchronize()
    calls = (("update_meshes", "host"), ("rebuild_meshes", "host"), ("update_meshes_device", "device"), ("rebuild_meshes_device", "device"))
    for name, where in calls:
        pair = {"off": context(None), "on": context("scatter")}
        for t in pair.values():
            getattr(t, name)(back[where])                           # the context's first call of its kind: allocates
        ms = {"off": [], "on": []}
        for _ in range(reps):
            for arg in (there[where], back[where]):
                for side in ("off", "on"):
                    ms[side].append(timed(getattr(pair[side], name), arg))
        for t in pair.values():
            t.close()
        fo, fn = stats(ms["off"]), stats(ms["on"])
        out[name] = {"off_ms": fo, "on_ms": fn, "on_adds_ms": fn["median"] - fo["median"]}
    return out


def measure_rays(pkg, s, a):
    """-> the --rays line.  One context on scenes.mesh_scene() as uploaded (no feature ON: the closest, occluded and surface kernels
    without the cut test and the normal map).  Two ray sets of width * height rays each: the camera's ("coherent") and random ones
    through the scene's box ("incoherent").  A sample is `launches` launches in a row between two device events on torch's current
    stream; medians of `reps`.  The 1-spp resident frame alternates with the closest hit of the camera's rays."""
    import numpy as np
    import torch

    def stats(xs):
        xs = sorted(xs)
        return {"median": xs[len(xs) // 2], "min": xs[0], "max": xs[-1]}

    reps, launches = max(5, a.reps), 20
    n = a.width * a.height
    tr = pkg.Tracer(s, device=0, seed=1)
    dev = torch.device("cuda", 0)
    sets = {"coherent": tr.camera_rays(a.width, a.height)}
    verts = np.concatenate([np.asarray(v, np.float64).reshape(-1, 3) for v, _, _ in s.meshes])
    lo, hi = verts.min(0), verts.max(0)
    lo, hi = lo - 0.25 * (hi - lo), hi + 0.25 * (hi - lo)
    rng = np.random.default_rng(0x5EED0007)
    d = rng.normal(size=(n, 3))
    r = np.zeros((n, 8), np.float32)
    r[:, 0:3] = lo + rng.uniform(size=(n, 3)) * (hi - lo)
    r[:, 3] = np.inf
    r[:, 4:7] = d / np.linalg.norm(d, axis=1, keepdims=True)
    sets["incoherent"] = torch.from_numpy(r).to(dev)
    hits = torch.empty((n, 8), dtype=torch.float32, device=dev)
    surf = torch.empty((n, 16), dtype=torch.float32, device=dev)
    occ = torch.empty((n,), dtype=torch.uint8, device=dev)
    lib, h = pkg.lib(), tr._h
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    calls = {
        "closest": lambda rays: lib.rpt_trace_rays_device(h, rays.data_ptr(), n, hits.data_ptr(), None, 0, stream),
        "closest_with_surfaces": lambda rays: lib.rpt_trace_rays_device(h, rays.data_ptr(), n, hits.data_ptr(), surf.data_ptr(), 0, stream),
        "occluded": lambda rays: lib.rpt_occluded_device(h, rays.data_ptr(), n, occ.data_ptr(), 0, stream),
    }

    def rays_per_s(call, rays):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(launches):
            pkg._lib.check(call(rays), h)
        e1.record()
        e1.synchronize()
        return n * launches / (e0.elapsed_time(e1) * 1e-3)

    def frame_samples_per_s():
        tr.render_resident(a.width, a.height, 1)
        return n / (tr.resident_kernel_ms() * 1e-3)

    for call in calls.values():                                     # warm-up: every kernel, both sets (and the query's own allocation)
        for rays in sets.values():
            rays_per_s(call, rays)
    for _ in range(3):
        frame_samples_per_s()                                       # (and the dispatch order's first costs)
    rates = {k: {name: [] for name in calls} for k in sets}
    frame, beside = [], []
    for _ in range(reps):
        for k, rays in sets.items():
            for name, call in calls.items():
                rates[k][name].append(rays_per_s(call, rays))
        frame.append(frame_samples_per_s())                         # alternating: the 1-spp frame, then the closest hit of its rays
        beside.append(rays_per_s(calls["closest"], sets["coherent"]))
    cam_ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(launches):
            pkg._lib.check(lib.rpt_camera_rays_device(h, a.width, a.height, sets["coherent"].data_ptr(), stream), h)
        e1.record()
        e1.synchronize()
        cam_ms.append(e0.elapsed_time(e1) / launches)
    out = tr.trace(sets["coherent"])
    torch.cuda.synchronize()
    kinds = torch.bincount(out["kind"].to(torch.int64), minlength=4).cpu().numpy() / float(n)
    tr.close()
    f, b = stats(frame), stats(beside)
    return {"workload": "mesh_scene ray queries, %d rays per launch (%dx%d), %d launches per sample" % (n, a.width, a.height, launches), "reps": reps,
            "grays_per_s": {k: {name: {kk: vv / 1e9 for kk, vv in stats(v).items()} for name, v in rates[k].items()} for k in sets},
            "frame_1spp_gsamples_per_s": {kk: vv / 1e9 for kk, vv in f.items()}, "frame_1spp_ms": n / f["median"] * 1e3,
            "closest_coherent_beside_the_frame_grays_per_s": {kk: vv / 1e9 for kk, vv in b.items()},
            "closest_rays_over_frame_samples": b["median"] / f["median"],
            "camera_rays_ms": stats(cam_ms),
            "camera_rays_hit": {"none": kinds[0], "sphere": kinds[1], "plane": kinds[2], "triangle": kinds[3]}}


def measure_radiance(pkg, a):
    """-> the --radiance line.  Two contexts, one per scene; on each the radiance query over the camera's sample rays alternates with
    the resident render of the same frame, then the probe batch runs."""
    import numpy as np
    import torch
    from rust_pathtracer_amd import scenes

    def stats(xs):
        xs = sorted(xs)
        return {"median": xs[len(xs) // 2], "min": xs[0], "max": xs[-1]}

    def form(tr):
        f = C.c_uint32(0)
        pkg._lib.check(pkg.lib().rpt_debug_mesh_form(tr._h, C.byref(f)), tr._h)
        return f.value

    reps, probes = max(5, a.reps), 2_000_000
    n = a.width * a.height
    dev = torch.device("cuda", 0)
    media_scene, media = scenes.mesh_media_scene()
    out = {"workload": "radiance queries, %dx%d x %d spp over the camera's sample rays; %d probe rays x %d spp" % (a.width, a.height, a.spp, probes, a.spp),
           "reps": reps}
    for name, scene, setup in (("flat", scenes.mesh_scene(), None), ("media", media_scene, media)):
        tr = pkg.Tracer(scene, device=0, seed=1)
        if setup:
            tr.set_mesh_media(setup)
        rays = tr.camera_sample_rays(a.width, a.height, 0)
        acc = torch.zeros((n, 4), dtype=torch.float32, device=dev)

        def query_rate(r, buf):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            buf.zero_()
            e0.record()
            tr.radiance(r, spp=a.spp, out=buf)
            e1.record()
            e1.synchronize()
            return r.shape[0] * a.spp / (e0.elapsed_time(e1) * 1e-3) / 1e6

        def render_rate():
            tr.resident_reset()
            tr.render_resident(a.width, a.height, a.spp)
            return n * a.spp / (tr.resident_kernel_ms() * 1e-3) / 1e6

        for _ in range(2):                                          # warm-up (the query's own allocation; the dispatch order's first costs)
            query_rate(rays, acc)
            render_rate()
        q, f = [], []
        for _ in range(reps):
            q.append(query_rate(rays, acc))
            f.append(render_rate())
        verts = np.concatenate([np.asarray(v, np.float64).reshape(-1, 3) for v, _, _ in scene.meshes])
        lo, hi = verts.min(0), verts.max(0)
        lo, hi = lo - 0.25 * (hi - lo), hi + 0.25 * (hi - lo)
        rng = np.random.default_rng(0x5EED0009)
        d = rng.normal(size=(probes, 3))
        r = np.zeros((probes, 8), np.float32)
        r[:, 0:3] = lo + rng.uniform(size=(probes, 3)) * (hi - lo)
        r[:, 3] = np.inf
        r[:, 4:7] = d / np.linalg.norm(d, axis=1, keepdims=True)
        probe_rays = torch.from_numpy(r).to(dev)
        probe_acc = torch.zeros((probes, 4), dtype=torch.float32, device=dev)
        query_rate(probe_rays, probe_acc)
        p = [query_rate(probe_rays, probe_acc) for _ in range(reps)]
        qs, fs = stats(q), stats(f)
        out[name] = {"render_form": form(tr), "radiance_msamples_per_s": qs, "render_msamples_per_s": fs,
                     "radiance_over_render": qs["median"] / fs["median"], "probe_msamples_per_s": stats(p)}
        tr.close()
    return out


if __name__ == "__main__":
    main()
