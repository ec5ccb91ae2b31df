"""The mesh scene (rust_pathtracer_amd.scenes.mesh_scene: ~3.9e5 triangles) at 1920x1080 on one GPU: prints ONE JSON line with
Gsamples/s of the resident render, the triangle and BVH node counts, the BVH's depth and build time (host, inside the upload) and the
whole upload's time.  Loads the test build (its rpt_debug_mesh_stats, include/rpt_test.h).

    python tools/mesh_bench.py [--spp 16] [--reps 5]
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
    t.close()
    print(json.dumps({"workload": "mesh_scene %dx%d x %d spp, resident" % (a.width, a.height, a.spp), "triangles": n_tris,
                      "gsamples_per_s_median": sorted(rates)[len(rates) // 2], "gsamples_per_s": rates,
                      "bvh_nodes": nodes.value, "bvh_depth": depth.value, "bvh_build_ms": build_ms.value, "upload_s": upload_s}))


if __name__ == "__main__":
    main()
