"""Scene upload on the GPU (include/rpt.h, rpt_upload_scene; csrc/capi.hip stages a scene's tables on every device, then commits):
one context cycles through every scene class — small, large (grid), mesh, small with the mapped material table, the SDF object,
media — and back, on one device and on a context with the device listed twice.  After each upload the frame and the kernel choice
are those of a fresh context on that scene, bit for bit; a rejected upload of each class answers its code and leaves the frame as
it was.  Needs an MI355X."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H, SPP, SEED = 64, 48, 2, 5


def _scenes(rpt):
    from rust_pathtracer_amd import scenes
    return [("analytical", rpt.AnalyticalScene()),
            ("large", scenes.random_spheres_scene(200, 4)),
            ("mesh", scenes.mesh_scene(subdivisions=2, n_major=16, n_minor=8)),
            ("six_primitives", scenes.six_primitive_scene()),
            ("sdf", scenes.sdf_scene()),
            ("media", scenes.media_scene()),
            ("analytical again", rpt.AnalyticalScene())]


def _rejected(rpt):
    """One descriptor of each class that the class's own checks reject: (name, scene kept alive, descriptor, code)."""
    from rust_pathtracer_amd import scenes
    A = rpt._abi
    small = scenes.sdf_scene()
    d_small = small.describe()
    d_small.sdf.smooth_k = 0.0
    large = scenes.random_spheres_scene(200, 4)
    d_large = large.describe()
    d_large.spheres[7].material = d_large.n_materials - 1                # the checker floor's patch: large scenes need whole materials
    mesh = scenes.mesh_scene(subdivisions=2, n_major=16, n_minor=8)
    d_mesh = mesh.describe()
    d_mesh.meshes[1].material = 2                                        # ... and so do meshes
    return [("small", small, d_small, A.RPT_ERR_INVALID_ARG), ("large", large, d_large, A.RPT_ERR_UNSUPPORTED),
            ("mesh", mesh, d_mesh, A.RPT_ERR_UNSUPPORTED)]


def _tracer(rpt, scene, multi):
    return rpt.Tracer(scene, devices=[0, 0], seed=SEED) if multi else rpt.Tracer(scene, device=0, seed=SEED)


def _frame(rpt, t):
    """A host ColorBuffer's frame (rpt_render: every device of the context renders its rows) and the kernel choice bits."""
    buf = rpt.ColorBuffer(W, H)
    t.render_n(buf, SPP)
    choice = C.c_uint32(0)
    assert rpt.lib().rpt_debug_kernel_choice(t._h, C.byref(choice)) == 0
    return buf.pixels.copy(), choice.value


def _same(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("multi", [False, True], ids=["one-device", "device-listed-twice"])
def test_one_context_cycles_through_every_scene_class(rpt, multi):
    cycle = _scenes(rpt)
    rejected = _rejected(rpt)
    t = _tracer(rpt, cycle[0][1], multi)
    try:
        for name, scene in cycle:
            d = scene.describe()
            rpt._lib.check(rpt.lib().rpt_upload_scene(t._h, C.byref(d)), t._h)
            got, choice = _frame(rpt, t)
            fresh = _tracer(rpt, scene, multi)
            want, want_choice = _frame(rpt, fresh)
            fresh.close()
            assert _same(got, want), "%s: the frame differs from a fresh context's" % name
            assert choice == want_choice, "%s: kernel choice %#x, a fresh context takes %#x" % (name, choice, want_choice)
            assert np.isfinite(got).all() and got[..., :3].mean() > 0.01, name
            for bad, _keep, bad_d, code in rejected:
                assert rpt.lib().rpt_upload_scene(t._h, C.byref(bad_d)) == code, "%s, then a bad %s scene" % (name, bad)
                after, after_choice = _frame(rpt, t)
                assert _same(after, got) and after_choice == choice, "%s: a rejected %s upload changed the frame" % (name, bad)
    finally:
        t.close()
