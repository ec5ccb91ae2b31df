"""Mesh media on a context of several devices (include/rpt.h, "mesh media"): rpt_set_mesh_media writes every device of a
rpt_create_multi context.  One test, modelled on the other mesh features' "device listed twice" tests: the device listed twice renders
the one-context frame, and removing the medium there returns the form of before."""
import numpy as np
import pytest

from kernel_census import MESH_RENDER_KERNELS
from test_gpu_mesh_compose_f64 import inputs
from test_gpu_mesh_material_map_f64 import mesh_form, set_composed
from test_gpu_mesh_media import FOG, form_of
from test_gpu_mesh_update import _same

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch


def test_a_device_listed_twice_renders_the_one_context_frame(rpt, torch_cuda):
    from rust_pathtracer_amd import scenes
    w, h, spp = 32, 24, 4
    frames = []
    for devices in (dict(device=0), dict(devices=[0, 0])):
        s = scenes.mesh_media_scene(None)[0]
        t = rpt.Tracer(s, seed=11, **devices)
        try:
            set_composed(t, inputs(s, "F"))
            t.set_mesh_media({0: FOG})
            t.render_resident(w, h, spp)
            assert mesh_form(rpt, t) == form_of("F") == 33
            frames.append(t.resident_to_host(w, h).pixels.reshape(h, w, 4).copy())
            if "devices" in devices:
                t.set_mesh_media({0: None})
                t.resident_reset()
                t.render_resident(w, h, spp)
                assert mesh_form(rpt, t) == MESH_RENDER_KERNELS.index("meshnrm_env_regen_kernel")
        finally:
            t.close()
    assert _same(frames[0], frames[1]) and np.isfinite(frames[0]).all()
