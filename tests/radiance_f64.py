"""Radiance queries restated in float64 (include/rpt.h, "radiance queries"): one sample of the integrator's estimate along a ray the
caller brings, through the float64 restatements the render forms are held to — mesh_media_f64.MediaMeshPath for the media cases
(with no medium it reduces to the composed path's own operations), mesh_emap_f64.EmapPath where material and emission maps are ON,
pt_f64.Path on the flat scene.  No bounce loop is copied here: a path's own sample() runs, as it is, with its first segment replaced.

The section's rules, each where this file applies it:

  * the path starts from the caller's origin and direction exactly as given (first_segment): for the length of one call pt_f64.gen_ray
    — what every restatement's sample() makes its camera ray with — is swapped for a function that returns (o, d), behind a context
    manager that puts it back
  * the stream's first two draws are made and discarded: sample() draws them for the camera's jitter and hands them to gen_ray, which
    here ignores them
  * the stream of ray i is (seed, frames_done, first_index + i), the index in uint32 arithmetic (sample_rays)
  * everything else starts as a camera path does — the restatements' own initial state, in_medium false wherever the origin lies

Faults a device could have are planted by `fault`, each a single line; tests/test_radiance_f64.py holds each to rays that must see it:
  draws_not_discarded       the path's own draws start at the stream's first draw
  key_without_first_index   ray i runs on the stream of index i
  starts_inside_medium      a path whose origin lies inside a mesh that bounds a medium starts with in_medium true"""
import contextlib

import numpy as np

import media_sdf_f64 as MS
import pt_f64 as P
from mesh_compose_f64 import N_DRAWS
from test_gpu_mesh_f64 import MeshDescScene

FAULTS = ("draws_not_discarded", "key_without_first_index", "starts_inside_medium")
_PathState = MS.PathState                                             # (the class itself, whatever first_segment swaps in)
PROBE_DIR = P.normalize((0.2672612419124244, 0.5345224838248488, 0.8017837257372732))


@contextlib.contextmanager
def first_segment(o, d, state=None):
    """Within the block every restatement's sample() starts its path at (o, d); `state`: a replacement for media_sdf_f64.PathState
    (the planted fault's)."""
    saved_ray, saved_state = P.gen_ray, MS.PathState
    P.gen_ray = lambda cam, p, offset, width, height: (o, d)
    if state is not None:
        MS.PathState = state
    try:
        yield
    finally:
        P.gen_ray, MS.PathState = saved_ray, saved_state


def medium_around(sc, o):
    """The medium of the mesh `o` lies inside of, or None: crossings of each medium-carrying mesh's triangles along a fixed direction,
    counted without the cut test (a mask has holes, a boundary does not); an odd count is inside."""
    for m, medium in sorted(getattr(sc, "mesh_medium", {}).items()):
        hit, _ = MeshDescScene._triangles(sc, o, PROBE_DIR, P.Margin())
        if int((hit & (sc.tri_mesh == m)).sum()) % 2 == 1:
            return medium
    return None


def sample(path, o, d, draws, fault=None):
    """One sample along (o, d) on the stream `draws` -> (radiance, rays, margin), as the path's own sample() returns them."""
    state = None
    if fault == "starts_inside_medium":
        inside = medium_around(path.scene, o)
        if inside is not None:
            def state():
                ps = _PathState()
                ps.in_medium, ps.medium = True, inside              # (the fault)
                return ps
    if fault == "draws_not_discarded":
        draws = np.concatenate([draws[:2], draws])                    # (the two draws sample() spends come before the stream)
    with first_segment(o, d, state):
        return path.sample(0, 0, 1, 1, draws)



def sample_rays(path, oracle, seed, frames_done, rays, first_index=0, fault=None, n_draws=N_DRAWS):
    """One sample of each of `rays` [n, 8] f32 (rpt_ray rows: origin, max_dist, direction, reserved), of frame `frames_done` ->
    (radiance [n, 3], margins [n]).  The oracle only supplies the random draws (rng_f32)."""
    out, marg = np.zeros((len(rays), 3)), np.zeros(len(rays))
    for i, r in enumerate(np.asarray(rays, np.float32)):
        index = (int(first_index) + i) & 0xFFFFFFFF
        if fault == "key_without_first_index":
            index = i
        dr = oracle.rng_f32(seed, int(frames_done), index, n_draws)
        P.noise_begin(seed, int(frames_done), index)
        o, d = tuple(float(x) for x in r[0:3]), tuple(float(x) for x in r[4:7])
        out[i], _, marg[i] = sample(path, o, d, dr, fault)
    return out, marg


def probe_rays(scene, n, seed):
    """`n` rpt_rays [n, 8] f32 no camera sends: origins uniform in the box of the scene's mesh vertices grown by half its size on
    every side, directions uniform on the sphere, normalised in float32; max_dist +inf, reserved 0."""
    rng = np.random.default_rng(seed)
    verts = np.concatenate([np.asarray(v, np.float64).reshape(-1, 3) for v, _, _ in scene.meshes])
    lo, hi = verts.min(0), verts.max(0)
    lo, hi = lo - 0.5 * (hi - lo), hi + 0.5 * (hi - lo)
    r = np.zeros((n, 8), np.float32)
    r[:, 0:3] = (lo + rng.uniform(size=(n, 3)) * (hi - lo)).astype(np.float32)
    d = rng.normal(size=(n, 3)).astype(np.float32)
    r[:, 4:7] = d / np.sqrt((d * d).sum(axis=1, dtype=np.float32))[:, None]
    r[:, 3] = np.inf
    return r


__all__ = ["FAULTS", "first_segment", "medium_around", "sample", "sample_rays", "probe_rays"]
