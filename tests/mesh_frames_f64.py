"""A launch of several samples restated in float64: what csrc/regen_body.h's body does with a pixel between reading it and writing
it back, over any restatement of ONE pixel-sample (mesh_compose_f64.sample_pixels and its subclasses' paths, or pt_f64.sample_many).

A launch receives frames_done (api.py: buffer.frames) and spp = n.  Its sample s, s = 0 .. n - 1, is frame f = frames_done + s:
  * its random stream is keyed by (seed, f, pixel)                      (kernel_common.h, lane_setup_ex: frame_key(seed, frames_done + s))
  * it enters the pixel's running mean with v = 1 / (f + 1): acc = (1 - v) * acc + c * v, c = (r, g, b, 1), in sample order
                                                                         (kernel_common.h, blend; tracer.rs:105-117)
  * a sample that is not finite is blended as black                     (kernel_common.h, blend: PROJECT-DEFINED)
The accumulator starts from what the buffer held — zero for a fresh one.  Which lane of a wave renders a sample, and when, is no part
of the statement: "which lane renders a sample never changes it ... what must not change is the ORDER" (kernel_common.h, above
share_init), so the restatement is the sequential loop and nothing else.  Everything is float64; the device's v is the f32
1 / (float)(f + 1), 6e-8 away, and its blend rounds to f32 at every step.

A pixel's margin is the smallest of its samples' margins: the mean is as far from a branch flip as its nearest sample.

Three planted faults, each by a keyword argument, each in one place:
  frame_ignored             every sample draws frame 0's stream (the running mean of a fresh buffer is then sample 0)
  key_without_frames_done   sample s of a launch draws stream s, not frames_done + s (invisible from frames_done = 0)
  weight_off_by_one         v = 1 / f, and 1 at f = 0 (invisible in a one-sample launch at a frame so late that 1 / f and 1 / (f + 1)
                            are REL_CLEAN apart or less: the comparison scales the device's pixel by f + 1)
tests/test_mesh_frames_f64.py (CPU) counts what each moves; tests/test_gpu_mesh_frames_f64.py holds the device to frame_f64.
A fourth, for the ends of the launch domain (tests/test_launch_domain.py): frame_low_word_only keys sample s by
(frames_done + s) & 0xFFFFFFFF, a frame counter truncated to 32 bits (invisible below 2^32).
A fifth, subtle one: weight_late_from = F takes v = 1 / (f + 2) from frame F on (a running mean one frame off at high counts, a
part in a thousand at f = 1000), which only the samples' own f32 tolerances see (tests/f32_spread.py).

Under pt_f64's noise mode the blend carries what the device rounds in f32: the weight 1 / (f + 1), each of the two products and the
sum.  With the mode off every value keeps its bits.

Measured on the CPU: 1.5 ms per sample of the emission-mapped restatement (cases A .. H), 1.2 ms per sample of the flat one."""
import numpy as np

import pt_f64 as P
from mesh_compose_f64 import sample_pixels


def frame_f64(path, oracle, seed, pixels, w, h, frames_done, n, acc=None, sample_frame=None,
              frame_ignored=False, key_without_frames_done=False, weight_off_by_one=False, weight_late_from=None, frame_low_word_only=False):
    """A launch of `n` samples on top of `frames_done` earlier frames, for `pixels` [(col, row)] ->
    (mean [p, 4], margins [p], samples [p, n, 3]).

    acc: the pixels' accumulator before the launch, [p, 4]; zero (a fresh buffer) by default.  sample_frame(f) -> (radiance [p, 3],
    margins [p]): the restatement of the pixels' sample of frame f; by default sample_pixels(path, ..., frame=f).  A caller hands
    its own to share samples between comparisons, or to restate through pt_f64.sample_many."""
    if sample_frame is None:
        sample_frame = lambda f: sample_pixels(path, oracle, seed, pixels, w, h, frame=f)      # noqa: E731
    mean = np.zeros((len(pixels), 4)) if acc is None else np.array(acc, dtype=np.float64).reshape(len(pixels), 4)
    margins = np.full(len(pixels), np.inf)
    samples = np.zeros((len(pixels), n, 3))
    for s in range(n):
        frame = frames_done + s
        stream = 0 if frame_ignored else s if key_without_frames_done else frame & 0xFFFFFFFF if frame_low_word_only else frame
        rad, marg = sample_frame(stream)
        samples[:, s] = rad
        margins = np.minimum(margins, marg)
        if weight_off_by_one:
            v = 1.0 / frame if frame else 1.0
        elif weight_late_from is not None and frame >= weight_late_from:
            v = 1.0 / (frame + 2)
        else:
            v = P.noisy(1.0 / (frame + 1))
        c = np.concatenate([np.where(np.isfinite(rad).all(axis=1, keepdims=True), rad, 0.0), np.ones((len(pixels), 1))], axis=1)
        mean = P.noisy_array(P.noisy_array((1.0 - v) * mean) + P.noisy_array(c * v))
    return mean, margins, samples
