"""Times temporal accumulation (include/rpt.h, "temporal accumulation") in its three forms — first frame, IDENTITY, reprojecting under
a one-pixel pan — next to the guided denoiser at its defaults on the same frame, in one process: 1080p and 4K, the four calls
alternating inside one timed loop.  Prints one line per measurement and one JSON line at the end.  Needs a GPU: there is no fallback.

    python tools/temporal_bench.py [--reps 20] [--warmup 5]

Rates are ALGORITHMIC bytes over device-event time, and that rate over the HBM peak (8.0 TB/s, the specification's):
  first frame    64 B per pixel (16 B of colour read; 16 B of colour and 32 B of history written)
  IDENTITY      176 B per pixel (the same, 48 B of the pixel's guide, and 32 B of previous guide + 32 B of previous history)
  reprojecting  176 B per pixel (four taps per pixel, but every previous record is needed once: what neighbouring pixels share is the
                caches' business)
  guided filter 80 B per pixel and iteration + 32 B per pixel and call (tools/denoise_guided_bench.py)
The guides are analytic (tests/tacc_fuzz.py: a ground plane in three key regions, a sphere, the sky), the history what the first-frame
form leaves for the previous camera."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import conftest  # noqa: E402
import tacc_fuzz  # noqa: E402
import torch  # noqa: E402

HBM_PEAK_GBS = 8000.0
BYTES = {"first frame": 64.0, "identity": 176.0, "reproject": 176.0}


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("temporal_bench: needs a GPU (nothing is measured on a CPU)")
    rpt = conftest.load_package()
    dev = torch.device("cuda", 0)
    results = []

    def report(name, w, h, ms, nbytes):
        best, med = min(ms), sorted(ms)[len(ms) // 2]
        gbs = nbytes / best / 1e6
        results.append(dict(name=name, width=w, height=h, best_ms=round(best, 4), median_ms=round(med, 4), algorithmic_bytes=int(nbytes),
                            algorithmic_GBs=round(gbs, 1), frac_of_hbm_peak=round(gbs / HBM_PEAK_GBS, 4)))
        print("%-14s %4dx%-4d: best %8.4f ms  median %8.4f ms  -> %7.1f GB/s algorithmic = %5.1f %% of the HBM peak" % (
            name, w, h, best, med, gbs, 100.0 * gbs / HBM_PEAK_GBS), flush=True)

    pin = lambda c: rpt.Pinhole(tuple(float(v) for v in c[0:3]), tuple(float(v) for v in c[3:6]), float(c[6]))      # noqa: E731
    for w, h in ((1920, 1080), (3840, 2160)):
        n = w * h
        cam = tacc_fuzz.CAM_A
        prev_cam = tacc_fuzz.pan(cam, w, h, 1.0)
        guides = torch.from_numpy(tacc_fuzz.analytic_guides(cam, w, h)).to(dev)
        prev_guides = torch.from_numpy(tacc_fuzz.analytic_guides(prev_cam, w, h)).to(dev)
        buf, out, filtered = rpt.DeviceColorBuffer(w, h), rpt.DeviceColorBuffer(w, h), rpt.DeviceColorBuffer(w, h)
        torch.manual_seed(1)
        buf.pixels.uniform_(0.0, 2.0)
        # one accumulator per form, each brought to the state its timed call starts from; accumulate() swaps the two history tensors,
        # so every call reads what the call before it wrote: the same traffic every time
        first, ident, repro = (rpt.TemporalAccumulator(w, h, device=dev) for _ in range(3))
        ident.accumulate(buf, guides, pin(cam), out=out)
        repro.accumulate(buf, prev_guides, pin(prev_cam), out=out)

        def run_first():
            first.reset()
            first.accumulate(buf, guides, pin(cam), out=out)

        def run_ident():
            ident.accumulate(buf, guides, pin(cam), out=out)

        def run_repro():                                               # the camera goes back and forth by one pixel
            repro.accumulate(buf, *((guides, pin(cam)) if repro._prev_guides is prev_guides else (prev_guides, pin(prev_cam))), out=out)

        def run_filter():
            buf.denoise_guided(guides, out=filtered)

        calls = (("first frame", run_first), ("identity", run_ident), ("reproject", run_repro), ("guided filter", run_filter))
        for _ in range(args.warmup):
            for _, fn in calls:
                fn()
        torch.cuda.synchronize()
        ms = {name: [] for name, _ in calls}
        for _ in range(args.reps):                                     # alternating: all see the same neighbours on a shared machine
            for name, fn in calls:
                ms[name].append(timed(fn))
        share = float((repro.samples() > 1).float().mean())
        for name, _ in calls:
            report(name, w, h, ms[name], (BYTES[name] if name in BYTES else 80.0 * 4 + 32.0) * n)
        print("               %4dx%-4d: %.1f %% of the pixels found history under the one-pixel pan" % (w, h, 100.0 * share), flush=True)
    print(json.dumps(dict(tool="temporal_bench", device=torch.cuda.get_device_name(0), hbm_peak_GBs=HBM_PEAK_GBS, results=results)))


if __name__ == "__main__":
    main()
