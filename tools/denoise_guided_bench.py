"""Times the guided denoiser (include/rpt.h, "guided denoiser") next to the colour-only one on the same frame, and the pack, in one
process: 1080p and 4K, 3 and 5 iterations, the two filters alternating inside one timed loop.  Prints one line per measurement and
one JSON line at the end.  Needs a GPU: there is no fallback.

    python tools/denoise_guided_bench.py [--reps 30] [--warmup 5]        (RPT_LIB selects a variant: tools/build_variants.py gdn_unfused)

Rates are ALGORITHMIC bytes over device-event time, and that rate over the HBM peak (8.0 TB/s, the specification's):
  colour-only   32 B per pixel and iteration (16 read, 16 written)
  guided        80 B per pixel and iteration (16 B of colour and the guide's position, ns and ng lines read, 16 B written) + 32 B per
                pixel and call (the albedo line at compression and at expansion)
  pack          192 B per record (ray 32, hit 32, surface 64 read; guide 64 written)
What the kernels really move (halos re-fetched by neighbouring tiles, taps served by L2) is a counter's business, not this tool's."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import conftest  # noqa: E402
import numpy as np  # noqa: E402
import torch  # noqa: E402

HBM_PEAK_GBS = 8000.0


def plain_bytes(n, it):
    return 32.0 * n * it


def guided_bytes(n, it):
    return (80.0 * it + 32.0) * n


def pack_bytes(n):
    return 192.0 * n


def synthetic_guides(w, h, device):
    """A floor and a wall split by a horizon, two keys, a checker albedo: guides that keep every term of the weight busy."""
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    g = np.zeros((h, w, 16), np.float32)
    floor = yy > 0.45 * h
    t = np.where(floor, 0.5 * h / np.maximum(yy - 0.45 * h + 1.0, 1.0), 6.0).astype(np.float32)
    g[..., 0], g[..., 1], g[..., 2] = (xx / w - 0.5) * t, np.where(floor, -0.5, (0.5 - yy / h) * t), -t
    g.view(np.uint32)[..., 3] = np.where(floor, (2 << 28) | 0, (2 << 28) | 1)
    g[..., 4:7] = np.where(floor[..., None], (0.0, 1.0, 0.0), (0.0, 0.0, 1.0))
    g[..., 7] = t
    g[..., 8:11] = g[..., 4:7]
    g.view(np.uint32)[..., 11] = 2
    g[..., 12:15] = (0.15 + 0.7 * ((xx // 8 + yy // 8) % 2))[..., None]
    return torch.from_numpy(g.reshape(-1, 16)).to(device)


def timed(fn, reps):
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("denoise_guided_bench: needs a GPU (nothing is measured on a CPU)")
    rpt = conftest.load_package()
    dev = torch.device("cuda", 0)
    results = []

    def report(name, w, h, it, ms, nbytes):
        best, med = min(ms), sorted(ms)[len(ms) // 2]
        gbs = nbytes / best / 1e6
        rec = dict(name=name, width=w, height=h, iterations=it, best_ms=round(best, 4), median_ms=round(med, 4), algorithmic_bytes=int(nbytes),
                   algorithmic_GBs=round(gbs, 1), frac_of_hbm_peak=round(gbs / HBM_PEAK_GBS, 4))
        results.append(rec)
        print("%-12s %4dx%-4d x%d: best %8.4f ms  median %8.4f ms  -> %7.1f GB/s algorithmic = %5.1f %% of the HBM peak" % (
            name, w, h, it, best, med, gbs, 100.0 * gbs / HBM_PEAK_GBS), flush=True)

    for w, h in ((1920, 1080), (3840, 2160)):
        n = w * h
        buf = rpt.DeviceColorBuffer(w, h)
        torch.manual_seed(1)
        buf.pixels.uniform_(0.0, 2.0)
        guides = synthetic_guides(w, h, dev)
        out_p, out_g = rpt.DeviceColorBuffer(w, h), rpt.DeviceColorBuffer(w, h)
        for it in (3, 5):
            for _ in range(args.warmup):
                buf.denoise(it, 2.0, out=out_p)
                buf.denoise_guided(guides, it, out=out_g)
            torch.cuda.synchronize()
            ms_p, ms_g = [], []
            for _ in range(args.reps):                                 # alternating: both see the same neighbours on a shared machine
                ms_p += timed(lambda: buf.denoise(it, 2.0, out=out_p), 1)
                ms_g += timed(lambda: buf.denoise_guided(guides, it, out=out_g), 1)
            report("colour-only", w, h, it, ms_p, plain_bytes(n, it))
            report("guided", w, h, it, ms_g, guided_bytes(n, it))
        rays = torch.zeros((n, 8), dtype=torch.float32, device=dev)
        rays[:, 4:7] = torch.tensor([0.0, 0.0, -1.0], device=dev)
        hits = torch.zeros((n, 8), dtype=torch.float32, device=dev)
        hits[:, 0] = 3.0
        hits.view(torch.int32)[:, 1] = 3                               # every record a triangle hit: the full 192 B
        surf = torch.rand((n, 16), dtype=torch.float32, device=dev)
        for _ in range(args.warmup):
            rpt.pack_guides(rays, hits, surf)
        torch.cuda.synchronize()
        report("pack", w, h, 0, timed(lambda: rpt.pack_guides(rays, hits, surf), args.reps), pack_bytes(n))
    print(json.dumps(dict(tool="denoise_guided_bench", device=torch.cuda.get_device_name(0), lib=os.path.basename(os.environ.get("RPT_LIB", "")),
                          hbm_peak_GBs=HBM_PEAK_GBS, results=results)))


if __name__ == "__main__":
    main()
