"""A sample's own float32 error bound, from the float64 restatement run again with f32-sized noise in its arithmetic
(pt_f64.perturbed: relative noise uniform in +-2^-24 on the result of every helper in pt_f64.PERTURBED and on the outputs the mesh
and media restatements compute outside them).  Test infrastructure; no GPU needed.

One bound for every sample cannot be both safe and sharp: a path that grazes or bounces often amplifies rounding by orders of
magnitude, most paths do not.  How far a sample moves under the noise is that sample's sensitivity:

  spread      the largest rel_distance of RUNS noisy runs of the restatement from the plain one, per sample
  tolerance   min(REL_CLEAN, Z_MAX * max(spread, FLOOR)): test_path_f64's 5e-2 stays as a cap, so nothing that fails without
              spreads passes with them
  z           rel_distance(plain restatement, f32 result) / max(spread, FLOOR)

FLOOR = 2^-22: a sample with zero spread (a miss returns the background exactly) still carries the rounding of the f32 output and of
the blend's multiply, 2 x 2^-24; the floor doubles that.

Z_MAX, Z_MEDIAN and the bias statement are calibrated in tests/test_path_f64.py on the f32 oracle (the analytical device kernels'
bit-identical twin) against the restatement, never on the device.  Statements holds a set of samples to them:

  each clean sample     rel_distance <= its tolerance
  median                the median z over the clean samples with a non-zero spread <= Z_MEDIAN
  bias                  the signed mean relative difference over the clean samples is within BIAS_SIGMAS of its own standard
                        errors + BIAS_FLOOR, as f64_compare.Bounds states it for frames
Only samples that have a spread (not NaN) take part; the others are held to REL_CLEAN by the caller as before.

Files that pass spreads to Tally.add: test_gpu_path_f64 (the small scenes), test_gpu_mesh_compose_f64, test_gpu_mesh_material_map_f64,
test_gpu_mesh_emission_map_f64, test_gpu_mesh_media_f64, test_gpu_radiance_f64, and the single-feature files test_gpu_mesh_f64,
test_gpu_mesh_smooth_f64, test_gpu_mesh_light_f64, test_gpu_mesh_texture_f64, test_gpu_mesh_env_f64, test_gpu_mesh_cutout_f64,
test_gpu_mesh_normal_map_f64 (through Cases below) and test_gpu_mesh_frames_f64 (through test_mesh_frames_f64's noisy_samples, at
64 x 48).  Each holds its CPU-side conditions and plants a subtle fault (teeth) without a GPU; the cutout file has no teeth of its
own and says why."""
import time

import numpy as np

import pt_f64 as P
import test_path_f64 as T

FLOOR = 2.0 ** -22
RUNS = 8
BIAS_SIGMAS, BIAS_FLOOR = 4.0, 1e-6
SHARP = 1e-3                                                          # the tolerance most clean samples must stay below (a condition)


def _radiance(result):
    r = result[0] if isinstance(result, tuple) else result
    return np.nan_to_num(np.asarray(r, np.float64), nan=0.0, posinf=0.0, neginf=0.0)      # blended as black


def spread(restate, runs=RUNS, seed=0, plain=None):
    """restate() -> radiance [n, 3] (or a tuple that starts with it).  -> the per-sample spread [n]: the largest rel_distance of
    `runs` noisy runs from the plain one (`plain`: the plain run's radiance, if the caller has it)."""
    base = _radiance(restate() if plain is None else plain)
    out = np.zeros(len(base))
    for run in range(runs):
        with P.perturbed(seed, run):
            noisy = _radiance(restate())
        out = np.maximum(out, T.rel_distance(base, noisy))
    return out


def timed_spread(restate, **kw):
    """-> (spread, the CPU seconds it took)."""
    t0 = time.process_time()
    s = spread(restate, **kw)
    return s, time.process_time() - t0


def tolerance(spreads, z_max=None):
    z_max = T.Z_MAX if z_max is None else z_max
    return np.minimum(T.REL_CLEAN, z_max * np.maximum(spreads, FLOOR))


def z_of(rel, spreads):
    return rel / np.maximum(spreads, FLOOR)


def signed_difference(got, dev):
    """The signed relative difference of a sample: the mean over channels of (dev - got) / max(|got|, 1e-3)."""
    got, dev = _radiance(got), _radiance(dev)
    return ((dev - got) / np.maximum(np.abs(got), 1e-3)).mean(axis=1)


def subset_spreads(n, indices, values):
    """Spreads for `indices` of n samples, NaN (no spread) elsewhere."""
    out = np.full(n, np.nan)
    out[np.asarray(indices, np.int64)] = values
    return out


def first_clean(margins, count, tau=None):
    """The indices of the first `count` clean samples (all of them if there are fewer)."""
    tau = T.TAU if tau is None else tau
    return np.nonzero(np.asarray(margins) > tau)[0][:count]


class Statements:
    """Clean samples that have a spread, collected over add() calls, and what they are held to."""

    def __init__(self, z_max=None, z_median=None):
        self.z_max_bound = T.Z_MAX if z_max is None else z_max
        self.z_median_bound = T.Z_MEDIAN if z_median is None else z_median
        self.rel, self.sgn, self.spr = [np.zeros(0)], [np.zeros(0)], [np.zeros(0)]

    def add(self, got, dev, clean, spreads):
        """got: the plain restatement [n, 3]; dev: the f32 result; clean: margin > tau; spreads [n], NaN where there is none.
        -> the indices of the clean samples beyond their tolerance."""
        got, dev = _radiance(got), _radiance(dev)
        spreads = np.asarray(spreads, np.float64)
        has = np.asarray(clean, bool) & ~np.isnan(spreads)
        rel = T.rel_distance(got, dev)
        self.rel.append(rel[has])
        self.sgn.append(signed_difference(got, dev)[has])
        self.spr.append(spreads[has])
        tol = tolerance(np.where(has, spreads, 0.0), self.z_max_bound)
        return np.nonzero(has & (rel > tol))[0]

    def figures(self):
        rel, sgn, spr = (np.concatenate(x) for x in (self.rel, self.sgn, self.spr))
        z = z_of(rel, spr)
        nz = spr > 0.0
        n = len(rel)
        return dict(n=n, z_max=float(z.max()) if n else 0.0, z_median=float(np.median(z[nz])) if nz.any() else 0.0,
                    n_nonzero=int(nz.sum()), bias=float(sgn.mean()) if n else 0.0,
                    bias_se=float(sgn.std(ddof=1) / np.sqrt(n)) if n > 1 else 0.0,
                    beyond=int((rel > tolerance(spr, self.z_max_bound)).sum()),
                    above_sharp=float((tolerance(spr, self.z_max_bound) > SHARP).mean()) if n else 0.0)

    def failures(self, bias=True):
        """The set-wide statements broken (empty: none).  bias=False leaves the bias statement out."""
        f = self.figures()
        out = []
        if not f["z_median"] <= self.z_median_bound:
            out.append("median z %.3g > %.3g" % (f["z_median"], self.z_median_bound))
        if bias and not abs(f["bias"]) <= BIAS_SIGMAS * f["bias_se"] + BIAS_FLOOR:
            out.append("bias %.3g beyond %g standard errors (%.3g) + %g" % (f["bias"], BIAS_SIGMAS, f["bias_se"], BIAS_FLOOR))
        return out

    def line(self):
        f = self.figures()
        return "%d clean samples with a spread, largest z %.3g, median z %.3g, bias %.3g (se %.3g), %.2f %% with a tolerance above %g" % (
            f["n"], f["z_max"], f["z_median"], f["bias"], f["bias_se"], 100.0 * f["above_sharp"], SHARP)


# ---- the mesh files' draws: [(seed, pixels, radiance, margins)] per case -------------------------------------------------------------
MIN_CLEAN = 150                                                       # spreads for at least the first 150 clean samples of a case
MIN_WITH_SPREAD = 100                                                 # a condition on every case
SHARP_SHARE_CASE = 0.05                                               # at most 5 % of a case's clean samples with a tolerance above SHARP


def spreads_of_draws(path, oracle, entries, w, h, count=MIN_CLEAN):
    """The spreads of the first `count` clean samples (None: of every clean sample) of a case whose draws `entries` = [(seed, pixels, radiance, margins)] were
    restated through `path` by mesh_compose_f64.sample_pixels -> ([spreads per entry, NaN where there is none], CPU seconds)."""
    from mesh_compose_f64 import sample_pixels
    out, seconds, left = [], 0.0, count
    for seed, pixels, radiance, margins in entries:
        idx = first_clean(margins, len(margins) if count is None else left)
        left = None if count is None else left - len(idx)
        values = np.zeros(0)
        if len(idx):
            sub = [pixels[i] for i in idx]
            values, dt = timed_spread(lambda: sample_pixels(path, oracle, seed, sub, w, h), plain=radiance[idx])
            seconds += dt
        s = subset_spreads(len(pixels), idx, values)
        s.setflags(write=False)
        out.append(s)
    return out, seconds


class Cases:
    """A file's cases, each restated and given its spreads once for the CPU and the GPU leg.  path_of(case) -> the restatement as a
    path for mesh_compose_f64.sample_pixels (pt_f64.Path(scene) for the files that restate through pt_f64.sample_many: the same
    sample from the same stream); draws_of(case) -> [(seed, pixels)], the file's own draws.  Nobody writes to what comes back."""

    def __init__(self, path_of, draws_of, w=64, h=48):
        self.path_of, self.draws_of, self.w, self.h = path_of, draws_of, w, h
        self._path, self._restated, self._spreads = {}, {}, {}

    def path(self, case):
        if case not in self._path:
            self._path[case] = self.path_of(case)
        return self._path[case]

    def restated(self, oracle, case):
        """[(seed, pixels, radiance, margins)] over the case's draws."""
        from mesh_compose_f64 import sample_pixels
        if case not in self._restated:
            entries = [(seed, pixels) + sample_pixels(self.path(case), oracle, seed, pixels, self.w, self.h) for seed, pixels in self.draws_of(case)]
            for _, _, radiance, margins in entries:
                radiance.setflags(write=False)
                margins.setflags(write=False)
            self._restated[case] = entries
        return self._restated[case]

    def spreads(self, oracle, case):
        """([spreads per entry, NaN where there is none], CPU seconds): of the case's first MIN_CLEAN clean samples."""
        if case not in self._spreads:
            self._spreads[case] = spreads_of_draws(self.path(case), oracle, self.restated(oracle, case), self.w, self.h)
        return self._spreads[case]

    def conditions(self, oracle, what, case):
        spreads, seconds = self.spreads(oracle, case)
        case_conditions(what, self.restated(oracle, case), spreads, seconds)


def case_conditions(what, entries, spreads, seconds=None):
    """The CPU-side conditions of a case: at least MIN_WITH_SPREAD clean samples have a spread, and at most SHARP_SHARE_CASE of them
    a tolerance above SHARP.  Prints the figures."""
    spr = np.concatenate([s[(np.asarray(m) > T.TAU) & ~np.isnan(s)] for (_, _, _, m), s in zip(entries, spreads)])
    above = float((tolerance(spr) > SHARP).mean())
    print("%s: %d clean samples with a spread (median %.3g, 99th percentile %.3g, largest %.3g), %.2f %% with a tolerance above %g%s" % (
        what, len(spr), np.median(spr), np.percentile(spr, 99), spr.max(), 100.0 * above, SHARP,
        "" if seconds is None else "; the spreads took %.2f s of CPU time" % seconds))
    assert len(spr) >= MIN_WITH_SPREAD, "%s: %d clean samples with a spread" % (what, len(spr))
    assert above <= SHARP_SHARE_CASE, "%s: %.2f %% of the clean samples have a tolerance above %g" % (what, 100.0 * above, SHARP)


def teeth_on(what, good, faulty, oracle, draws, w, h):
    """teeth() for a restatement `good` and a subtly faulty one, both paths for mesh_compose_f64.sample_pixels, over `draws` =
    [(seed, pixels)] with a spread for every clean sample: for faults planted on inputs other than a case's own."""
    from mesh_compose_f64 import sample_pixels
    entries = [(seed, pixels) + sample_pixels(good, oracle, seed, pixels, w, h) for seed, pixels in draws]
    spreads, _ = spreads_of_draws(good, oracle, entries, w, h, count=None)
    return teeth(what, entries, spreads, [sample_pixels(faulty, oracle, seed, pixels, w, h) for seed, pixels in draws])


def teeth(what, entries, spreads, faulty):
    """A subtly faulty restatement's samples, rounded to f32, stand in for a device: `faulty` = [(radiance, margins)] for the draws
    of `entries`.  Asserts that the comparison without spreads passes it (no clean sample beyond REL_CLEAN) and that the statements
    with spreads do not (at least 10 clean samples beyond their own tolerance); prints and returns the counts."""
    st = Statements()
    far = beyond = moved = 0
    for (_, _, radiance, margins), s, (rad2, marg2) in zip(entries, spreads, faulty):
        dev = _radiance(rad2).astype(np.float32).astype(np.float64)
        clean = (np.asarray(margins) > T.TAU) & (np.asarray(marg2) > T.TAU)
        rel = T.rel_distance(_radiance(radiance), dev)
        far += int((clean & (rel > T.REL_CLEAN)).sum())
        moved += int((clean & (rel > FLOOR)).sum())
        beyond += len(st.add(radiance, dev, clean, s))
    print("%s: %d clean samples beyond REL_CLEAN, %d beyond their own tolerance (%d moved at all); %s" % (what, far, beyond, moved, st.line()))
    assert far == 0, "%s: the fault is not subtle: %d clean samples beyond REL_CLEAN" % (what, far)
    assert beyond >= 10, "%s: only %d clean samples beyond their own tolerance" % (what, beyond)
    return far, beyond
