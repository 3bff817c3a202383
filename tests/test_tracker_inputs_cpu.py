"""Preconditions of tests/test_trackers_gpu.py, on the CPU: the oracle alone, on its own spectrogram of each input rounded
through float32 (the stand-in for the device's).  They assert that the inputs do what the GPU tests rely on -- the band
sequences reach the paths of k_track_cog the tests are there for, no band edge sits on a rounding cliff, and no oracle
tracker raises on a sweep seed.  pytest -s prints the band statistics and the smallest cliff margin."""
import warnings

import numpy as np
import pytest

import tracker_inputs as T
from oracle import oracle_np as O


@pytest.fixture(scope="module")
def mags():
    cache = {}

    def get(c):
        if c.name not in cache:
            cache[c.name] = T.oracle_mag(c)
        return cache[c.name]
    return get


@pytest.mark.parametrize("name", T.NAMED + T.TRAIL_SHAPES)
def test_band_sequence_reaches_the_paths(mags, name):
    c = T.case(name)
    spec = mags(c)
    stats, raw = T.assert_paths(name, spec, c)
    print(f"\n{name}: {stats}, NaN frames before patching {np.isnan(raw).nonzero()[0].tolist()}")
    # the replay is the oracle's own walk: patched like track_cog patches, it is track_cog's result
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        times, freqs = O.track_cog(spec, c.trail, c.n_fft, c.hop, c.sr, c.tol)
    O._interp_nans(raw)
    assert len(times) == stats["frames"] and np.array_equal(raw, freqs)
    assert np.isfinite(freqs).all()


def test_bin0_oracle_behaviour(mags):
    """What the GPU test of `bin0` expects of the oracle: Peak, Peak Track and Center of Gravity return (no exception,
    the NaN frames patched); Correlation's band starts on bin 0, log2(0) poisons every frame and patching an all-NaN
    line raises ValueError."""
    c = T.case("bin0")
    spec = mags(c)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for name in ("Peak", "Peak Track", "Center of Gravity"):
            times, freqs = O.TRACKERS[name](spec, c.trail, c.n_fft, c.hop, c.sr, c.tol)
            assert len(freqs) == len(times) > 100 and np.isfinite(freqs).all(), name
        with pytest.raises(ValueError):
            O.TRACKERS["Correlation"](spec, c.trail, c.n_fft, c.hop, c.sr, c.tol)


def test_trail_shapes_frame_counts(mags):
    for name, frames in (("clipped_end", 94), ("one_frame", 1)):
        c = T.case(name)
        for k in T.TRACKERS:
            times, freqs = O.TRACKERS[k](mags(c), c.trail, c.n_fft, c.hop, c.sr, c.tol)
            assert len(times) == len(freqs) == frames, (name, k, len(freqs))


def test_no_band_edge_on_a_rounding_cliff(mags):
    """Every argument the oracle rounds to a band edge lies at least CLIFF_MARGIN bins from a half-integer, in the named
    cases and in every sweep seed.  A libm that differs by an ulp moves such an argument by about 1e-13 bins, so with this
    holding a band that differs on the GPU is a kernel error.  A sweep seed that fails here is replaced in
    tracker_inputs.SWEEP_SEEDS; the margin stays."""
    margins = {}
    for name in T.NAMED + T.TRAIL_SHAPES:
        c = T.case(name)
        margins[name] = T.cliff_margin(mags(c), c)
    for seed in T.SWEEP_SEEDS:
        c = T.sweep_case(seed)
        margins[c.name] = T.cliff_margin(mags(c), c)
    for cfg in T.REFINED:                                   # the refined runs round Peak's and Peak Track's edges only
        c = T.refined_case(*cfg)
        margins[c.name] = T.cliff_margin(T.float64_mag(c), c)
    worst = min(margins, key=margins.get)
    print(f"\nsmallest cliff margin: {margins[worst]:.2e} bins ({worst}); named cases "
          f"{min(margins[k] for k in T.NAMED):.2e}")
    bad = {k: v for k, v in margins.items() if not v >= T.CLIFF_MARGIN}
    assert not bad, bad


@pytest.mark.filterwarnings("ignore::RuntimeWarning")      # a sweep band may reach bin 0 too: log2(0), patched
def test_sweep_seeds_all_compare(mags):
    """No oracle tracker raises on a sweep seed and every one traces at least a few frames, so the GPU sweep skips
    nothing: 32 seeds x 4 trackers compare.  The generator must also reach what it is there for."""
    assert len(set(T.SWEEP_SEEDS)) == 32
    hops_off_grid = starts_at_0 = ends_past_file = 0
    for seed in T.SWEEP_SEEDS:
        c = T.sweep_case(seed)
        spec = mags(c)
        for k in T.TRACKERS:
            times, freqs = O.TRACKERS[k](spec, c.trail, c.n_fft, c.hop, c.sr, c.tol)
            assert len(times) == len(freqs) >= 4 and np.isfinite(freqs).all(), (seed, k)
        ts = sorted(t for t, _ in c.trail)
        hops_off_grid += c.n_fft % c.hop != 0
        starts_at_0 += ts[0] == 0.0
        ends_past_file += ts[-1] > len(c.x) / c.sr
    assert hops_off_grid >= 3 and starts_at_0 >= 3 and ends_past_file >= 3, (hops_off_grid, starts_at_0, ends_past_file)
