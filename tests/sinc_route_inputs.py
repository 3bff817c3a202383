"""Seeded inputs at the sizes where K_sinc's routing rule (csrc/sinc_route.h) changes its answer: a file goes to the streaming
kernel from 4096 outputs AND 4096 input samples on (four 1024-output tiles; at exactly four only tile 1 is streamed).  No device
code is imported here: tests/test_sinc_route_inputs_cpu.py proves with the C oracle that every curve gives the number of
outputs written beside it, tests/test_sinc_routes_gpu.py runs the kernels on them.

The reference cuts a segment of `period` input samples into round(period * mean speed) outputs (util/resampling.py:93-137), so a
curve over [0, T] gives T + a few outputs; T is chosen per curve so that the count lands where it should."""
from collections import namedtuple

import numpy as np

EDGE = 4096                       # kSincStreamMin of csrc/sinc_route.h, for len_out and for len_in
KNOTS = 40

Curve = namedtuple("Curve", "T k base n_in len_out")

# name -> (span of the curve in input samples, phase, mean speed, input samples, outputs the oracle gives)
CURVES = {
    "edge": Curve(4103, 0, 1.0, 4303, 4096),              # exactly four tiles
    "below": Curve(4102, 0, 1.0, 4302, 4095),             # one output short of them, the input long enough
    "short_in": Curve(4000, 0, 1.05, 4095, 4194),         # enough outputs from one input sample too few
    "edge_in": Curve(3910, 0, 1.05, 4096, 4099),          # ... and from exactly enough
    # further files of a batch: other curves, lengths around and above the edge, odd ends
    "f1": Curve(4092, 1, 1.0, 4300, 4096),
    "f2": Curve(4098, 2, 1.0, 4400, 4096),
    "f3": Curve(5000, 1, 1.0, 5200, 5005),
    "f4": Curve(6203, 2, 1.0, 6400, 6200),
    "f5": Curve(4777, 3, 1.0, 5000, 4777),
    "f6": Curve(8190, 4, 1.0, 8400, 8194),
    "f7": Curve(4500, 5, 1.0, 4700, 4495),
    "f8": Curve(5121, 6, 1.0, 5300, 5129),
}
MONO_NINE = ("edge", "f1", "f2", "f3", "f4", "f5", "f6", "f7", "f8")


def speed_curve(name):
    """(sampletimes, speeds) of CURVES[name]: one radian of a sine of amplitude 0.008 around its zero crossing, rising or
    falling, so that a unit-speed file has an fc = 1 and an fc < 1 stretch.  The speed changes by at most 0.008 / 3900 = 2.1e-6
    per output: inside the 2.7e-6 up to which the plan describes a block of outputs by its quadratic alone (seg_fast_record,
    csrc/pos.hip), which is what the streaming kernel places from -- steeper blocks it hands to the tile list."""
    c = CURVES[name]
    st = np.linspace(0.0, float(c.T), KNOTS)
    theta = np.linspace(-0.5, 0.5, KNOTS) + 0.07 * (c.k - 3)
    sp = c.base + (0.008 if c.k % 2 == 0 else -0.008) * np.sin(theta)
    return st, sp


def signal(name, channels=1, seed=0):
    """float32 noise of CURVES[name].n_in frames, (n_in,) or (n_in, channels) with different material per channel"""
    rng = np.random.default_rng([81, sorted(CURVES).index(name), channels, seed])
    n = CURVES[name].n_in
    x = rng.standard_normal(n if channels == 1 else (n, channels)).astype(np.float32)
    return x
