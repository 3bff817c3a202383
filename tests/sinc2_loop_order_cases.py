"""Inputs and oracle outputs shared by test_sinc2_loop_orders_cpu.py and test_sinc2_loop_orders_gpu.py: the smallest mono
NT = 32 files that still enter each hot loop of the streaming kernel (csrc/sinc2.hip) and leave it again.

Shape: 40 full 1024-output tiles and a partial one (about 41 500 outputs).  The launch cuts a file this short into streams of
three tiles (make_stream_args: nine tiles per wave, and the whole file falls into the launch's last round of third-length
streams); the first, the last two full and the partial tile are the end tiles' workgroups.
A speed s moves the read head by 1 / s input samples per output (oracle_c.speed_to_pos): s > 1 is a period below 1, fc = 1;
s < 1 is a period above 1, fc = s < 1, and the moment correction runs in 1 - fc = 1 - s.
Curves, sampled every 256 input samples:
    fast6    constant 1.006                      fc = 1: the fc = 1 kernel <1, 1> only
    mixed    1 + 0.01 sin, period 12 tiles       the speed moves by up to 5.1e-6 per sample: beyond the 2.7e-6 to which the plan's
                                                 block records are plain quadratics (pos.hip seg_fast_record), so the blocks on the
                                                 curve's flanks carry the cubic flag and their tiles are the block kernel's (28 of
                                                 41 through the list); the loops get the stretches around the extrema
    fast115  constant 1.0115                     fc = 1 again, the 128 centres of a pass hold 129.5 outputs
    slow6    constant 0.994                      1 - fc = 0.0060: the fc < 1 loop to order 5 only
    list     `mixed`, 64 samples set to 40.0     beyond the float16 images' range: the pass leaves the loop, its tile goes to
                                                 the block kernel's list, the loop is primed again behind it
    order6   constant 0.9886                     1 - fc = 0.0114 > 0.0105: the order-6 loop, which none of the above enters
                                                 (not 1 / 1.0115: a period of 1.0115 puts every 2000th position ON a half-integer,
                                                 and window-centre ties are the block kernel's)
    mixed25  1 + 0.01 sin, period 25 tiles       2.5e-6 per sample: every block a plain record, so regimes change inside streams,
                                                 both kernels of the launch get streams and NO tile leaves for the list
    list25   `mixed25` with the 64 samples       the tile list's way out of the loop and back, from an empty list
Signals: seeded noise at 0.5 peak, a 0.49 fs tone."""
import functools

import numpy as np

NT = 32
TILE = 1024
OUT_TARGET = 41_500                              # 40 full tiles + 540 outputs
SPIKE_TILE, SPIKE_LEN, SPIKE_VALUE = 20, 64, 40.0
CURVES = ("fast6", "mixed", "fast115", "slow6", "list", "order6", "mixed25", "list25")
SIGNALS = ("noise", "tone")


CONSTANT = {"fast6": 1.006, "fast115": 1.0115, "slow6": 0.994, "order6": 0.9886}
SINE_PERIOD_TILES = {"mixed": 12.0, "list": 12.0, "mixed25": 25.0, "list25": 25.0}


def _speed(curve, st):
    if curve in CONSTANT:
        return np.full(len(st), CONSTANT[curve])
    return 1.0 + 0.01 * np.sin(2.0 * np.pi * st / (SINE_PERIOD_TILES[curve] * TILE))


def curve(name):
    """(sampletimes, speeds, n_in) of one curve"""
    n = int(round(OUT_TARGET / CONSTANT.get(name, 1.0)))            # len_out ~ n_in x speed
    m = n // 256
    st = np.linspace(0, n, m)
    return st, _speed(name, st), n


def signal(name, curve_name, n):
    if name == "noise":
        x = np.random.default_rng(8).standard_normal(n)
        x = (0.5 * x / np.max(np.abs(x))).astype(np.float32)
    else:
        x = np.cos(0.98 * np.pi * np.arange(n) + 0.3).astype(np.float32)
    if curve_name in ("list", "list25"):
        at = SPIKE_TILE * TILE + 300             # (speed ~ 1 there: input sample ~ output sample, inside tile 20 either way)
        x[at:at + SPIKE_LEN] = np.float32(SPIKE_VALUE)
    return x


@functools.lru_cache(maxsize=None)
def case(curve_name, signal_name):
    """(sampletimes, speeds, n_in, signal, oracle positions, oracle output); computed once, read-only"""
    from oracle import oracle_c as C
    st, sp, n = curve(curve_name)
    pos, _ = C.speed_to_pos(st, sp, n)
    x = signal(signal_name, curve_name, n)
    want = C.sinc(pos, x, NT, threads=4)
    for a in (st, sp, x, pos, want):
        a.setflags(write=False)
    return st, sp, n, x, pos, want
