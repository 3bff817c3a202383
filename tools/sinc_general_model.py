"""Numerical model of K_sinc's fc < 1 tap loops (taps_general / taps_general_ct, csrc/sinc_block.h): the loop restated in float32
numpy -- same seeding, same `gentle` branch, same fma order, R_n exact -- against a float64 evaluation of the reference's sum.

  out = centre + s accM + accP,   accM = sum_n (G - H) R_n,  accP = sum_n n (G + H) R_n,   G = x[c+n] U_n,  H = x[c-n] V_n
  U_n = sin(theta (n - s)),  V_n = sin(theta (n + s)),  theta = pi fc,  R_n = (win_n / pi) / (n^2 - s^2)

How U_n, V_n are carried (--form):
  plain     U_{n+1} = c2 U_n - U_{n-1}, c2 = 2 cos(theta), from n = 1 to NT.  With fc just below 1 the rounding of c2 ~ -2 alone
            turns the angle by 6e-8 / sin(pi dd) per step, and every rounding of U is amplified by 1 / sin(theta) on its way out.
  reseed    the same recurrence, restarted every SEG taps from sinpi of the reduced angle:
            (n -+ s) fc = n - (n dd +- h), h = fc s, so U_n = -(-1)^n sinpi(n dd + h), V_n = -(-1)^n sinpi(n dd - h);
            n dd is split into a float32 product and its fma remainder, so the fraction is as good as dd itself -- and far out a
            float32 dd is not good enough (n dd ~ 280 to 1e-6 at NT = 512, fc = 0.45): the position-array form hands on what of
            1 - fc lies below it (ddl; place() below restates place_from_pos and k_sinc_pos, the hardware reciprocal taken to be
            up to one ulp off).  `plain` at fc <= 0.6 is as bad as it is for that reason, not for the recurrence's.
The signal on which the drift adds coherently is a tone AT the cutoff, cos(pi fc n + phi); noise is the benign case.

usage: python tools/sinc_general_model.py [--form plain|reseed] [--seg 8] [--quick]
Prints the worst absolute error on a unit tone (output peak ~ 0.5) per NT and fc; the contract is 1e-5 of the output peak."""
import argparse

import numpy as np

f32 = np.float32


def fma(a, b, c):
    return (np.asarray(a, dtype=np.float64) * np.asarray(b, dtype=np.float64) + np.asarray(c, dtype=np.float64)).astype(f32)


def sinpi_half(x):
    x = x.astype(f32)
    z = x * x
    p = np.full_like(x, f32(-0.00737043094))
    for c in (0.0821458866, -0.599264529, 2.55016404, -5.16771278, 3.14159265):
        p = fma(p, z, f32(c))
    return p * x


def cospi_half(x):
    x = x.astype(f32)
    z = x * x
    p = np.full_like(x, f32(0.00192957431))
    for c in (-0.0258068914, 0.235330630, -1.33526277, 4.05871213, -4.93480220, 1.0):
        p = fma(p, z, f32(c))
    return p


def sinpi_reduced(hi, lo, plus):
    """sinpi(hi + lo + plus) for a float32 product hi with its exact remainder lo: the whole part of hi leaves exactly"""
    k = np.rint(hi)
    r = ((hi - k).astype(f32) + (lo + plus).astype(f32)).astype(f32)          # |r| <= 1: fold once more
    k2 = np.rint(r)
    r = (r - k2).astype(f32)
    odd = (k.astype(np.int64) + k2.astype(np.int64)) & 1
    v = sinpi_half(r)
    return np.where(odd == 1, -v, v).astype(f32)


def seeds_at(n, dd, ddl, h):
    """(U_n, V_n) from the reduced angle; 1 - fc = dd + ddl"""
    fn = f32(n)
    hi = (fn * dd).astype(f32)
    lo = fma(fn, ddl, fma(fn, dd, -hi))
    sign = f32(1.0 if n % 2 else -1.0)                                         # -(-1)^n
    return sign * sinpi_reduced(hi, lo, h), sign * sinpi_reduced(hi, lo, -h)


def model(x, c, s, fc, dd, NT, form="reseed", seg=8, ddl=None):
    """float32 taps_general on outputs with window centres c (indices into x), shifts s, cutoffs fc, dd = 1 - fc (arrays)"""
    win = np.hanning(2 * NT + 1).astype(f32)[NT:].astype(np.float64)
    s, fc, dd = s.astype(f32), fc.astype(f32), dd.astype(f32)
    ddl = np.zeros_like(dd) if ddl is None else ddl.astype(f32)
    x = x.astype(f32)
    h = (fc * s).astype(f32)
    sphi = sinpi_half(h)
    if np.all(dd <= f32(0.03125)):                                             # `gentle` is wave-wide; here: the whole run
        z = dd * dd
        U, V = sinpi_half(dd + h), sinpi_half(dd - h)
        c2 = fma(z, fma(z, f32(-8.11742426), f32(9.86960440)), f32(-2.0))
    else:
        cphi = cospi_half(h)
        low = dd <= f32(0.5)
        sth = np.where(low, sinpi_half(dd), sinpi_half(fc)).astype(f32)
        cth = np.where(low, -cospi_half(dd), cospi_half(fc)).astype(f32)
        U, V = fma(sth, cphi, -(cth * sphi).astype(f32)), fma(sth, cphi, (cth * sphi).astype(f32))
        c2 = (f32(2.0) * cth).astype(f32)
    Up, Vp = -sphi, sphi.copy()
    q = (s * s).astype(f32)
    centre = x[c] * (Up * (f32(1.0) / (s * f32(-np.pi))).astype(f32)).astype(f32)
    accP, accM = np.zeros_like(s), np.zeros_like(s)
    for n in range(1, NT):                                                      # (tap -NT has weight 0, tap +NT is outside)
        if form == "reseed" and n > 1 and (n - 1) % seg == 0:
            Up, Vp = seeds_at(n - 1, dd, ddl, h)
            U, V = seeds_at(n, dd, ddl, h)
        Rn = ((win[n] / np.pi) / (float(n * n) - q.astype(np.float64))).astype(f32)
        G, H = (x[c + n] * U).astype(f32), (x[c - n] * V).astype(f32)
        accM = fma((G - H).astype(f32), Rn, accM)
        accP = fma(((G + H).astype(f32) * Rn).astype(f32), f32(n), accP)
        U, Up = fma(c2, U, -Up), U
        V, Vp = fma(c2, V, -Vp), V
    return (centre + fma(s, accM, accP)).astype(f32)


def exact(x, c, s, fc, NT):
    win = np.hanning(2 * NT + 1).astype(f32).astype(np.float64)
    k = np.arange(-NT, NT)
    arg = (k[None, :] - s[:, None]) * fc[:, None]
    return np.sum(x.astype(f32).astype(np.float64)[c[:, None] + k[None, :]] * np.sinc(arg) * fc[:, None] * win[None, :2 * NT], axis=1)


def place(period, n, rcp_ulps=0, low_part=True):
    """fc, 1 - fc and the float32 remainder of 1 - fc as place_from_pos hands them on; rcp_ulps: how far the hardware
    reciprocal is taken to be off"""
    inv = f32(1.0) / f32(period)
    for _ in range(abs(rcp_ulps)):
        inv = np.nextafter(inv, f32(2.0 if rcp_ulps > 0 else 0.0))
    dd = f32(f32(period - 1.0) * inv)
    ddl = f32(f32((period - 1.0) - float(dd) * period) * inv) if low_part else f32(0.0)
    return np.full(n, inv, dtype=f32), np.full(n, dd, dtype=f32), np.full(n, ddl, dtype=f32)


def worst_error(NT, fc, form, seg, signal="tone", n_out=1500, seed=7, rcp_ulps=0, low_part=True):
    rng = np.random.default_rng(seed)
    pos = NT + 3.3 + np.arange(n_out) / fc
    c = np.rint(pos).astype(np.int64)
    s = pos - c
    s = np.where(s == 0.0, 1e-20, s)
    fc32, dd32, ddl32 = place(1.0 / fc, n_out, rcp_ulps, low_part and form == "reseed")
    n = np.arange(int(pos[-1]) + NT + 3)
    x = np.cos(np.pi * fc * (n - pos[0])) if signal == "tone" else rng.uniform(-1, 1, len(n))
    got = model(x, c, s, fc32, dd32, NT, form, seg, ddl32)
    want = exact(x, c, s, np.full(n_out, fc), NT)
    return float(np.max(np.abs(got - want))), float(np.max(np.abs(want)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--form", default=None, choices=["plain", "reseed"])
    ap.add_argument("--seg", type=int, default=8)
    ap.add_argument("--quick", action="store_true")
    a = ap.parse_args()
    nts = (50, 100, 512) if a.quick else (32, 50, 64, 100, 128, 200, 512)
    fcs = (0.9995, 0.995, 0.99, 0.985, 0.9, 0.6, 0.45, 0.2)
    for form in ([a.form] if a.form else ["plain", "reseed"]):
        what = "the generic loops before the re-seeding; taps_general_ct<32>, <50> to this day" if form == "plain" else \
            f"taps_general as shipped: re-seeded every {a.seg} taps"
        print(f"--form {form} ({what}): worst |error| on a unit tone at the cutoff (output peak ~0.5) / on unit noise")
        print("  NT " + " ".join(f"{fc:>17}" for fc in fcs))
        for NT in nts:
            cells = []
            for fc in fcs:
                # the hardware reciprocal is good to an ulp: the worst of exact and one ulp either way
                et = max(worst_error(NT, fc, form, a.seg, "tone", rcp_ulps=u)[0] for u in (-1, 0, 1))
                en = max(worst_error(NT, fc, form, a.seg, "noise", rcp_ulps=u)[0] for u in (-1, 0, 1))
                cells.append(f"{et:8.1e}/{en:8.1e}")
            print(f"{NT:4d} " + " ".join(cells))


if __name__ == "__main__":
    main()
