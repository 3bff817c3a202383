"""Group delay by bands (the reference's experiments/group_delay.py, get_group_delay :30-96) on the device.

The script splits f_lower .. f_upper into log-spaced bands (:41, :54), filters both transfers with an order-1 zero-phase
Butterworth band-pass per band (:61-62), correlates the two WHOLE filtered signals (:69), takes the parabola-refined peak
lag (:72-75) and the two RMS levels (:77-78), and keeps the band when the correlation exceeds min_corr (:79-86).  The curve
of lag against frequency is then compared with a Bessel low-pass's phase delay (:118-138, filter_phase_delay here) to find
the head or crosstalk filter of a tape.

Here a chunk of bands is ONE batch: the two signals, extended at their ends as scipy extends them, are replicated band by
band in HBM, every band's filter runs in one K_sosfiltfilt batch (filters.bandpass_batch_dev) and every band's delay search
in one par_find_delay_sect_f64 call (correlation.find_delay_rows_dev), which also hands back the norms the levels come
from.  Nothing waits for the device until the per-band results are read at the end.
"""
import logging
import warnings
from collections import namedtuple

import numpy as np
import scipy.signal
import torch

from . import _dev, _lib, correlation, filters

GroupDelay = namedtuple("GroupDelay", "band_lo band_hi band_centers lags correlations magnitudes kept levels_ref levels_src "
                                      "lags_all correlations_all")


def BATCHED(n, n_bands):
    """Whether `measure` sends its bands through par_find_delay_sect_f64 (True) or through a loop of correlation.find_delay
    (False), for signals of n samples and n_bands bands: the rule read off tools/bench_group_delay.py's figures
    (profiles/group_delay_bench.json, NOTES.md "Group delay").  On the MI355X the one call won at every measured shape -- 17 x the
    loop at 10 s of 44.1 kHz, 2.9 x at 60 s, 2.0 x at 180 s, 43 bands -- so the rule is "always"; the loop stays for comparison."""
    return True


def band_limits(f_lower=10, f_upper=2000, bandwidth=45):
    """The script's band edges (:41, :54): int((f_upper - f_lower) / bandwidth) log-spaced edges, TRUNCATED to uint16 like
    the reference's dtype=np.uint16 -- the first edge of the defaults is 9, not 10.  Two equal neighbours (narrow bands at low
    frequencies) make scipy's butter fail in the reference: a ValueError that names the band here."""
    num_bands = int((f_upper - f_lower) / bandwidth)
    edges = np.logspace(np.log2(f_lower), np.log2(f_upper), num=num_bands, endpoint=True, base=2, dtype=np.uint16)
    for k in range(len(edges) - 1):
        if edges[k] == edges[k + 1]:
            raise ValueError(f"band {k} is empty: both its edges truncate to {int(edges[k])} Hz (f_lower {f_lower}, f_upper {f_upper}, "
                             f"bandwidth {bandwidth})")
    return edges


def _span(n_ref, n_src, sr, t0, t1):
    """(s_start, s_end) of :43-50: the span the script meant to select with t0, t1, or -- what it actually runs -- 0 .. len(src)"""
    s_start = 0 if t0 is None else int(t0 * sr)
    s_end = n_src if t1 is None else int(t1 * sr)
    if s_start < 0 or s_end <= s_start:
        raise ValueError(f"empty span: samples {s_start} .. {s_end}")
    return s_start, s_end


def _row(sig, dev):
    """the signal on the device: float32 stays float32 (it crosses the bus as it is and widens in HBM, AFTER the extension
    below), everything else becomes float64"""
    if isinstance(sig, torch.Tensor):
        if sig.ndim != 1:
            raise ValueError("measure takes 1-D signals")
        return sig.to(device=f"cuda:{dev}", dtype=torch.float32 if sig.dtype == torch.float32 else torch.float64)
    sig = np.asarray(sig)
    if sig.ndim != 1:
        raise ValueError("measure takes 1-D signals")
    return _dev.to_dev(sig, torch.float32 if sig.dtype == np.float32 else torch.float64, dev)


def _odd_ext(x_t, pad):
    """scipy's odd_ext(x, pad) as sosfiltfilt forms it, IN THE SIGNAL'S OWN dtype (2 x[0] - x[pad:0:-1] | x | 2 x[-1] -
    x[-2:-pad-2:-1]), then float64.  The reference hands float32 signals to scipy, whose extension is then rounded to float32
    before the float64 recurrence sees it; a narrow low band carries that into its correlation (1e-9 at 12-14 Hz on the
    fixture), so the extension is formed here as scipy forms it and K_sosfiltfilt filters the extended row with padlen 0."""
    n = x_t.numel()
    if n <= pad:
        raise ValueError("The length of the input vector x must be greater than padlen, which is %d." % pad)
    if pad == 0:
        return x_t.double()
    left = 2 * x_t[:1] - x_t[1:pad + 1].flip(0)
    right = 2 * x_t[-1:] - x_t[n - pad - 1:n - 1].flip(0)
    return torch.cat((left, x_t, right)).double()


def _shape_key(sos):
    return None if sos is None else (sos.shape[0], filters._padlen(sos))


def measure(ref_sig, src_sig, sr, f_lower=10, f_upper=2000, bandwidth=45, t0=None, t1=None, min_corr=0.6, order=1, strict=True,
            batched=None, section=None, max_bytes=4 << 30, device=None):
    """get_group_delay(ref_sig, src_sig) (:30-96) -> GroupDelay.  ref_sig, src_sig: 1-D numpy arrays or device tensors; a float32
    signal is extended at its ends in float32, as scipy's sosfiltfilt does for the reference, and filtered in float64.

    band_lo, band_hi, lags_all, correlations_all, kept, levels_ref, levels_src hold every band; band_centers, lags,
    correlations, magnitudes are the script's four lists -- the kept bands, in its order.  lags = s_dur // 2 - i_interp
    (the exact negation of find_delay's delay), levels = RMS of the filtered spans, magnitudes = ref level - src level:
    the reference's LINEAR difference, kept as it is.  A band is kept only if corr > min_corr (NaN fails).  A peak on the last
    lag raises the reference's IndexError under `strict`; otherwise that band is dropped with a warning.
    batched: None = the measured rule BATCHED; section: section_log2 of the delay search (None: its own choice);
    max_bytes: device bytes a chunk of bands may take (at least one band goes through)."""
    dev = _dev.device_index(device if device is not None else (ref_sig.device if isinstance(ref_sig, torch.Tensor) else None))
    edges = band_limits(f_lower, f_upper, bandwidth)
    lo, hi = edges[:-1].astype(np.float64), edges[1:].astype(np.float64)
    n_bands = len(lo)
    ref_t, src_t = _row(ref_sig, dev), _row(src_sig, dev)
    s_start, s_end = _span(ref_t.numel(), src_t.numel(), sr, t0, t1)
    s_dur = s_end - s_start
    ref_t, src_t = ref_t[s_start:s_end], src_t[s_start:s_end]
    na, nb = ref_t.numel(), src_t.numel()
    if na < 3 or nb < 1:
        raise ValueError(f"the span holds {na} and {nb} samples")
    if batched is None:
        batched = BATCHED(max(na, nb), n_bands)
    designs = [filters._design(float(a), float(b), sr, order) for a, b in zip(lo, hi)]
    groups = {}                                             # cascade shape -> bands, in the script's order
    for k, sos in enumerate(designs):
        groups.setdefault(_shape_key(sos), []).append(k)
    # a chunk holds per band the two replicated rows, their filtered copies and the filter's work, and the search's scratch
    per_band = 8 * (na + nb) * 4
    chunk = max(1, int((max_bytes // 2) // per_band))
    delays = torch.full((n_bands,), float("nan"), dtype=torch.float64, device=f"cuda:{dev}")
    corrs, status = torch.full_like(delays, float("nan")), torch.zeros(n_bands, dtype=torch.int32, device=f"cuda:{dev}")
    norms = torch.full((n_bands, 2), float("nan"), dtype=torch.float64, device=f"cuda:{dev}")
    host_loop = {}
    L = _lib.lib()
    for key, bands in groups.items():
        pad = 0 if key is None else key[1]                  # scipy's default padlen of this cascade shape
        ea, eb = _odd_ext(ref_t, pad), _odd_ext(src_t, pad)
        for c0 in range(0, len(bands), chunk):
            sel = bands[c0:c0 + chunk]
            k = len(sel)
            if na == nb:
                x = _dev.empty((2 * k, na + 2 * pad), torch.float64, dev)
                x[:k] = ea
                x[k:] = eb
                y = x if key is None else filters.bandpass_batch_dev(x, np.tile(lo[sel], 2), np.tile(hi[sel], 2), sr, order, dev, padlen=0)
                ya, yb = y[:k, pad:pad + na], y[k:, pad:pad + nb]
            else:                                           # rows of two lengths: a batch each
                xa, xb = ea.expand(k, na + 2 * pad).contiguous(), eb.expand(k, nb + 2 * pad).contiguous()
                ya = (xa if key is None else filters.bandpass_batch_dev(xa, lo[sel], hi[sel], sr, order, dev, padlen=0))[:, pad:pad + na]
                yb = (xb if key is None else filters.bandpass_batch_dev(xb, lo[sel], hi[sel], sr, order, dev, padlen=0))[:, pad:pad + nb]
            idx = torch.as_tensor(sel, dtype=torch.int64, device=f"cuda:{dev}")
            if batched:
                sec = correlation._auto_section(na, nb) if section is None else int(section)
                nbytes = max(int(L.par_find_delay_sect_scratch_bytes(na, nb, 1, sec)),       # one row's worth at the least
                             min(int(L.par_find_delay_sect_scratch_bytes(na, nb, k, sec)), int(max_bytes // 2)))
                d, c, st, nr = correlation.find_delay_rows_dev(ya, yb, False, section, want_norms=True, scratch_bytes=nbytes)
                delays[idx], corrs[idx], status[idx], norms[idx] = d, c, st, nr
            else:                                           # the comparison route: the norms are torch's here (another summation order)
                norms[idx] = torch.stack((torch.linalg.vector_norm(ya, dim=1), torch.linalg.vector_norm(yb, dim=1)), dim=1)
                for j, band in enumerate(sel):
                    try:
                        host_loop[band] = correlation.find_delay(ya[j], yb[j]) + (0,)
                    except IndexError:
                        host_loop[band] = (np.nan, np.nan, 1)
    delays, corrs, status, norms = (_dev.to_host(t) for t in (delays, corrs, status, norms))
    for band, (d, c, st) in host_loop.items():
        delays[band], corrs[band], status[band] = d, c, st
    for band in np.flatnonzero(status == 1):
        msg = f"index {na} is out of bounds for axis 0 with size {na} (band {int(band)}, {int(edges[band])} .. {int(edges[band + 1])} Hz)"
        if strict:
            raise IndexError(msg)
        warnings.warn(f"band dropped, its correlation peaks on the last lag: {msg}")
    lags_all = float(s_dur // 2 - na // 2) - delays
    levels_ref, levels_src = norms[:, 0] / np.sqrt(float(na)), norms[:, 1] / np.sqrt(float(nb))
    kept = corrs > min_corr                                 # NaN fails, like the reference's `if corr > min_corr`
    for band in np.flatnonzero(~kept & (status == 0)):
        logging.warning(f"Band had too little correlation {corrs[band]}")
    centers = (edges[:-1] + edges[1:]) / 2                  # uint16 sums, like the script's
    return GroupDelay(edges[:-1].copy(), edges[1:].copy(), centers[kept], lags_all[kept], corrs[kept], (levels_ref - levels_src)[kept],
                      kept, levels_ref, levels_src, lags_all, corrs)


def filter_phase_delay(sos, sr, worN=512):
    """The overlay of :124-138 for one filter: (freqs_hz, delay_samples) with w, h = freqz_sos(sos), phase = unwrap(angle(h)),
    freqs_hz = w / pi * sr / 2 and delay = -(phase / (2 pi)) * sr / freqs_hz -- the script's arithmetic, on the host (the
    point at 0 Hz divides by zero, as it does there)."""
    freqz_sos = getattr(scipy.signal, "freqz_sos", None) or scipy.signal.sosfreqz       # one function under its new and old name
    w, h = freqz_sos(sos, worN=worN)
    phase = np.unwrap(np.angle(h))
    freqs_hz = w / np.pi * sr / 2
    with np.errstate(divide="ignore", invalid="ignore"):
        return freqs_hz, -(phase / (2 * np.pi)) * sr / freqs_hz


def measure_file(path, ref_channel=0, src_channel=1, **kw):
    """measure() on two channels of one file (the script's get_group_delay(sig[:, 0], sig[:, 1]), :149-150)"""
    from . import io_ops
    sig, sr, ch = io_ops.read_file(path)
    if not (0 <= ref_channel < ch and 0 <= src_channel < ch):
        raise ValueError(f"{path} has {ch} channel(s)")
    return measure(sig[:, ref_channel], sig[:, src_channel], sr, **kw)


def report(result):
    """the figures of a GroupDelay as plain Python values (what the CLI writes with --json)"""
    out = {k: np.asarray(getattr(result, k)).tolist() for k in GroupDelay._fields}
    out["n_bands"] = int(len(result.kept))
    out["n_kept"] = int(np.count_nonzero(result.kept))
    return out
