"""Headless pyrespeeder: a fresh replacement for the reference's stale
experiments/pyrespeeder_cmd.py.  Files are independent work items: one host thread per GPU pulls
(file) items from a queue, every file goes STFT -> tracker -> master speed curve -> fused sinc
resample on that GPU, results are written as <stem>_res<suffix>.wav like resampling.run does
(util/resampling.py:235-237).  No Qt, no collective communication.

    python -m pyaudiorestoration_amd.cli respeed --trail 0.2,4000,4.0,4000 tape1.flac tape2.wav
    python -m pyaudiorestoration_amd.cli respeed --project tape.spd tape.flac      # traces / regressions saved by the GUI
    python -m pyaudiorestoration_amd.cli resample --curve curve.json tape.wav      # [[t_seconds, speed], ...]
    python -m pyaudiorestoration_amd.cli resample --speed 1.015 tape.wav           # constant correction
    python -m pyaudiorestoration_amd.cli tapesync --project take.tapesync take2.flac
    python -m pyaudiorestoration_amd.cli heal --project tape.drop tape.flac
    python -m pyaudiorestoration_amd.cli expand --channels L+R --clip -120,-85 tape.wav     # Spectral Expander -> tape_decompressed.wav
    python -m pyaudiorestoration_amd.cli renoise --noise hiss.wav tape.wav                  # renoiser -> "tape fft=2048.wav"
    python -m pyaudiorestoration_amd.cli renoise --gauge tape.wav                           # "Gauge offset": logs the best pad
    python -m pyaudiorestoration_amd.cli renoise --noise hiss.wav --offset auto tape.wav    # ... and applies with it
    python -m pyaudiorestoration_amd.cli hpss --kernel 31,17 --margin 2,3 take.flac         # -> take_H.wav, take_P.wav, take_R.wav
    python -m pyaudiorestoration_amd.cli humspeed --hum 50 --resample tape.wav              # -> tape_resampled_<percent>.wav
    python -m pyaudiorestoration_amd.cli dynamics remaster.flac original.flac               # -> remaster.flacdecompressed.wav
    python -m pyaudiorestoration_amd.cli azimuth take.tapesync --ref take1.flac --box 12,300,22,3000 --out take2.tapesync
    python -m pyaudiorestoration_amd.cli pan tape.pan                                       # stereo balance project -> tape_out.wav
    python -m pyaudiorestoration_amd.cli pan --box 12,300,14,5000 --fft 4096 --overlap 8 tape.wav --out tape.pan --apply
    python -m pyaudiorestoration_amd.cli difeq transfer.wav master.wav --out eq.txt         # Differential EQ -> eq.txt, eq_L.txt, eq_R.txt
    python -m pyaudiorestoration_amd.cli cyclic side_a.wav --rpm 33.333 --pilot 3150 --resample   # cyclic wow of a pilot tone -> side_a_res.wav
    python -m pyaudiorestoration_amd.cli flutter tape.flac --band 3000,5000 --resample            # zero-crossing flutter of a pilot tone -> tape_res.wav
    python -m pyaudiorestoration_amd.cli spectrogram tape.flac --range 60,75 --freq 20,12000     # the picture -> tape_spec.png + tape_spec.json
    python -m pyaudiorestoration_amd.cli spectrogram tape.flac --range 60,75 --at 512,300        # (s, Hz) of a pixel of that picture
"""
import argparse
import json
import logging
import os
import queue
import sys
import threading

import numpy as np


def _worker(dev, jobs, args, results):
    """One host thread per GPU.  The next file of the queue is read and decoded (native FLAC decoder / numpy, both
    release the GIL) on a helper thread while the current one is on the GPU."""
    from concurrent.futures import ThreadPoolExecutor
    import torch
    from . import _dev, expander, hpss, humspeed, io_ops, pipeline, renoiser, resampling
    torch.cuda.set_device(dev)

    def take():
        try:
            path = jobs.get_nowait()
        except queue.Empty:
            return None
        if args.cmd in ("tapesync", "heal", "humspeed") or (args.cmd == "respeed" and args.project):   # these flows read their source themselves
            return path, None
        return path, reader.submit(io_ops.read_file, path)

    with ThreadPoolExecutor(max_workers=1) as reader:
        nxt = take()
        while nxt is not None:
            (path, pending), nxt = nxt, take()       # the next file starts decoding now
            try:
                if args.cmd in ("tapesync", "heal") or (args.cmd == "respeed" and args.project):
                    flow = {"tapesync": pipeline.tapesync, "heal": pipeline.heal_project, "respeed": pipeline.respeed_project}[args.cmd]
                    if args.cmd == "respeed":       # --suffix / --quality / --resampling override the project's own only when given
                        flow(args.project, source=path, out_suffix=args.suffix, device=dev, sinc_quality=args.quality,
                             resampling_mode=getattr(args, "resampling", None))
                    else:
                        flow(args.project, source=path, out_suffix=args.suffix, device=dev)
                    results.append((path, None))
                    continue
                if args.cmd == "humspeed":
                    res = humspeed.analyse(path, args.channels, args.hum, args.harmonies, args.tolerance, args.fft)
                    for f, db, ratio in zip(res["marker_freqs"], res["marker_dBs"], res["ratios"]):
                        logging.info("%s: marker %.4f Hz %.2f dB, Percent Change: %.3f", path, f, db, (ratio - 1) * 100)
                    if not res["ratios"]:
                        logging.warning("%s: hum was not close enough", path)
                    elif args.resample:                 # the last ratio, like the GUI's Resample button
                        logging.info("%s: wrote %s", path, humspeed.resample_file(path, res["ratios"][-1], device=dev))
                    results.append((path, None))
                    continue
                signal, sr, ch = pending.result()
                if args.cmd == "expand":
                    expander.expand_file(path, args.channels, args.fft_size, args.hop, args.band[0], args.band[1], args.smoothing,
                                         args.clip[0], args.clip[1], args.transition, args.order, args.suffix, device=dev,
                                         signal_data=(signal, sr, ch))
                    results.append((path, None))
                    continue
                if args.cmd == "renoise" and args.gauge:        # "Gauge offset" on channel 0: no audio is written
                    _, stds, pad = renoiser.sniff_offset(signal, sr, args.fft, args.fft // args.overlap, 0, device=dev)
                    logging.info("%s: gauge maximum %.9g at pad %d of %d", path, stds[pad], pad, len(stds))
                    results.append((path, None))
                    continue
                if args.cmd == "renoise":
                    renoiser.renoise_file(path, args.noise, args.select, args.fft, args.overlap, args.gain, args.overhead, args.curve,
                                          args.channels, device=dev, signal_data=(signal, sr, ch), resample_noise=args.resample_noise,
                                          offset=args.offset)
                    results.append((path, None))
                    continue
                if args.cmd == "hpss":
                    hpss.separate_file(path, args.fft, args.overlap, args.kernel, args.power, args.margin, device=dev,
                                       signal_data=(signal, sr, ch))
                    results.append((path, None))
                    continue
                quality = 50 if args.quality is None else args.quality          # the GUI's default (util/widgets.py:998-1000)
                suffix = args.suffix or ""
                if args.cmd == "respeed":
                    t0, f0, t1, f1 = args.trail
                    r = pipeline.respeed(signal, sr, [(t0, f0), (t1, f1)], args.fft_size, args.hop, 1, args.mode,
                                         args.tolerance, (0, args.lowpass), quality, device=dev)
                    out = _dev.to_host(r["output"])
                    io_ops.write_wav_float(f"{os.path.splitext(path)[0]}_res{suffix}.wav", out, sr)
                    np.save(f"{os.path.splitext(path)[0]}_speed{suffix}.npy", r["speed_curve"])
                else:
                    if args.speed is not None:          # constant correction: a two-point curve over the whole file
                        curve = np.array([[0.0, args.speed], [len(signal) / sr, args.speed]], dtype=np.float64)
                    else:
                        curve = np.asarray(json.load(open(args.curve)), dtype=np.float64)
                    resampling.run((path,), signal_data=((signal, sr),), speed_curve=curve, resampling_mode=args.resampling,
                                   sinc_quality=quality, suffix=suffix)
                results.append((path, None))
            except Exception as e:                      # keep the other files going; report at the end
                logging.exception(f"{path} failed")
                results.append((path, e))


def parser():
    ap = argparse.ArgumentParser(prog="pyaudiorestoration_amd.cli")
    sub = ap.add_subparsers(dest="cmd", required=True)
    a = sub.add_parser("respeed", help="trace a pilot tone / hum and remove wow & flutter")
    what = a.add_mutually_exclusive_group(required=True)
    what.add_argument("--trail", type=lambda s: [float(v) for v in s.split(",")], help="t0,f0,t1,f1 (s, Hz): trace it here")
    what.add_argument("--project", help=".spd JSON written by the GUI: its traces and regressions make the master curve")
    a.add_argument("--mode", default="Peak", help="tracker name as in wow_detection.wow_detectors")
    a.add_argument("--tolerance", type=float, default=0.5, help="semitones")
    a.add_argument("--fft-size", type=int, default=1024)
    a.add_argument("--hop", type=int, default=256)
    a.add_argument("--lowpass", type=float, default=20.0, help="speed-curve low-pass (Hz)")
    b = sub.add_parser("resample", help="apply a given speed curve")
    how = b.add_mutually_exclusive_group(required=True)
    how.add_argument("--curve", help="JSON [[t_seconds, speed], ...]")
    how.add_argument("--speed", type=float, help="constant speed factor of the recording (1.015 = it ran 1.5 %% fast)")
    b.add_argument("--resampling", default="Sinc", choices=("Sinc", "Linear"))
    c = sub.add_parser("tapesync", help="apply the lag curve of a saved pytapesynch project (.tapesync) to files")
    c.add_argument("--project", required=True, help=".tapesync JSON written by the GUI")
    d = sub.add_parser("heal", help="inpaint the marked dropouts of a saved dropout-healer project (.drop)")
    d.add_argument("--project", required=True, help=".drop JSON written by the GUI")
    for p in (a, b, c, d):
        p.add_argument("--quality", type=int, default=None, help="sinc_quality (NT); default: the project's, else the GUI's 50")
        p.add_argument("--suffix", default=None, help="output suffix; default: the project's, else none")
        p.add_argument("--gpus", type=int, default=0, help="GPUs to use (0 = all visible)")
        p.add_argument("files", nargs="+")
    pair = lambda s: [float(v) for v in s.split(",")]
    e = sub.add_parser("expand", help="Spectral Expander: boost quiet passages by the level of a noise-floor band")
    e.add_argument("--channels", default="L+R", choices=("L+R", "L", "R", "Mean"), help="which channels are analysed")
    e.add_argument("--band", type=pair, default=[13000.0, 17000.0], help="LO,HI (Hz): the noise-floor band")
    e.add_argument("--clip", type=pair, default=[-120.0, -85.0], help="LO,HI (dB): gain boundaries of the noise floor")
    e.add_argument("--smoothing", type=float, default=0.11, help="smoothing window (s)")
    e.add_argument("--transition", type=int, default=0, help="high-pass transition (Hz); 0: the whole band is expanded")
    e.add_argument("--order", type=int, default=1, help="order of the transition filters")
    e.add_argument("--fft-size", type=int, default=512)
    e.add_argument("--hop", type=int, default=64)
    e.add_argument("--suffix", default="_decompressed", help="output suffix")
    e.add_argument("--gpus", type=int, default=0, help="GPUs to use (0 = all visible)")
    e.add_argument("files", nargs="+")
    ints = lambda s: [int(v) for v in s.split(",") if v != ""]
    curve = lambda s: [[float(v) for v in p.split(":")] for p in s.split(",")]
    r = sub.add_parser("renoise", help="renoiser: gate (or boost) every STFT bin at or under a noise profile + gain + overhead")
    prof = r.add_mutually_exclusive_group()
    prof.add_argument("--noise", default=None, help="noise recording at the file's sample rate (its first channel is the profile)")
    r.add_argument("--resample-noise", action="store_true", help="resample a noise recording at another rate to the file's (default: refuse it)")
    prof.add_argument("--select", type=pair, default=None, help="T0,T1 (s): the profile is this time range of channel 0")
    r.add_argument("--fft", type=int, default=2048, help="FFT size")
    r.add_argument("--overlap", type=int, default=4, help="hop = fft / overlap")
    r.add_argument("--gain", type=float, default=12.0, help="dB applied to every bin at or under the final profile")
    r.add_argument("--overhead", type=float, default=3.0, help="dB added to the profile")
    r.add_argument("--curve", type=curve, default=None, help="F:DB,... control curve (default 1:0,<sr/2>:0)")
    r.add_argument("--channels", type=ints, default=None, help="channel numbers, e.g. 0,1 (default: all)")
    r.add_argument("--gauge", action="store_true", help="only gauge the frame offset of an earlier denoise on channel 0 and log it")
    r.add_argument("--offset", type=lambda s: s if s == "auto" else int(s), default=0,
                   help="zeros in front of the signal before the STFT, 0 <= K < hop, or 'auto' for the gauged pad")
    r.add_argument("--gpus", type=int, default=0, help="GPUs to use (0 = all visible)")
    r.add_argument("files", nargs="+")

    def one_or_two(kind):
        def parse(s):
            v = [kind(x) for x in s.split(",")]
            if len(v) not in (1, 2):
                raise argparse.ArgumentTypeError(f"one value or two (harmonic,percussive): {s!r}")
            return v[0] if len(v) == 1 else tuple(v)
        return parse
    h = sub.add_parser("hpss", help="harmonic / percussive separation by median filtering: <stem>_H.wav, _P.wav (and _R.wav)")
    h.add_argument("--fft", type=int, default=512, help="FFT size")
    h.add_argument("--overlap", type=int, default=4, help="hop = fft / overlap")
    h.add_argument("--kernel", type=one_or_two(int), default=(31, 31), help="median sizes HARMONIC,PERCUSSIVE (1..99; one value: both)")
    h.add_argument("--power", type=float, default=2.0, help="exponent of the soft mask (inf: hard mask)")
    h.add_argument("--margin", type=one_or_two(float), default=1.0, help="mask margin(s) >= 1; other than 1 also writes the residual")
    h.add_argument("--gpus", type=int, default=0, help="GPUs to use (0 = all visible)")
    h.add_argument("files", nargs="+")
    m = sub.add_parser("humspeed", help="hum speed analysis: how far the mains hum is off its nominal frequency; --resample corrects it")
    m.add_argument("--channels", default="L+R", choices=("L+R", "L", "R"), help="which channels are analysed")
    m.add_argument("--hum", type=int, default=50, help="base frequency of the hum (Hz)")
    m.add_argument("--harmonies", type=int, default=2, help="number of hum harmonics to consider")
    m.add_argument("--tolerance", type=int, default=8, help="largest deviation from a hum frequency (percent)")
    m.add_argument("--fft", type=int, default=524288, help="FFT size of the averaged spectrum")
    m.add_argument("--resample", action="store_true", help="write <stem>_resampled_<percent>.wav, corrected by the last ratio")
    m.add_argument("--gpus", type=int, default=0, help="GPUs to use (0 = all visible)")
    m.add_argument("files", nargs="+")
    y = sub.add_parser("dynamics", help="dynamics matcher (decompressor_cmd): restore SRC's dynamics to those of REF -> SRC + 'decompressed.wav'")
    y.add_argument("src", metavar="SRC", help="the transfer to restore")
    y.add_argument("ref", metavar="REF", help="a transfer of the same recording with the intended dynamics (same length, rate and channels)")
    z = sub.add_parser("azimuth", help="tape-sync azimuth mode: measure one azimuth line of a pytapesynch project (.tapesync)")
    z.add_argument("project", metavar="PROJECT", help=".tapesync JSON written by the GUI")
    z.add_argument("--ref", required=True, help="the reference file")
    z.add_argument("--src", default=None, help="the file to synchronise (default: the project's source)")
    z.add_argument("--box", required=True, type=pair, help="T0,F0,T1,F1 (s, Hz): the selection in the reference's spectrogram")
    z.add_argument("--win", type=float, default=0.2, help="half window (s)")
    z.add_argument("--overlap", type=int, default=32, help="windows per half window")
    z.add_argument("--reject", type=float, default=0.1, help="lags whose |correlation| is below this are interpolated over")
    z.add_argument("--ignore-phase", action="store_true", help="correlate on |.|")
    z.add_argument("--out", default=None, metavar="PROJECT2", help="write the project with the line appended (default: only log)")
    w = sub.add_parser("pan", help="stereo balance (pypan): apply a .pan project, or measure L/R boxes and append them to one")
    w.add_argument("file", metavar="FILE", help="a .pan JSON written by the GUI or by --out (applied), or the stereo file to measure")
    w.add_argument("--box", action="append", type=pair, default=[], help="T0,F0,T1,F1 (s, Hz): a box to measure; may be repeated")
    w.add_argument("--fft", type=int, default=4096, help="FFT size of the measurement")
    w.add_argument("--overlap", type=int, default=8, help="hop = fft / overlap")
    w.add_argument("--zeropad", type=int, default=1, help="zero-padding factor of the measurement")
    w.add_argument("--out", default=None, metavar="PROJECT", help="append the measured markers to this .pan project (created if missing)")
    w.add_argument("--apply", action="store_true", help="after measuring, also write <stem>_out.wav (a project is always applied)")
    w.add_argument("--keep-left", action="store_true", help="extension: write a stereo file with the untouched left channel")
    q = sub.add_parser("difeq", help="Differential EQ: the averaged EQ curve that takes every SRC to its REF, as Audacity FilterCurve presets")
    q.add_argument("files", nargs="+", metavar="SRC REF", help="pairs: the file to equalise, then a transfer of the same recording to match")
    q.add_argument("--out", required=True, metavar="EQ.txt", help="writes EQ.txt (channel mean), EQ_L.txt and EQ_R.txt")
    q.add_argument("--channels", default="L+R", choices=("L+R", "L", "R"), help="which channels are analysed")
    q.add_argument("--highpass", type=int, default=0, help="no influence under this frequency (Hz)")
    q.add_argument("--rolloff", type=pair, default=[21000, 22000], help="A,B (Hz): full influence up to A, none from B on")
    q.add_argument("--resolution", type=int, default=200, help="keys of the output curve, 20..2000")
    q.add_argument("--smoothing", type=int, default=50, help="points of the box average, 1..200")
    q.add_argument("--strength", type=int, default=100, help="percent")
    q.add_argument("--keep-gain", action="store_true", help="take the curve's mean gain off, so that the level stays")
    k = sub.add_parser("cyclic", help="cyclic wow analysis: the wow of an off-centre or warped record, measured from a pilot tone")
    k.add_argument("files", nargs="+")
    k.add_argument("--rpm", type=float, default=45.0, help="nominal rotation: the search starts at its cycle length")
    k.add_argument("--pilot", type=float, default=700.0, help="frequency of the pilot tone (Hz)")
    k.add_argument("--tolerance", type=float, default=0.1, help="cycle lengths within this share of the nominal one are tried")
    k.add_argument("--tolerance-st", type=float, default=10, help="half width of the tracker's band (semitones)")
    k.add_argument("--fft", type=int, default=16384, help="FFT size")
    k.add_argument("--hop", type=int, default=None, help="hop (default: fft / 128)")
    k.add_argument("--channels", default="L", choices=("L", "R"), help="the channel the pilot is traced in")
    k.add_argument("--json", default=None, metavar="REPORT.json", help="write the figures (a list when several files are given)")
    k.add_argument("--resample", action="store_true", help="remove the measured cycle: <stem>_res.wav through the sinc resampler")
    k.add_argument("--quality", type=int, default=50, help="sinc_quality (NT) of --resample")
    u = sub.add_parser("flutter", help="zero-crossing flutter analysis: the pitch of a clean pilot tone from the spacing of its sign changes")
    u.add_argument("files", nargs="+")
    u.add_argument("--band", type=pair, default=None, help="LO,HI (Hz): band-pass around the pilot first (default: no filter)")
    u.add_argument("--order", type=int, default=3, help="order of the band-pass")
    u.add_argument("--hop", type=int, default=256, help="samples between the points of the regular pitch curve")
    u.add_argument("--channel", default="L", choices=("L", "R"), help="the channel the pilot is in")
    u.add_argument("--json", default=None, metavar="REPORT.json", help="write the figures (a list when several files are given)")
    u.add_argument("--resample", action="store_true", help="remove the measured flutter: <stem>_res.wav through the sinc resampler")
    u.add_argument("--quality", type=int, default=50, help="sinc_quality (NT) of --resample")
    x = sub.add_parser("maxmono", help="MaxMono dropout repair of a two-track transfer: per STFT bin the louder channel -> <stem>max.wav, "
                                       "the quieter -> <stem>min.wav")
    x.add_argument("files", nargs="+")
    x.add_argument("--fft", type=int, default=512, help="FFT size")
    x.add_argument("--overlap", type=int, default=4, help="hop = fft / overlap")
    g = sub.add_parser("groupdelay", help="group delay by bands: lag, correlation and level difference of two transfers per log-spaced band")
    g.add_argument("file", help="the reference transfer; without --ref its channel 0 is measured against its channel 1")
    g.add_argument("--ref", default=None, metavar="OTHER", help="the other transfer: channel 0 of FILE against channel 0 of OTHER")
    g.add_argument("--range", type=pair, default=None, metavar="T0,T1", help="span in seconds (default: the whole signal)")
    g.add_argument("--bands", type=pair, default=[10, 2000, 45], metavar="LO,HI,BW", help="log-spaced band edges from LO to HI Hz, (HI - LO) / BW of them")
    g.add_argument("--min-corr", type=float, default=0.6, help="bands at or below this correlation are dropped")
    g.add_argument("--json", default=None, metavar="OUT.json", help="write the per-band arrays")
    v = sub.add_parser("spectrogram", help="the spectrogram picture the coordinates of the other tools are read from: <stem>_spec.png + .json")
    v.add_argument("file")
    v.add_argument("--range", type=pair, default=None, metavar="T0,T1", help="span in seconds (default: the whole file)")
    v.add_argument("--freq", type=pair, default=None, metavar="F0,F1", help="band in Hz (default: 0 to sr / 2)")
    v.add_argument("--size", type=ints, default=[2048, 1024], metavar="W,H", help="pixels")
    v.add_argument("--fft", type=int, default=4096, help="FFT size")
    v.add_argument("--overlap", type=int, default=8, help="hop = fft / overlap")
    v.add_argument("--scale", default="mel", choices=("mel", "linear", "log"), help="frequency axis (log needs F0 > 0)")
    v.add_argument("--clim", type=pair, default=[-120.0, 0.0], metavar="LO,HI", help="colour limits in dB (write --clim=-90,-20: a leading minus needs the = form)")
    v.add_argument("--cmap", default="heat", help="gray, heat, or a matplotlib name where matplotlib is installed")
    v.add_argument("--channel", default="L", help="L, R or a channel number")
    v.add_argument("--out", default=None, metavar="PNG", help="default: <stem>_spec.png")
    v.add_argument("--at", type=pair, default=None, metavar="X,Y", help="print the (s, Hz) of this pixel and write nothing")
    return ap


def _spectrogram(args):
    from . import cyclic_wow, io_ops, spectrogram
    for name, val in (("--range", args.range), ("--freq", args.freq), ("--size", args.size), ("--clim", args.clim), ("--at", args.at)):
        if val is not None and len(val) != 2:
            raise SystemExit(f"{name} takes two values")
    t0, t1 = args.range if args.range is not None else (None, None)
    f0, f1 = args.freq if args.freq is not None else (None, None)
    signal, sr, ch = io_ops.read_file(args.file)
    channel = cyclic_wow.channel_index(args.channel if args.channel in ("L", "R") else int(args.channel), ch)
    kw = dict(width=args.size[0], height=args.size[1], fft_size=args.fft, overlap=args.overlap, t0=t0, t1=t1, f0=f0, f1=f1,
              scale=args.scale)
    if args.at is not None:
        geo = spectrogram.geometry(len(signal), sr, args.fft, max(1, args.fft // args.overlap), 1, args.size[0], args.size[1], t0, t1,
                                   f0, f1, args.scale)
        t, f = geo.to_time_freq(args.at[0], args.at[1])
        print(f"{t!r} {f!r}")
        return 0
    png, meta, geo = spectrogram.render_file(args.file, args.out, signal_data=(signal, sr), vmin=args.clim[0], vmax=args.clim[1],
                                             cmap=args.cmap, channel=channel, **kw)
    logging.info("wrote %s and %s: %d x %d pixels of %.6g .. %.6g s, %.6g .. %.6g Hz (%s)", png, meta, geo.width, geo.height, geo.t0,
                 geo.t1, geo.f0, geo.f1, geo.scale)
    return 0


def _groupdelay(args):
    from . import group_delay, io_ops
    if len(args.bands) != 3 or (args.range is not None and len(args.range) != 2):
        raise SystemExit("--bands takes LO,HI,BW and --range T0,T1")
    t0, t1 = args.range if args.range is not None else (None, None)
    sig, sr, ch = io_ops.read_file(args.file)
    if args.ref is None:
        if ch < 2:
            raise SystemExit(f"{args.file} has one channel: give the other transfer with --ref")
        ref, src = sig[:, 0], sig[:, 1]
    else:
        other, sr2, _ = io_ops.read_file(args.ref)
        if sr2 != sr:
            raise SystemExit(f"sample rates differ: {sr} and {sr2}")
        ref, src = sig[:, 0], other[:, 0]
    res = group_delay.measure(ref, src, sr, args.bands[0], args.bands[1], args.bands[2], t0, t1, args.min_corr, strict=False)
    for k in range(len(res.kept)):
        logging.info("band %2d  %5d .. %5d Hz  lag %+.6f samples  corr %.6f  levels %.6g / %.6g%s", k, int(res.band_lo[k]),
                     int(res.band_hi[k]), res.lags_all[k], res.correlations_all[k], res.levels_ref[k], res.levels_src[k],
                     "" if res.kept[k] else "  (dropped)")
    rep = dict(group_delay.report(res), file=args.file, ref=args.ref, sr=sr)
    logging.info("%d of %d bands kept", rep["n_kept"], rep["n_bands"])
    if args.json:
        with open(args.json, "w") as out:
            json.dump(rep, out, indent=1)
        logging.info("wrote %s", args.json)
    return 0


def _maxmono(args):
    from . import dropouts
    failed = 0
    for path in args.files:
        try:
            for p in dropouts.process(path, args.fft, args.overlap):
                logging.info("wrote %s", p)
        except Exception:                               # keep the other files going, as the GUI does
            logging.exception(f"{path} failed")
            failed += 1
    return 1 if failed else 0


def _difeq(args):
    from . import difeq
    if len(args.files) % 2 or len(args.rolloff) != 2:
        raise SystemExit("difeq takes SRC REF pairs, and --rolloff A,B")
    if not (20 <= args.resolution <= 2000 and 1 <= args.smoothing <= 200):
        raise SystemExit("--resolution is 20..2000 and --smoothing 1..200 (the GUI's spin boxes)")
    pairs = list(zip(args.files[0::2], args.files[1::2]))
    res = difeq.process(pairs, args.out, args.channels, highpass=args.highpass, rolloff_start=args.rolloff[0], rolloff_end=args.rolloff[1],
                        resolution=args.resolution, smoothing=args.smoothing, strength=args.strength, keep_gain=args.keep_gain)
    logging.info("%d pair(s), %d keys, gain %.9g dB", len(pairs), len(res["freqs_av"]), res["gain"])
    for p in res["paths"]:
        logging.info("wrote %s", p)
    return 0


def _cyclic(args):
    from . import cyclic_wow, io_ops, resampling
    reports = []
    for path in args.files:
        signal, sr, _ = io_ops.read_file(path)
        hop = cyclic_wow.default_hop(args.fft) if args.hop is None else args.hop
        res = cyclic_wow.analyse(signal, sr, args.rpm, args.pilot, args.tolerance, args.tolerance_st, args.fft, hop, args.channels)
        rep = dict(cyclic_wow.report(res), file=path, sr=sr, fft_size=args.fft, hop=hop)
        logging.info("%s: best cycle length %d frames of %d samples: %.9g s (nominal %.9g s), the record was playing at %.6f rpm", path,
                     rep["frames_per_rotation"], hop, rep["cycle_duration_s"], 60.0 / args.rpm, rep["rpm_measured"])
        logging.info("%s: depth of the cycle %.6g octaves = %.6g semitones peak to peak", path, rep["delta_octaves"], rep["delta_semitones"])
        if args.resample:
            resampling.run((path,), signal_data=((signal, sr),), speed_curve=cyclic_wow.speed_curve(res, sr, hop), resampling_mode="Sinc",
                           sinc_quality=args.quality)
            rep["resampled"] = f"{os.path.splitext(path)[0]}_res.wav"
            logging.info("wrote %s", rep["resampled"])
        reports.append(rep)
    if args.json:
        with open(args.json, "w") as out:
            json.dump(reports[0] if len(reports) == 1 else reports, out, indent=1)
        logging.info("wrote %s", args.json)
    return 0


def _flutter(args):
    from . import cyclic_wow, io_ops, resampling, zerocrossing_wow
    if args.band is not None and len(args.band) != 2:
        raise SystemExit("--band takes LO,HI")
    if args.hop < 1:
        raise SystemExit("--hop is at least 1")
    reports = []
    for path in args.files:
        signal, sr, ch = io_ops.read_file(path)
        res = zerocrossing_wow.detect_crossings(signal, sr, cyclic_wow.channel_index(args.channel, ch), args.band, args.order, args.hop)
        rep = dict(zerocrossing_wow.report(res), file=path, sr=sr, hop=args.hop, band=args.band)
        logging.info("%s: %d crossings, smoothing span %d; pilot at %.9g Hz, flutter %.6g %% peak to peak, %.6g %% RMS", path,
                     rep["crossings"], rep["span"], rep["mean_hz"], rep["peak_to_peak_percent"], rep["rms_percent"])
        if args.resample:
            resampling.run((path,), signal_data=((signal, sr),), speed_curve=zerocrossing_wow.speed_curve(res), resampling_mode="Sinc",
                           sinc_quality=args.quality)
            rep["resampled"] = f"{os.path.splitext(path)[0]}_res.wav"
            logging.info("wrote %s", rep["resampled"])
        reports.append(rep)
    if args.json:
        with open(args.json, "w") as out:
            json.dump(reports[0] if len(reports) == 1 else reports, out, indent=1)
        logging.info("wrote %s", args.json)
    return 0


def _pan(args):
    from . import pypan
    if any(len(b) != 4 for b in args.box):
        raise SystemExit("--box takes T0,F0,T1,F1")
    if args.file.lower().endswith(pypan.EXT):
        if args.box:
            raise SystemExit("--box measures an audio file; give the project to extend with --out")
        written, _ = pypan.process(project=args.file, keep_left=args.keep_left)
    else:
        if not args.box:
            raise SystemExit("nothing to do: give --box to measure, or a .pan project to apply")
        cfg = {"fft_size": args.fft, "fft_overlap": args.overlap, "fft_zeropad": args.zeropad, "source": args.file, "markers": []}
        if args.out and os.path.exists(args.out):
            cfg = json.load(open(args.out))
        written, markers = pypan.process(args.file, project=cfg, boxes=args.box, keep_left=args.keep_left, apply=args.apply)
        for m in markers[len(cfg.get("markers", ())):]:
            logging.info("%s: box %s .. %s: L/R = %.9g", args.file, m.a, m.b, m.pan)
        if args.out:
            pypan.save_project(args.out, dict(cfg, markers=markers))
            logging.info("wrote %s", args.out)
    if written:
        logging.info("wrote %s", written)
    return 0


def main(argv=None):
    args = parser().parse_args(argv)
    logging.basicConfig(level=logging.INFO, format="%(levelname)s %(message)s")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("no ROCm GPU visible; this tool has no CPU fallback")
    if args.cmd == "dynamics":                  # one pair of files, one GPU
        from . import decompressor
        logging.info("wrote %s", decompressor.process(args.src, args.ref))
        return 0
    if args.cmd == "azimuth":                   # one pair of files, one GPU
        from . import pipeline
        if len(args.box) != 4:
            raise SystemExit("--box takes T0,F0,T1,F1")
        pipeline.measure_azimuth(args.project, args.ref, args.src, args.box, args.win, args.overlap, args.reject, args.ignore_phase,
                                 args.out)
        if args.out:
            logging.info("wrote %s", args.out)
        return 0
    if args.cmd == "pan":                       # one file, one GPU
        return _pan(args)
    if args.cmd == "difeq":                     # pairs of files, one GPU
        return _difeq(args)
    if args.cmd == "cyclic":                    # file after file, one GPU
        return _cyclic(args)
    if args.cmd == "flutter":                   # file after file, one GPU
        return _flutter(args)
    if args.cmd == "maxmono":                   # file after file, one GPU
        return _maxmono(args)
    if args.cmd == "groupdelay":                # one pair of transfers, one GPU
        return _groupdelay(args)
    if args.cmd == "spectrogram":               # one file, one GPU
        return _spectrogram(args)
    n_gpu = torch.cuda.device_count() if args.gpus <= 0 else min(args.gpus, torch.cuda.device_count())
    jobs = queue.Queue()
    for f in sorted(args.files, key=lambda p: -os.path.getsize(p)):     # longest first
        jobs.put(f)
    results = []
    threads = [threading.Thread(target=_worker, args=(d, jobs, args, results)) for d in range(n_gpu)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    failed = [p for p, e in results if e is not None]
    logging.info(f"{len(results) - len(failed)} file(s) done on {n_gpu} GPU(s), {len(failed)} failed")
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
