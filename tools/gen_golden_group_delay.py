"""Fixture of the group-delay measurement, computed by the REFERENCE's own function (build container only).

    python tools/gen_golden_group_delay.py --ref /path/to/pyaudiorestoration

experiments/group_delay.py is a script: its top level reads files from a fixed folder and writes others.  This tool therefore
reads the script at run time, keeps its imports and its `def`s and compiles only those (matplotlib and soundfile are stand-ins,
oracle/ref_gui.py's import hook), swaps `plot_corr_lag` for a recorder and calls get_group_delay(ref, src) unchanged on the
seeded pair of tests/group_delay_np.fixture_signals: n = 65 659 samples at 44.1 kHz, `ref` float32 white noise, `src` the same
through a first-order Bessel low-pass at 300 Hz, rolled by 7 samples, plus a small noise that grows along the file.  Nothing of
the script is copied; only arrays it computed are stored.

tests/golden/group_delay.npz:

  ref, src (float32), sr
  band_limits                           the script's np.logspace(..., dtype=np.uint16), recomputed here as it writes it
  band_centers, correlations, lags, magnitudes     the four lists it hands to plot_corr_lag (the kept bands)

Deterministic: running it twice writes identical files."""
import argparse
import ast
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import group_delay_np as G  # noqa: E402
from gen_golden_expander import save  # noqa: E402
from oracle import ref_gui  # noqa: E402


def load_defs(path):
    """the script's namespace with only its imports and function definitions executed"""
    tree = ast.parse(open(path).read(), filename=path)
    tree.body = [node for node in tree.body if isinstance(node, (ast.Import, ast.ImportFrom, ast.FunctionDef))]
    ns = {"__name__": "group_delay_defs"}
    exec(compile(tree, path, "exec"), ns)
    return ns


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="checkout of the reference (pyaudiorestoration)")
    a = ap.parse_args()
    ref_gui.import_reference_gui(a.ref)
    ns = load_defs(os.path.join(a.ref, "experiments", "group_delay.py"))
    recorded = []
    ns["plot_corr_lag"] = lambda *lists: recorded.append([np.array(v, dtype=np.float64) for v in lists])
    ref, src = G.fixture_signals()
    with np.errstate(all="ignore"):
        ns["get_group_delay"](ref, src)
    assert len(recorded) == 1 and len(recorded[0]) == 4
    centers, corrs, lags, mags = recorded[0]
    num_bands = int((2000 - 10) / 45)
    edges = np.logspace(np.log2(10), np.log2(2000), num=num_bands, endpoint=True, base=2, dtype=np.uint16)
    print(f"{len(edges) - 1} bands, {len(centers)} kept; lowest correlation kept {corrs.min():.4f}")
    save("group_delay", ref=ref, src=src, sr=np.array(G.SR), band_limits=edges, band_centers=centers, correlations=corrs, lags=lags,
         magnitudes=mags)


if __name__ == "__main__":
    main()
