"""Builds libpar_hip.so in-tree with hipcc for gfx950 (cross-compiles without a GPU).

Each csrc/*.hip is compiled to an object with per-file flags, then linked.  pos.hip (float64
positions that must be bit-identical to numpy), resample_fixed.hip (float64 positions and table offsets likewise), expander.hip and dynamics.hip (numpy's interpolation, compensated sums) and hpss.hip (numpy's
float32 soft mask) are built with -ffp-contract=off; the other kernels
keep hipcc's default contraction and spell their FMAs explicitly (gauge.hip among them: every tap is an fmaf)."""
import glob
import os
import subprocess
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
OBJ = os.path.join(CSRC, "obj")
OUT = os.path.join(HERE, "libpar_hip.so")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC"]
PER_FILE = {"pos.hip": ["-ffp-contract=off"],
            "lag.hip": ["-ffp-contract=off"],
            "expander.hip": ["-ffp-contract=off"],
            "hpss.hip": ["-ffp-contract=off"],
            "resample_fixed.hip": ["-ffp-contract=off"],
            "dynamics.hip": ["-ffp-contract=off"],    # numpy's overlap-add and interpolation, rounding by rounding
            "pan.hip": ["-ffp-contract=off"],         # np.interp once more (np_interp.h)
            "crossings.hip": ["-ffp-contract=off"],   # np.interp a fourth time; the smoothing sum's products and adds rounded apart
            # SLP packing into v_pk_*_f32 buys no throughput on gfx950 and costs v_mov shuffles
            "sinc.hip": ["-fno-slp-vectorize"],
            "sinc2.hip": ["-fno-slp-vectorize"],
            "gauge.hip": ["-fno-slp-vectorize"],      # K_gauge's tap loop is 256 v_fma per 16 taps; packed, half of them plus v_mov shuffles
            "stft.hip": ["-fno-slp-vectorize"]}


def sources():
    return sorted(glob.glob(os.path.join(CSRC, "*.hip")))


def _headers():
    return glob.glob(os.path.join(CSRC, "*.h")) + glob.glob(os.path.join(HERE, "..", "include", "*.h"))


def source_digest():
    """sha256 (first 16 hex digits) over the kernel sources and headers: stamps the committed PMC summaries
    (tools/summarise_profiles.py) so that bench.py can tell whether they were measured on the code that is running."""
    import hashlib
    h = hashlib.sha256()
    for path in sorted(sources() + glob.glob(os.path.join(CSRC, "*.h"))):
        h.update(os.path.basename(path).encode())
        h.update(open(path, "rb").read())
    return h.hexdigest()[:16]


def _newer(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def build(force=False, verbose=False):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    os.makedirs(OBJ, exist_ok=True)
    hdrs = _headers() + [os.path.abspath(__file__)]
    jobs = []
    objs = []
    for src in sources():
        obj = os.path.join(OBJ, os.path.basename(src)[:-4] + ".o")
        objs.append(obj)
        if force or _newer(obj, [src] + hdrs):
            jobs.append([hipcc] + FLAGS + PER_FILE.get(os.path.basename(src), []) + ["-c", src, "-o", obj])

    def run(cmd):
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.check_call(cmd)
    with ThreadPoolExecutor(max_workers=min(8, max(1, len(jobs)))) as ex:
        list(ex.map(run, jobs))
    if force or jobs or _newer(OUT, objs):
        run([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC"] + objs + ["-o", OUT])
    return OUT


if __name__ == "__main__":
    build(force=True, verbose=True)
