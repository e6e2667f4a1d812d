"""Times of the detection post-processing kernels beside the host path they replace: A = 8400 anchors, 80 classes, fp16, "cn", for
1 / 16 / 64 streams at two pass rates (about 1 % of the anchors over the threshold -- a quiet scene -- and about 30 %, more than
max_candidates = 1024, so the exact top-K works).  The measuring program is tools/detpost_prof.hip: HIP events around each kernel of
the library's own sequence, 5 warm-up and 30 timed calls, and the device-to-host copy of the same tensor.  This script makes the
tensor (tests/detpost_ref.py random_pred, one stream, copied to every stream), runs the program, checks its checksum against the NumPy
reference's rows, and times that reference on this host: the host path is the copy plus S times the reference of one stream.

    python tools/detpost_prof.py [--streams 1 16 64] [--rates 0.01 0.3] [--repeats 30] [--out DIR]

Needs a gfx950 device.  profiles/detpost_timing.txt is the output of one such run."""
import argparse
import os
import subprocess
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
SRC = ROOT / "tools" / "detpost_prof.hip"
EXE = ROOT / "tools" / "_build" / "detpost_prof"
CSRC = ROOT / "boxmot_amd" / "csrc"
DEPS = [SRC, CSRC / "det_post.hpp", CSRC / "kernel_macros.hpp"]
sys.path[:0] = [str(ROOT / "tests"), str(ROOT)]          # the reference lives with the tests


def build() -> Path:
    if not EXE.exists() or any(d.stat().st_mtime > EXE.stat().st_mtime for d in DEPS):
        EXE.parent.mkdir(parents=True, exist_ok=True)
        subprocess.check_call([os.environ.get("HIPCC", "hipcc"), "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-o", str(EXE), str(SRC)])
    return EXE


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--streams", type=int, nargs="+", default=[1, 16, 64])
    ap.add_argument("--rates", type=float, nargs="+", default=[0.01, 0.3])
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--out", default=None, help="directory for the tensor files (default: a temporary one)")
    ap.add_argument("--build-only", action="store_true", help="compile the measuring program and stop (no device needed)")
    a = ap.parse_args()
    exe = build()
    if a.build_only:
        return 0
    import detpost_ref as ref
    A, nc, K, max_det = 8400, 80, 1024, 256
    geo = ref.GEO_CENTER
    out = Path(a.out) if a.out else Path(tempfile.mkdtemp())
    out.mkdir(parents=True, exist_ok=True)
    for rate in a.rates:
        pred = ref.random_pred(A, nc, "cn", np.float16, 1, rate, n_obj=60)
        path = out / f"detpost_pred_{rate}.bin"
        pred.tofile(path)
        times = []
        for _ in range(5):
            t0 = time.perf_counter()
            rows, counters = ref.detpost(pred, geo, "cn", 0.25, 0.45, max_det, K)
            times.append(time.perf_counter() - t0)
        want = f"checksum: rows {len(rows)} counters {counters[0]} {counters[1]} {counters[2]} sum {float(rows.astype(np.float64).sum()):.6f}"
        print(f"== pass rate {rate}: {counters[0]} of {A} anchors pass, {counters[1]} candidates, {counters[2]} kept by NMS, {len(rows)} rows", flush=True)
        print(f"NumPy reference of ONE stream on this host (tests/detpost_ref.py): median {1e3 * sorted(times)[2]:.2f} ms of 5", flush=True)
        for S in a.streams:
            r = subprocess.run([str(exe), str(path), str(S), str(A), str(nc), "0", "1", str(K), str(max_det), str(a.repeats)], capture_output=True, text=True,
                               timeout=300)
            print(r.stdout, end="", flush=True)
            if r.returncode != 0:
                print(r.stderr, file=sys.stderr)
                return r.returncode
            got = [ln for ln in r.stdout.splitlines() if ln.startswith("checksum:")][0]
            if got != want:
                print(f"CHECKSUM MISMATCH: device `{got}`, reference `{want}`", file=sys.stderr)
                return 1
            print("checksum equals the reference's", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
