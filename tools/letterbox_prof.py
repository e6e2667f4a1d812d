"""Time of the ingest ring's letterbox kernel beside the NV12 -> BGR kernel of the same slot, by HIP events: 64 streams of 1080p into
640 x 640 fp16 by default, 5 warm-up and 30 timed launches of each kernel, alternating, every launch with its own event pair; median,
min and max.  The measuring program is tools/letterbox_prof.hip (it includes the two kernels' headers as the library does); this
script builds it when it is older than its sources and runs it, for the default and for any further (H, W, dtype) asked for.

    python tools/letterbox_prof.py [--streams 64] [--rows 1080] [--cols 1920] [--size 640 640] [--fp32] [--mode center] [--repeats 30]

Needs a gfx950 device.  profiles/letterbox_timing.txt is the output of one such run."""
import argparse
import os
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
SRC = ROOT / "tools" / "letterbox_prof.hip"
EXE = ROOT / "tools" / "_build" / "letterbox_prof"
CSRC = ROOT / "boxmot_amd" / "csrc"
DEPS = [SRC] + [CSRC / n for n in ("ingest_letterbox.hpp", "ingest_nv12.hpp", "reid_kernels_v1.hpp", "reid_layout.hpp", "kernel_macros.hpp")]


def build() -> Path:
    if not EXE.exists() or any(d.stat().st_mtime > EXE.stat().st_mtime for d in DEPS):
        EXE.parent.mkdir(parents=True, exist_ok=True)
        subprocess.check_call([os.environ.get("HIPCC", "hipcc"), "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-o", str(EXE), str(SRC)])
    return EXE


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--streams", type=int, default=64)
    ap.add_argument("--rows", type=int, default=1080)
    ap.add_argument("--cols", type=int, default=1920)
    ap.add_argument("--size", type=int, nargs=2, default=(640, 640), metavar=("H", "W"))
    ap.add_argument("--fp32", action="store_true")
    ap.add_argument("--mode", choices=("center", "topleft"), default="center")
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--build-only", action="store_true", help="compile the measuring program and stop (no device needed)")
    a = ap.parse_args()
    exe = build()
    if a.build_only:
        return 0
    return subprocess.call([str(exe), str(a.streams), str(a.rows), str(a.cols), str(a.size[0]), str(a.size[1]), "0" if a.fp32 else "1",
                            str(a.repeats), "0" if a.mode == "center" else "1"])


if __name__ == "__main__":
    sys.exit(main())
