"""Times of the ORIENTED ReID front end beside the axis-aligned one it mirrors, by HIP events: 64 streams x 64 crops, 1080p frames,
OSNet-x0.25 in mode 2 by default; 5 warm-up and 30 timed runs of each side, alternating, every run with its own event pair;
median, min and max.  Three pairs: the crop-list kernels (axis-aligned on the enclosing boxes | oriented, which also makes the crop
geometry), the (hi, lo) crop kernels (k_crop_resize_rgbx_hl on the enclosing boxes | k_crop_resize_obb_rgbx_hl), and the whole ReID
launch set of a counted pass (axis-aligned with the crop fused into the stem, as shipped, and with the separate crop kernel |
oriented).  The measuring program is tools/obb_reid_prof.hip (it includes the kernels' headers as the library does); this script
builds it when it is older than its sources and runs it.  Figures side by side, nothing gated.

    python tools/obb_reid_prof.py [--streams 64] [--crops 64] [--rows 1080] [--cols 1920] [--repeats 30] [--build-only]

Needs a gfx950 device.  profiles/obb_reid_timing.txt is the output of one such run."""
import argparse
import os
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
SRC = ROOT / "tools" / "obb_reid_prof.hip"
EXE = ROOT / "tools" / "_build" / "obb_reid_prof"
CSRC = ROOT / "boxmot_amd" / "csrc"
DEPS = [SRC] + sorted(CSRC.glob("*.hpp"))


def build() -> Path:
    if not EXE.exists() or any(d.stat().st_mtime > EXE.stat().st_mtime for d in DEPS):
        EXE.parent.mkdir(parents=True, exist_ok=True)
        subprocess.check_call([os.environ.get("HIPCC", "hipcc"), "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-o", str(EXE), str(SRC)])
    return EXE


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--streams", type=int, default=64)
    ap.add_argument("--crops", type=int, default=64, help="crops per stream (streams x crops <= 4096)")
    ap.add_argument("--rows", type=int, default=1080)
    ap.add_argument("--cols", type=int, default=1920)
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--build-only", action="store_true", help="compile the measuring program and stop (no device needed)")
    a = ap.parse_args()
    exe = build()
    if a.build_only:
        return 0
    return subprocess.call([str(exe), str(a.streams), str(a.crops), str(a.rows), str(a.cols), str(a.repeats)])


if __name__ == "__main__":
    sys.exit(main())
