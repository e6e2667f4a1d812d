"""A/B of compile-time kernel variants on the device (development tool).

Builds `libboxmot_hip` once per variant into tools/_build/ (run this part in the build container -- hipcc cross-compiles),
then, on the GPU box, runs the ReID parity tests and `bench.py --no-cpu-baseline` against each and prints one line per
variant.  What remains selectable in the fp16 OSNet-x0.25 family is the shipped build (`base`) and the stage-1 EMIT / RECON
hand-over (`s1_handover`, BM_STAGE1_HANDOVER in reid_fused.hpp); the other round-2 / round-3 variants were measured, left at
their shipped values and removed from the source (profiles/README.md, profiles/fp16_switch_prune_isa.txt):

    python tools/ab_variants.py build                      # in the build container
    python tools/ab_variants.py run                        # on the GPU box
"""
import json
import os
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
OUT = ROOT / "tools" / "_build"
VARIANTS = {
    "base": [],
    "s1_handover": ["-DBM_STAGE1_HANDOVER=1"],        # stage 1 as an EMIT / RECON block pair, like stage 0
}


def build():
    sys.path.insert(0, str(ROOT))
    import __graft_entry__ as g
    OUT.mkdir(parents=True, exist_ok=True)
    for name, flags in VARIANTS.items():
        lib = OUT / f"libboxmot_hip_{name}.so"
        cmd = [os.environ.get("HIPCC", "hipcc"), *g.HIPCC_FLAGS, *flags, "-o", str(lib), str(g.CSRC / "boxmot_hip.hip")]
        print(" ".join(cmd), flush=True)
        subprocess.check_call(cmd)


def run(with_tests: bool = False, rounds: int = 1, only=None):
    """Interleaved rounds (variant order repeated) so that clock / thermal drift does not read as a kernel property."""
    results = {name: [] for name in VARIANTS}
    parity = {}
    for r in range(rounds):
        for name in VARIANTS:
            lib = OUT / f"libboxmot_hip_{name}.so"
            if not lib.exists() or (only and name not in only):
                continue
            env = dict(os.environ, BOXMOT_HIP_LIB=str(lib))
            if with_tests and r == 0:
                t = subprocess.run([sys.executable, "-m", "pytest", "tests/test_gpu_reid.py", "-x", "-q"], cwd=ROOT, env=env,
                                   capture_output=True, text=True)
                parity[name] = t.returncode == 0
            b = subprocess.run([sys.executable, "bench.py", "--no-cpu-baseline", "--steps", "30", "--warmup", "8"], cwd=ROOT, env=env,
                               capture_output=True, text=True)
            line = b.stdout.strip().splitlines()[-1] if b.stdout.strip() else "{}"
            try:
                d = json.loads(line)
                results[name].append((d["value"], d["roofline"]["launch_ms"], d.get("parity_ids_exact_vs_oracle_stream0"),
                                      d.get("reid_max_abs_err_vs_fp32_oracle")))
            except Exception:
                print(f"{name:12s} bench failed: {b.stderr[-300:]}", flush=True)
    for name, rs in results.items():
        if not rs:
            print(f"{name}: not built / no result")
            continue
        fps = " ".join(f"{v:.0f}" for v, _, _, _ in rs)
        ms = " ".join(f"{m:.3f}" for _, m, _, _ in rs)
        print(f"{name:12s} frames/s [{fps}]  reid_launch_ms [{ms}]  ids_exact={rs[0][2]} emb_err={rs[0][3]}"
              + (f" reid_tests={'ok' if parity.get(name) else 'FAIL'}" if name in parity else ""), flush=True)


if __name__ == "__main__":
    {"build": build, "run": lambda: run(only=sys.argv[2:] or None), "run_tests": lambda: run(True)}[sys.argv[1] if len(sys.argv) > 1 else "run"]()
