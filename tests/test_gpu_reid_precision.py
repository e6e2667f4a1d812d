"""fp32-grade bands for the ReID families that claim fp32-grade arithmetic: mode 2 (fused kernels on fp16 (hi, lo) operand pairs) and
mode 0 (per-layer fp32 kernels), measured against a float64 oracle (oracle.osnet.osnet_forward on the state dict and the oracle's crops,
both as float64, L2-normalised in float64) instead of the fp32 oracle's 1e-3 north-star bar (which the fp16 family, mode 1, also meets
on the reference initialisation -- so that bar alone cannot tell fp32-grade arithmetic from fp16 arithmetic in one layer).

Per architecture and weight set (the reference initialisation, BatchNorm-calibrated seeds 0-2): one crop, and fourteen crops over
max_crops = 8 (two chunks) holding the odd boxes of the other ReID tests (empty, clipped at two borders, identity-sized, 2x).
Asserted: max|got - ref64| < BAND for every fp32-grade family, and mode 1 on the same inputs exceeds SEPARATION x that band -- the band
separates fp32-grade arithmetic from fp16 arithmetic.  The fp32 oracle's 1e-3 assertions of test_gpu_reid.py / test_gpu_long_parity.py
stay as they are."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# Bands per (architecture, mode, weights: "init" = the reference initialisation, "calib" = BatchNorm-calibrated seeds 0-2), about 4-5x the
# largest error measured on an MI355X (max over the weight sets of one kind, one and fourteen crops).  Two constants per family: on the
# reference initialisation mode 1 itself is only ~1.2e-4 from the float64 oracle, so a single band sized for the calibrated networks
# (~5e-6 measured) could not sit 10x below it.
#                                   measured           band      mode 1 (fp16) on the same inputs, smallest
#   x0.25 mode 2   init / calib     3.70e-7 / 5.24e-6  1.5e-6 / 2.5e-5    1.21e-4 / 8.27e-3
#   x0.25 mode 0   init / calib     9.59e-8 / 3.22e-6  4e-7 / 1.5e-5      1.21e-4 / 8.27e-3
#   x1.0  mode 2   init / calib     4.03e-7 / 3.93e-6  2e-6 / 1.8e-5      1.32e-4 / 2.19e-3
#   x1.0  mode 0   init / calib     1.81e-7 / 3.29e-6  8e-7 / 1.5e-5      1.32e-4 / 2.19e-3
#   x0.5  mode 2   init / calib     3.45e-7 / 4.22e-6  1.5e-6 / 2e-5      1.25e-4 / 4.99e-3
#   x0.75 mode 2   init / calib     3.12e-7 / 6.94e-6  1.5e-6 / 3e-5      1.37e-4 / 3.66e-3
BAND = {
    ("osnet_x0_25", 2, "init"): 1.5e-6, ("osnet_x0_25", 2, "calib"): 2.5e-5,
    ("osnet_x0_25", 0, "init"): 4e-7, ("osnet_x0_25", 0, "calib"): 1.5e-5,
    ("osnet_x1_0", 2, "init"): 2e-6, ("osnet_x1_0", 2, "calib"): 1.8e-5,
    ("osnet_x1_0", 0, "init"): 8e-7, ("osnet_x1_0", 0, "calib"): 1.5e-5,
    ("osnet_x0_5", 2, "init"): 1.5e-6, ("osnet_x0_5", 2, "calib"): 2e-5,
    ("osnet_x0_75", 2, "init"): 1.5e-6, ("osnet_x0_75", 2, "calib"): 3e-5,
}
SEPARATION = 10.0          # mode 1's error on the same inputs is at least this many bands
ODD_BOXES = np.array([[100, 100, 100, 150],          # empty (zero width): a blank crop
                      [-10, -5, 60, 120],           # clipped at the top-left corner
                      [1200, 650, 1300, 740],       # clipped at the bottom-right corner
                      [300, 200, 428, 456]],        # identity-sized: 128 x 256, no resampling
                     dtype=np.float32)


def _inputs():
    rng = np.random.default_rng(23)
    img = rng.integers(0, 255, (720, 1280, 3), dtype=np.uint8)
    b = np.stack([rng.uniform(0, 1100, 9), rng.uniform(0, 450, 9), np.zeros(9), np.zeros(9)], 1).astype(np.float32)
    b[:, 2] = b[:, 0] + rng.uniform(20, 160, 9)
    b[:, 3] = b[:, 1] + rng.uniform(40, 240, 9)
    big = np.array([[500, 100, 756, 612]], dtype=np.float32)                 # 2x: 256 x 512
    return img, np.concatenate([b, ODD_BOXES, big])


def _ref64(sd, boxes, img):
    import torch

    from oracle.crops import get_crops
    from oracle.osnet import osnet_forward
    sd64 = {k: (v.detach().to(torch.float64) if v.is_floating_point() else v) for k, v in sd.items()}
    x = torch.from_numpy(get_crops(boxes, img)).to(torch.float64)
    with torch.no_grad():
        f = osnet_forward(sd64, x).numpy()
    return f / np.linalg.norm(f, axis=1, keepdims=True)


def _weights(arch):
    from boxmot_amd.reid_weights import random_osnet_state_dict, reference_init_state_dict
    yield "init", "init", reference_init_state_dict(arch, seed=0)
    for seed in (0, 1, 2):
        yield "calib", f"calib seed {seed}", random_osnet_state_dict(arch, seed=seed)


@pytest.mark.parametrize("arch,modes", [pytest.param("osnet_x0_25", (2, 0), marks=pytest.mark.fast), ("osnet_x1_0", (2, 0)),
                                        ("osnet_x0_5", (2,)), ("osnet_x0_75", (2,))])
def test_fp32_grade_families_inside_their_band_and_fp16_outside(arch, modes):
    from boxmot_amd.reid import HipReID
    img, boxes = _inputs()
    assert len(boxes) == 14
    worst, lines, failures = {}, [], []
    for kind, name, sd in _weights(arch):
        ref = _ref64(sd, boxes, img)
        reid = HipReID(sd, max_crops=8)
        errs = {}
        for mode in (*modes, 1):
            reid.set_mode(mode)
            got = reid.get_features(boxes, img)                 # 14 crops: two chunks
            one = reid.get_features(boxes[:1], img)             # one crop
            assert np.all(np.isfinite(got)) and np.all(np.isfinite(one))
            errs[mode] = max(float(np.abs(got - ref).max()), float(np.abs(one - ref[:1]).max()))
        reid.close()
        lines.append(f"{arch} {name}: " + ", ".join(f"mode {m} {e:.2e}" for m, e in errs.items()))
        for mode in modes:
            band = BAND[(arch, mode, kind)]
            worst[(mode, kind)] = max(worst.get((mode, kind), 0.0), errs[mode])
            worst[(1, kind)] = min(worst.get((1, kind), np.inf), errs[1])
            if not errs[mode] < band:
                failures.append(f"{arch} {name} mode {mode}: max|got - ref64| = {errs[mode]:.3e} >= band {band:.1e}")
            if not errs[1] > SEPARATION * band:
                failures.append(f"{arch} {name}: mode 1 (fp16) error {errs[1]:.3e} is not above {SEPARATION:g} x the mode-{mode} band "
                                f"{band:.1e}: the band does not separate fp32-grade from fp16 arithmetic")
    for (mode, kind), e in sorted(worst.items()):
        if mode != 1:
            lines.append(f"{arch} mode {mode} [{kind}]: measured {e:.2e}, band {BAND[(arch, mode, kind)]:.1e}, "
                         f"mode 1 (fp16) smallest error {worst[(1, kind)]:.2e}")
    print("\n".join(lines))
    assert not failures, "\n".join(failures)
