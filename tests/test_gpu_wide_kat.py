"""Known-answer tests of the fp16 wide-OSNet kernels (ReID mode 1 at x1.0: boxmot_amd/csrc/osnet_wide_kernels.hpp), one kernel at a time
on the device: tests/kat/wide_kat.hip includes the header and osnet_wide_pack.hpp unchanged and launches each kernel as WideOsnet::forward
does; tests/wide_kat_common.py holds the inputs, the float64 references, the derived bounds, the wrong-reference controls and the poison /
guard / determinism / crop-independence checks.  exact and impulses are bit for bit, random is inside its worst-case bound.

  k_wide_stem<32 | 64>      262 x 136 x 4 input, {exact, impulses, random} x n in {1, 3}; impulses put conv maxima on conv rows 0, 1, 7, 8, 64,
                            126, 127 x columns 0, 1, 15, 16, 31, 32, 47, 48, 62, 63 (the real DPP row shifts at lanes 0 and 15)
  k_light_fused<C>          (C, H, W) = (64, 64, 32), (32, 64, 32), (96, 32, 16), (128, 32, 16), (128, 16, 8), (96, 16, 8), (32, 16, 8):
                            1 / 2 / 4 row groups, 64 idle threads at C = 96; three regimes x n in {1, 3}; gap_part given and null
  k_gate_sum4<C>            C in {32, 64, 96, 128} x (P, nbands) in {(128, 2), (512, 4), (136, 2)} x n in {1, 3}, {exact, random}; the gate
                            alone at pre-activations in [-8, 8] (measure_gate)
  k_wide_gap                C in {384, 512}, P = 128, n in {1, 3, 11}, {exact, random}
  k_wide_l2                 F in {128, 512}, n in {1, 4, 5, 9}, out_rows null and scattered into a poisoned table, {exact, random}

Measured on an MI355X by this file (every test prints its figures).  Largest error / bound of the random regime (below 1 by derivation;
the stem, the gate sum and the average pool sit near 1 because half an fp16 step of the output IS most of their bound):
  k_wide_stem<32>     0.949      k_light_fused<32>    0.571      k_gate_sum4<32>    0.980       k_wide_gap    0.966
  k_wide_stem<64>     0.959      k_light_fused<64>    0.623      k_gate_sum4<64>    0.977       k_wide_l2     0.016
  gap_part            0.022      k_light_fused<96>    0.659      k_gate_sum4<96>    0.936
  (against own sums)             k_light_fused<128>   0.764      k_gate_sum4<128>   0.909
The gate: largest |g - sigmoid64(v)| = 8.524e-08 over 768 pre-activations in [-8, 8] (the expected gate subtracted inside the kernel's sum,
so that the fp16 store does not hide it), allowance 4 x that = 3.410e-07, far below 2**-11 (wide_kat_common.MEASURED; the emulation's
own row is "emu").  Through out = fp16(g) alone the gate shows 2.439e-04, the fp16 rounding of g.
The whole file (27 tests) takes 3 s on the device, its 1.4 s build included; the five `fast` cases under a second."""
import pytest

import wide_kat_common as wk

pytestmark = pytest.mark.gpu

FAST = pytest.mark.fast


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return wk.WideKatLib(wk.build_gpu(tmp_path_factory.mktemp("wide_kat")), "gpu")


@pytest.mark.parametrize("regime", wk.REGIMES)
@pytest.mark.parametrize("c0", [32, 64])
def test_stem(lib, c0, regime):
    for n in (1, 3):
        wk.run_stem(lib, c0, regime, n, seed=10 + n)
    wk.report("gpu")


@pytest.mark.parametrize("case", wk.LIGHT_CASES, ids=lambda c: "C%d-%dx%d" % c)
def test_light(lib, case):
    for regime in wk.REGIMES:
        for n in (1, 3):
            wk.run_light(lib, case, regime, n, seed=20 + n)
    wk.report("gpu")


def test_gate_measured(lib):
    """the gate's own error through __expf, below the resolution of an fp16 output: see wide_kat_common.measure_gate"""
    for n in (1, 3):
        wk.measure_gate(lib, n)


@pytest.mark.parametrize("C", [32, 64, 96, 128])
def test_gate(lib, C):
    for regime in ("exact", "random"):
        for P, nbands in ((128, 2), (512, 4), (136, 2)):
            for n in (1, 3):
                wk.run_gate(lib, C, P, nbands, regime, n, seed=30 + n)
    wk.report("gpu")


@pytest.mark.parametrize("C", [384, 512])
def test_gap(lib, C):
    for regime in ("exact", "random"):
        for n in (1, 3, 11):
            wk.run_gap(lib, C, 128, regime, n, seed=40 + n)
    wk.report("gpu")


@pytest.mark.parametrize("F", [128, 512])
def test_l2(lib, F):
    for regime in ("exact", "random"):
        for n in (1, 4, 5, 9):
            for scatter in (False, True):
                wk.run_l2(lib, F, regime, n, scatter, seed=50 + n)
    wk.report("gpu")


@pytest.mark.parametrize("kernel", [pytest.param(k, marks=FAST) for k in ("stem", "light", "gate", "gap", "l2")])
def test_one_small_case_per_kernel(lib, kernel):
    if kernel == "stem":
        wk.run_stem(lib, 32, "impulses", 1, seed=1)
    elif kernel == "light":
        wk.run_light(lib, (32, 16, 8), "impulses", 3, seed=2)
    elif kernel == "gate":
        wk.run_gate(lib, 32, 136, 2, "random", 1, seed=3)
    elif kernel == "gap":
        wk.run_gap(lib, 384, 128, "exact", 3, seed=4)
    else:
        wk.run_l2(lib, 128, "random", 5, True, seed=5)
