"""The fp16 wide-OSNet known-answer harness (tests/kat/wide_kat.hip: osnet_wide_kernels.hpp and osnet_wide_pack.hpp unchanged) on CPU
threads: the emulated MFMA and row shifts of tests/host_emu/hip_shim.hpp.  Cases, float64 references, derived bounds, wrong-reference
controls and the checks around a launch are tests/wide_kat_common.py's; the device runs the full list (tests/test_gpu_wide_kat.py).
Device-only, to keep this file to half a minute: the stem at n = 3 in the exact and random regimes (its impulses run at n = 3 here
too); every other case of the device list runs here as well.  The emulation's row shifts are emu_row_shift, not the DPP instruction,
and its exponential is libm's: the device test is the one that proves lanes 0 and 15 and __expf.  Not a product path."""
import shutil

import pytest

import wide_kat_common as wk

CLANG = shutil.which("clang++", path="/opt/rocm/lib/llvm/bin") or shutil.which("clang++")
pytestmark = pytest.mark.skipif(CLANG is None, reason="needs a host clang with _Float16")


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return wk.WideKatLib(wk.build_emu(CLANG, tmp_path_factory.mktemp("wide_kat_emu")), "emu")


def test_impulse_sheets_cover_every_wanted_position():
    """the impulse regime's n = 3 and n = 1 runs together hold every wanted row, column and channel"""
    sheets = wk.stem_sheets()
    assert {p for s in sheets for p in s} == {(cy, cx) for cy in wk.STEM_ROWS for cx in wk.STEM_COLS} and all(sheets)
    for C, H, W in wk.LIGHT_CASES:
        got = [p for s in wk.light_sheets(C, H, W) for p in s]
        assert {0, 7, 8, H - 1} <= {p[0] for p in got} and {0, W - 1} <= {p[1] for p in got} and {0, 7, 8, C - 1} <= {p[2] for p in got}
        rpg = 8 // wk.light_groups(C, W)
        assert all({g * rpg - 1, g * rpg} <= {p[0] for p in got} for g in range(1, 8 // rpg))
    assert [wk.light_groups(C, W) for C, H, W in wk.LIGHT_CASES] == [1, 2, 1, 1, 2, 2, 4]


def test_controls_are_rejected():
    res = wk.controls()
    for name in ("light halo rows zeroed", "light columns wrapped", "stem tile-left neighbour dropped", "gate branches swapped",
                 "gate mean over nbands"):
        assert res[name] > 0, f"the band does not reject the wrong reference: {name}"
    # rounding to fp16 commutes with ReLU and max: "conv, then ReLU on fp16" is the same function, which no band can reject
    assert res["stem relu on fp16"] == 0
    print("light intermediate not rounded to fp16, elements rejected per regime:", res["light unrounded"])


@pytest.mark.parametrize("c0", [32, 64])
def test_stem_emulated(lib, c0):
    for regime in wk.REGIMES:
        wk.run_stem(lib, c0, regime, 1, seed=1)
    wk.run_stem(lib, c0, "impulses", 3, seed=2)
    wk.report("emu")


@pytest.mark.parametrize("case", wk.LIGHT_CASES, ids=lambda c: "C%d-%dx%d" % c)
def test_light_emulated(lib, case):
    for regime in wk.REGIMES:
        for n in (1, 3):
            wk.run_light(lib, case, regime, n, seed=3 + n)
    wk.report("emu")


def test_gate_measured_emulated(lib):
    for n in (1, 3):
        wk.measure_gate(lib, n)


@pytest.mark.parametrize("C", [32, 64, 96, 128])
def test_gate_emulated(lib, C):
    for regime in ("exact", "random"):
        for P, nbands in ((128, 2), (512, 4), (136, 2)):
            for n in (1, 3):
                wk.run_gate(lib, C, P, nbands, regime, n, seed=5 + n)
    wk.report("emu")


def test_gap_and_l2_emulated(lib):
    for regime in ("exact", "random"):
        for C in (384, 512):
            for n in (1, 3, 11):
                wk.run_gap(lib, C, 128, regime, n, seed=n)
        for F in (128, 512):
            for n in (1, 4, 5, 9):
                for scatter in (False, True):
                    wk.run_l2(lib, F, regime, n, scatter, seed=n)
    wk.report("emu")
