"""The fp32-grade OSNet-x0.25 known-answer harness (tests/kat/reid_hp_kat.hip, the device source of boxmot_amd/csrc/reid_hp.hpp unchanged)
on CPU threads: the emulated MFMA, DPP and asynchronous global -> LDS copies of tests/host_emu/hip_shim.hpp.  The units, references,
bands, wrong-reference controls and checks around a launch of tests/reid_hp_kat_common.py on a reduced case list (one calibrated and
the initial weight set, n = 1 for the large units, the count / independence protocol once per kernel shape); the device runs the full
list (tests/test_gpu_reid_hp_kat.py).  The emulation's MFMA operand layout is the author's model of the hardware and CPU threads cannot
show a hazard between the matrix pipe and the vector unit: this proves the index arithmetic, the packing, the guards and the bands' bite
against that model, the device test proves them on gfx950.  Not a product path."""
import shutil

import numpy as np
import pytest
import torch

import reid_hp_kat_common as rk

CLANG = shutil.which("clang++", path="/opt/rocm/lib/llvm/bin") or shutil.which("clang++")
pytestmark = pytest.mark.skipif(CLANG is None, reason="needs a host clang with _Float16")


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return rk.ReidHpKatLib(rk.build_emu(CLANG, tmp_path_factory.mktemp("reid_hp_kat_emu")), "emu")


def test_layout_and_reference_restatements():
    """The numpy L-layout round-trips and is the identity at 16 channels; osblock64 with nothing wrong IS oracle.osnet._osblock (bit for
    bit, on the float64 state dict); (e) -- a max pool padded with 0 instead of -inf -- is identical on post-ReLU values."""
    from oracle.osnet import _osblock
    assert np.array_equal(rk.l_position(16), np.arange(16))
    assert sorted(rk.l_position(96)) == list(range(96)) and rk.l_position(96)[16] == 4 and rk.l_position(96)[4] == 24
    v = np.random.default_rng(0).standard_normal((2, 8, 96)).astype(np.float32)
    h, l, v64 = rk.pack_hl(v)
    assert np.array_equal(rk.unpack_hl(h, l, 96), v64) and np.abs(v64 - v).max() <= 2.0 ** -22 * np.abs(v).max()
    sd = rk.weights("calib0")[0]
    x = torch.from_numpy(np.abs(np.random.default_rng(1).standard_normal((1, 96, 16, 8))))
    with torch.no_grad():
        assert torch.equal(rk.osblock64(sd, "conv4.0", x)[1], _osblock(sd, "conv4.0", x))


def test_crop_kernel_emulated(lib):
    """the whole box list at frame width 641 (general, clipped, empty, identity-sized, whole frame), count protocol included"""
    rel, beyond, _ = rk.run_crop(lib, rk.BOXES)
    print(f"emulated k_crop_resize_rgbx_hl: max |hi + lo - f| / |f| = {rel:.3e}; {beyond} elements beyond 2**-22 |f| (lo subnormal: 2**-25 absolute)")


@pytest.mark.parametrize("kind", ["init", "calib0"])
def test_stems_emulated(lib, kind):
    for regime in rk.REGIMES:
        rk.run_stem(lib, kind, regime, 1, seed=1, full=False)
    if kind == "calib0":
        rk.run_stem(lib, kind, "dense", 3, seed=2)
    boxes = rk.BOXES[[1, 2, 3]]
    rk.run_stem_fused(lib, kind, boxes, full=kind == "calib0", against_planes=rk.run_crop(lib, boxes, full=False)[2])
    rk.report("emu")


@pytest.mark.parametrize("unit", list(rk.UNITS))
def test_block_units_emulated(lib, unit):
    applied = 0
    for kind in ("init", "calib0"):
        for regime in rk.REGIMES:
            res = rk.run_block(lib, unit, kind, regime, 1, seed=3, full=False)
            applied += int("gate control applied" in res)
    res = rk.run_block(lib, unit, "calib0", "dense", 3 if rk.UNITS[unit].stage else 2, seed=4)
    assert applied, f"{unit}: the gate control (c) applied to no case"
    rk.report("emu")


def test_head_emulated(lib):
    for kind in ("init", "calib0"):
        for n in (1, 17):
            rk.run_head(lib, kind, n, seed=n)
    rk.report("emu")
