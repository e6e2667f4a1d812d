"""Known-answer tests of the fp32-grade OSNet-x0.25 kernels (ReID mode 2: boxmot_amd/csrc/reid_hp.hpp, k_stem_resize_fused_hp of
reid_fused.hpp), one kernel at a time on the device: tests/kat/reid_hp_kat.hip includes the headers unchanged, packs with the product's
packers and launches each kernel as reid_engine.hpp's prepare_hp / forward_hp do (grid, block, dynamic LDS, hipFuncSetAttribute per
instantiation); tests/reid_hp_kat_common.py holds the inputs, the float64 references, the bands, the wrong-reference controls and the
poison / guard / count / independence / determinism checks.

  k_crop_resize_rgbx_hl          eight boxes at frame width 641 (general, clipped, empty, identity-sized, whole frame): hi + lo within
                                 max(2**-22 |f|, 2**-25) of oracle.crops.get_crops, border untouched, X channel zero
  k_stem_hp                      {init, calib0, calib1} x {dense, impulses, blank} x n in {1, 3} on planes built directly
  k_stem_resize_fused_hp         the same weights on frame + boxes, n in {1, 3}; agrees with k_stem_hp run on the crop kernel's planes
  stage-0 pair (EMIT, RECON)     the two fp32 hand-over tensors after the first launch, the pooled conv2.2 output after the second
  conv3.0, conv3.1 + transition, conv4.0, conv4.1    each {init, calib0, calib1} x {dense, impulses, blank} x n in {1, 3}
  k_head_hp<128, 512>            n in {1, 15, 16, 17, 33} (HEAD_NB = 16), out_rows scattered, device-side count

Metric: max|got - ref64| / max|ref64| per crop and tensor; band = 4 x the largest value measured over every case of the unit and weight
kind (reid_hp_kat_common.MEASURED), none above 2e-5.  Measured on an MI355X by this file (every test prints its figures; the last line
of each test is the running table):

  unit          init:                   calib:                  (measured / band is 0.250 by construction; every test prints the ratio
                measured   band         measured   band          it sees, 1.0 would be a failure)
  stem          6.037e-07  2.415e-06   5.090e-07  2.036e-06
  stem_fused    3.158e-07  1.263e-06   3.977e-07  1.591e-06
  pair.x2s      2.371e-07  9.484e-07   5.394e-07  2.158e-06
  pair.x1s      3.676e-07  1.470e-06   6.151e-07  2.460e-06
  pair          6.563e-07  2.625e-06   9.995e-07  3.998e-06
  conv3.0       3.353e-07  1.341e-06   5.463e-07  2.185e-06
  conv3.1       6.654e-07  2.662e-06   9.397e-07  3.759e-06
  conv4.0       3.713e-07  1.485e-06   7.041e-07  2.816e-06
  conv4.1       1.374e-07  5.496e-07   6.223e-07  2.489e-06
  head          1.752e-06  7.008e-06   1.589e-06  6.356e-06
  (pair.x2s, pair.x1s: the hand-over tensors; pair: the pooled conv2.2 output.  The emulation's own row is MEASURED["emu"].)
  k_crop_resize_rgbx_hl: max |hi + lo - f| / |f| = 3.85e-06, 31603 of 786432 elements beyond 2**-22 |f| -- all of them where lo is an
  fp16 subnormal (|f - hi| < 2**-14), inside the derived 2**-25 absolute (reid_hp_kat_common.run_crop).

The whole file (31 tests) takes 10 s on the device after a 3 s build; the nine `fast` cases 4 s."""
import pytest

import reid_hp_kat_common as rk

pytestmark = pytest.mark.gpu

FAST = pytest.mark.fast


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return rk.ReidHpKatLib(rk.build_gpu(tmp_path_factory.mktemp("reid_hp_kat")), "gpu")


def test_crop_kernel(lib):
    rel, beyond, _ = rk.run_crop(lib, rk.BOXES)
    print(f"k_crop_resize_rgbx_hl: max |hi + lo - f| / |f| = {rel:.3e}; {beyond} elements beyond 2**-22 |f| (lo subnormal: 2**-25 absolute)")


@pytest.mark.parametrize("kind", rk.WEIGHT_KINDS)
def test_stems(lib, kind):
    """k_stem_hp on planes built directly, k_stem_resize_fused_hp on frame + boxes, and the two against each other"""
    for regime in rk.REGIMES:
        for n in (1, 3):
            rk.run_stem(lib, kind, regime, n, seed=10 + n)
    rk.run_stem_fused(lib, kind, rk.BOXES[:1])
    boxes = rk.BOXES[[1, 2, 3]]
    rk.run_stem_fused(lib, kind, boxes, against_planes=rk.run_crop(lib, boxes, full=False)[2])
    rk.run_stem_fused(lib, kind, rk.BOXES[[4, 5, 6]], full=False)
    rk.report("gpu")


@pytest.mark.parametrize("kind", rk.WEIGHT_KINDS)
@pytest.mark.parametrize("unit", list(rk.UNITS))
def test_block_units(lib, unit, kind):
    """every regime at n = 1 and n = 3 with the whole protocol around each launch.  The pair's docstring (BlockUnit.reference) states what
    the two hand-over tensors hold."""
    applied = 0
    for regime in rk.REGIMES:
        for n in (1, 3):
            applied += int("gate control applied" in rk.run_block(lib, unit, kind, regime, n, seed=20 + n))
    assert applied, f"{unit} [{kind}]: the gate control (c) applied to no case"
    rk.report("gpu")


@pytest.mark.parametrize("kind", rk.WEIGHT_KINDS)
def test_head(lib, kind):
    for n in (1, 15, 16, 17, 33):
        rk.run_head(lib, kind, n, seed=n)
    rk.report("gpu")


@pytest.mark.parametrize("unit", [pytest.param(u, marks=FAST) for u in ("crop", "stem", "stem_fused", *rk.UNITS, "head")])
def test_one_small_case_per_unit(lib, unit):
    if unit == "crop":
        rk.run_crop(lib, rk.BOXES[[1, 2, 3]])
    elif unit == "stem":
        rk.run_stem(lib, "calib0", "impulses", 1, seed=1)
    elif unit == "stem_fused":
        rk.run_stem_fused(lib, "calib0", rk.BOXES[:1])
    elif unit == "head":
        rk.run_head(lib, "calib0", 17, seed=17)
    else:
        rk.run_block(lib, unit, "calib0", "impulses", 1, seed=21)
