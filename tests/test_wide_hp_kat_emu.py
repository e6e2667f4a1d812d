"""The fp32-grade wide-OSNet known-answer harness (tests/kat/wide_hp_kat.hip: osnet_wide_hp_kernels.hpp and osnet_wide_hp_pack.hpp unchanged)
on CPU threads: the emulated MFMA, row shifts and global -> LDS copies of tests/host_emu/hip_shim.hpp.  Cases, float64 references, bands,
wrong-reference controls and the checks around a launch are tests/wide_hp_kat_common.py's; the device runs the full list
(tests/test_gpu_wide_hp_kat.py).  Here, one case per kernel family and regime at the smallest shapes:

  wide_pack_hp       the planes and biases of channels (32, 128, 128, 128), feat 128, bit for bit (host code: the same on both backends)
  k_wide_stem_hp<32> exact, impulses, dense at n = 1; impulses at n = 3
  k_gemm_hp          <0, 32, 1> (and <0, 32, 2> on the same inputs, identical bits), <0, 128, 2>, <1, 128, 2>, <4, 128, 2> at M in {3, 129} x
                     K in {32, 96} x N in {BN, 2 BN} x ReLU x bias, the second operand pair; <2, 128, 2> at H = 4 and 8, <3, 128, 2> at H = 8
                     and 16, n = 3, three regimes
  k_chain_hp         (32, 32, 24, 4) at H = 48 (one interior band), n = 1; (32, 8, 16, 0) at n = 3; three regimes
  k_gate_sum4_hp     C = 32 at (P, nbands) = (128, 1), (512, 4), (136, 2), n = 3; C = 128 at (136, 2), n = 1
  k_wide_gap_hp      C = 384, n in {1, 3, 11}

The emulation's exponential is libm's and its row shifts are emu_row_shift: the device test is the one that proves __expf, the DPP shifts at
lanes 0 and 15 and the real matrix pipe.  Measured here (wide_hp_kat_common.MEASURED["emu"], max|got - ref64| / max|ref64| of the dense and
impulse regimes, band = 4 x):
  stem 1.247e-06   gemm 7.385e-07   gemm.res 4.710e-07   gemm.pool 3.525e-07   gemm.f32 7.578e-07   chain 6.284e-07   gate 1.725e-07
  gap 6.486e-07    (the emulation is deterministic: every rerun shows figure / band = 0.25 at the worst case)
The whole file takes about 45 s, its 9 s build included (stem 11 s, the two GEMM lists 8 s each).  Not a product path."""
import shutil

import pytest

import wide_hp_kat_common as hk

CLANG = shutil.which("clang++", path="/opt/rocm/lib/llvm/bin") or shutil.which("clang++")
needs_clang = pytest.mark.skipif(CLANG is None, reason="needs a host clang with _Float16")


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return hk.WideHpKatLib(hk.build_emu(CLANG, tmp_path_factory.mktemp("wide_hp_kat_emu")), "emu")


def test_paired_order_is_the_definition():
    """logical channel 16 p + 4 g + r of a block of 32 sits at 8 g + 4 p + r; to_paired / from_paired are inverse"""
    pos = hk.paired_pos(64)
    for c in range(64):
        p, g, r = (c % 32) // 16, (c % 16) // 4, c % 4
        assert pos[c] == 32 * (c // 32) + 8 * g + 4 * p + r
    assert sorted(pos) == list(range(64))
    a = hk.np.arange(3 * 64.0).reshape(3, 64)
    assert hk.np.array_equal(hk.from_paired(hk.to_paired(a)), a) and hk.to_paired(a)[0, 4] == 16.0 and hk.to_paired(a)[0, 8] == 4.0


def test_controls_are_rejected():
    res = hk.controls()
    same = res.pop("same function")
    for name, count in res.items():
        assert count > 0, f"the comparison does not reject the wrong reference: {name}"
    print("controls that turned out to be the same function (reported, not asserted):", same)


def test_impulse_positions_cover_the_seams():
    """chain impulses sit on both sides of every wave seam and band seam, on the first and last window row of every band and on x = 15 / 16"""
    NT, R = 6, 16                       # ChainGeo<., 32, 24, 4>: 48 tiles over 8 waves (asserted against the harness in test_chain_emulated)
    pix = set(hk.chain_impulse_pixels((32, 32, 24, 4), 48, (NT, R, 0)))
    for band in range(3):
        y0 = band * R - 4
        for w in range(1, 8):
            for q in (w * NT * 16 - 1, w * NT * 16):
                y = y0 + q // 32
                assert not 0 <= y < 48 or (y, q % 32) in pix
        for y in (max(y0, 0), min(y0 + 23, 47), band * R, band * R + R - 1):
            assert any(p[0] == y for p in pix)
        assert {(band * R + 1, 15), (band * R + 1, 16)} <= pix
    assert {(0, 0), (0, 31), (47, 0), (47, 31)} <= pix
    rows = hk.pool_impulse_rows(8, 32, 3)
    for seam in range(4, 24, 4):        # 128 GEMM rows = 4 image rows: all four positions of the cells on both sides of every seam
        for gy in (seam - 2, seam - 1, seam, seam + 1):
            assert {(gy // 8, gy % 8, 0), (gy // 8, gy % 8, 1)} <= set(rows)


@needs_clang
def test_pack_planes_bit_for_bit(lib):
    assert hk.run_pack(lib) == 17          # conv1 and conv3 of six blocks, one downsample, two transitions, conv5, fc


@needs_clang
def test_outside_the_contract_is_refused(lib):
    assert hk.run_rejects(lib) > 20


@needs_clang
def test_stem_emulated(lib):
    for regime in hk.REGIMES:
        hk.run_stem(lib, 32, regime, 1, seed=1)
    hk.run_stem(lib, 32, "impulses", 3, seed=2)
    hk.report("emu")


@needs_clang
@pytest.mark.parametrize("regime", ["exact", "dense"])
def test_gemm_emulated(lib, regime):
    for epi, bn, db in ((0, 32, 1), (0, 128, 2), (1, 128, 2), (4, 128, 2)):
        hk.run_gemm_common(lib, epi, bn, db, regime, Ms=(3, 129), Ks=(32, 96), seed=60 + epi)
    hk.report("emu")


@needs_clang
@pytest.mark.parametrize("regime", hk.REGIMES)
def test_gemm_pool_emulated(lib, regime):
    for epi in (2, 3):
        hk.run_gemm_pool(lib, epi, regime, ns=(3,), seed=70)
    hk.report("emu")


@needs_clang
@pytest.mark.parametrize("regime", hk.REGIMES)
def test_chain_emulated(lib, regime):
    assert hk.chain_geo(lib, (32, 32, 24, 4))[:2] == (6, 16) and hk.chain_geo(lib, (32, 8, 16, 0))[:2] == (1, 16)
    hk.run_chain(lib, (32, 32, 24, 4), 48, regime, 1, seed=8)
    hk.run_chain(lib, (32, 8, 16, 0), 16, regime, 3, seed=10)
    hk.report("emu")


@needs_clang
def test_gate_and_gap_emulated(lib):
    for regime in ("exact", "dense"):
        for P, nbands in hk.GATE_CASES:
            hk.run_gate(lib, 32, P, nbands, regime, 3, seed=33)
        hk.run_gate(lib, 128, 136, 2, regime, 1, seed=31)
        for n in (1, 3, 11):
            hk.run_gap(lib, 384, 128, regime, n, seed=40 + n)
    hk.report("emu")
