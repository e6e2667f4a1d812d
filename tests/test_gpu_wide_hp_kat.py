"""Known-answer tests of the fp32-grade wide-OSNet kernels (ReID mode 2 at x1.0: boxmot_amd/csrc/osnet_wide_hp_kernels.hpp), one kernel at a
time on the device: tests/kat/wide_hp_kat.hip includes the header and osnet_wide_hp_pack.hpp unchanged and launches each kernel as
wide_hp_forward does; tests/wide_hp_kat_common.py holds the inputs, the float64 references, the bands, the wrong-reference controls and the
poison / guard / determinism / crop-independence checks.  exact is bit for bit in both planes (impulses too for the stem and the pooling
GEMM), dense and the chain's impulses are inside 4 x the measured figure.

  wide_pack_hp          planes and biases of channels (32, 128, 128, 128), feat 128, bit for bit
  k_wide_stem_hp<32|64> {exact, impulses, dense} x n in {1, 3}; impulses on conv rows 0, 1, 7, 8, 64, 126, 127 x columns 0, 1, 15, 16, 31, 32, 47,
                        48, 62, 63; zero border, zero X channel, non-zero lo plane, NaN after the last crop
  k_gemm_hp             <0, 32|64|96|128, 1|2>, <1|4, 128, 2>: M in {1, 3, 127, 128, 129, 257} x K in {32, 64, 96} x N in {BN, 2 BN} x ReLU x bias,
                        {exact, dense}; <0, BN, 1> and <0, BN, 2> on the same inputs, identical bits; EPI 0 with K2 in {32, 96} at K != K2; BN = 128 at
                        M = 257, N = 512; <2, 128, 2> at H in {4, 8}, <3, 128, 2> at H in {8, 16}, n in {1, 3}, three regimes; -1 outside the contract
  k_chain_hp            (32|64, 32, 24, 4) at H in {16, 48, 64}, (32|64|96, 16, 32, 0) at H = 32, (32|64|96|128, 8, 16, 0) at H = 16, n in {1, 3},
                        three regimes; gap_part against the kernel's own outputs
  k_gate_sum4_hp<C>     C in {32, 64, 96, 128} x (P, nbands) in {(128, 1), (512, 4), (136, 2)} (+ (2048, 4) at C = 64) x n in {1, 3}, {exact, dense}
  k_wide_gap_hp         C in {384, 512}, P = 128, n in {1, 3, 11}, {exact, dense}

Measured on an MI355X by this file (wide_hp_kat_common.MEASURED["gpu"]; every test prints its figures): max|got - ref64| / max|ref64| per
crop and tensor over the dense (and the chain's impulse) cases, the band 4 x that, and figure / band of a rerun (the kernels are
deterministic: every launch is also run twice for identical bits):
  unit        measured    band        ratio       unit        measured    band        ratio
  stem        5.631e-07   2.252e-06   0.250       chain       1.034e-06   4.136e-06   0.250
  gemm        4.250e-07   1.700e-06   0.250       gate        2.743e-07   1.097e-06   0.250   (+ gate_allowance = 3.410e-07 per unit of sum |y_b|)
  gemm.res    2.298e-07   9.192e-07   0.250       gap         6.486e-07   2.594e-06   0.250
  gemm.pool   1.943e-07   7.772e-07   0.250       gemm.f32    3.232e-07   1.293e-06   0.250
All far below the cap of 2e-5; every exact and impulse comparison is bit for bit on the device, the four-layer chains included.
The whole file (84 tests) takes 24 s on the device, its 4 s build included; no test above 1.1 s; the five `fast` cases under a second."""
import pytest

import wide_hp_kat_common as hk

pytestmark = pytest.mark.gpu

FAST = pytest.mark.fast


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return hk.WideHpKatLib(hk.build_gpu(tmp_path_factory.mktemp("wide_hp_kat")), "gpu")


def test_pack_planes_bit_for_bit(lib):
    assert hk.run_pack(lib) == 17


def test_outside_the_contract_is_refused(lib):
    assert hk.run_rejects(lib) > 20


@pytest.mark.parametrize("regime", hk.REGIMES)
@pytest.mark.parametrize("c0", [32, 64])
def test_stem(lib, c0, regime):
    for n in (1, 3):
        hk.run_stem(lib, c0, regime, n, seed=10 + n)
    hk.report("gpu")


@pytest.mark.parametrize("regime", ["exact", "dense"])
@pytest.mark.parametrize("inst", [i for i in hk.GEMM_INST if i[0] not in (2, 3)], ids=lambda i: "epi%d-bn%d-db%d" % i)
def test_gemm(lib, inst, regime):
    hk.run_gemm_common(lib, *inst, regime, seed=60 + inst[0])
    hk.report("gpu")


@pytest.mark.parametrize("regime", hk.REGIMES)
@pytest.mark.parametrize("epi", [2, 3])
def test_gemm_pool(lib, epi, regime):
    hk.run_gemm_pool(lib, epi, regime, seed=70)
    hk.report("gpu")


@pytest.mark.parametrize("regime", hk.REGIMES)
@pytest.mark.parametrize("case", [(i, H) for i in hk.CHAIN_INST for H in hk.chain_heights(i)], ids=lambda c: "C%d-W%d-WR%d-HALO%d-H%d" % (*c[0], c[1]))
def test_chain(lib, case, regime):
    for n in (1, 3):
        hk.run_chain(lib, case[0], case[1], regime, n, seed=7 + n)
    hk.report("gpu")


@pytest.mark.parametrize("C", [32, 64, 96, 128])
def test_gate(lib, C):
    for regime in ("exact", "dense"):
        for P, nbands in hk.GATE_CASES + (((2048, 4),) if C == 64 else ()):
            for n in (1, 3):
                hk.run_gate(lib, C, P, nbands, regime, n, seed=30 + n)
    hk.report("gpu")


@pytest.mark.parametrize("C", [384, 512])
def test_gap(lib, C):
    for regime in ("exact", "dense"):
        for n in (1, 3, 11):
            hk.run_gap(lib, C, 128, regime, n, seed=40 + n)
    hk.report("gpu")


@pytest.mark.parametrize("kernel", [pytest.param(k, marks=FAST) for k in ("stem", "gemm", "chain", "gate", "gap")])
def test_one_small_case_per_kernel(lib, kernel):
    if kernel == "stem":
        hk.run_stem(lib, 32, "impulses", 1, seed=1)
    elif kernel == "gemm":
        hk.run_gemm(lib, hk.gemm_inputs("exact", 0, 129, 64, 64, seed=2, K2=32), 32, 1, also_db=2)
    elif kernel == "chain":
        hk.run_chain(lib, (32, 8, 16, 0), 16, "exact", 3, seed=10)
    elif kernel == "gate":
        hk.run_gate(lib, 32, 136, 2, "exact", 1, seed=3)
    else:
        hk.run_gap(lib, 384, 128, "exact", 3, seed=4)
