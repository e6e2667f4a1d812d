"""The GEMM known-answer harness (tests/kat/gemm_kat.hip, the device source of boxmot_amd/csrc/gemm_f16.hpp unchanged) on CPU threads:
the emulated MFMA of tests/host_emu/hip_shim.hpp, fiber mode, global -> LDS copies that land only at the issuing thread's wait -- and for
k_gemm_f16_256 a COUNTED wait (vmcnt(6) leaves the thread's six youngest copies in flight), so a wrong count in the copy pipeline's
prologue, steady state or tail reads a tile before it has landed.  The exact and random regimes of tests/gemm_kat_common.py at small
shapes (M <= 300, N <= 256, K <= 256, and the pooled shapes of one or three crops); the device runs the full shape list
(tests/test_gpu_gemm_kat.py).  The emulation's MFMA operand layout is the author's model of the hardware: this proves the index
arithmetic, the tails and the pipeline against that model, the device test proves it on gfx950.  Not a product path."""
import shutil

import pytest

from gemm_kat_common import Case, KatLib, build_emu, run_case

CLANG = shutil.which("clang++", path="/opt/rocm/lib/llvm/bin") or shutil.which("clang++")
needs_clang = pytest.mark.skipif(CLANG is None, reason="needs a host clang with _Float16")


@pytest.fixture(scope="module")
def emu_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("gemm_kat_emu")


@pytest.fixture(scope="module")
def lib(emu_dir):
    return KatLib(build_emu(CLANG, emu_dir))


def _cases():
    cs = []
    # k_gemm_f16_256: K = 64 / 128 / 192 / 256 -- one to four k-tiles: the prologue's vmcnt(0) branch, the tail's, and the steady state
    for epi in range(5):
        cs += [Case("256", epi, 0, 17, 256, 64), Case("256", epi, 0, 257, 256, 192, relu=epi in (3, 4), res=epi == 4)]
    cs += [Case("256", 2, 0, 129, 256, 128), Case("256", 0, 0, 300, 256, 256), Case("256", 4, 0, 256, 256, 128, res=True)]
    # k_gemm_f16_glds<0..3, 64> (CLIP, M < 1024) and the wide OSNets' <3 | 4 | 5 | 6, 32>
    for epi in range(4):
        cs += [Case("glds", epi, 64, 129, 256, 128), Case("glds", epi, 64, 1, 128, 64)]
    cs += [Case("glds", 3, 32, 15, 256, 96, relu=1), Case("glds", 3, 32, 129, 128, 32, relu=1)]
    cs += [Case("glds", 4, 32, 130, 128, 64), Case("glds", 4, 32, 255, 256, 96, relu=1, res=True),
           Case("glds", 4, 32, 129, 128, 32, relu=1, res=True, K2=64), Case("glds", 4, 32, 17, 128, 64, K2=32, bias=False)]
    cs += [Case("glds", 5, 32, 64 * 32, 128, 64, pool_w=32), Case("glds", 6, 32, 32 * 16, 128, 96, pool_w=16),
           Case("glds", 6, 32, 3 * 32 * 16, 128, 32, pool_w=16)]
    # k_gemm_f16<4, 32 | 64 | 96> (WideOsNet::gemm, N % 128 != 0) and <0..3, 128> (ClipNet::gemm, K % 64 != 0)
    cs += [Case("f16", 4, 32, 129, 96, 64, relu=1, res=True), Case("f16", 4, 64, 17, 192, 96), Case("f16", 4, 96, 255, 288, 32, relu=1)]
    for epi in range(4):
        cs += [Case("f16", epi, 128, 129, 256, 96, relu=epi == 3), Case("f16", epi, 128, 1, 128, 32)]
    return cs


CASES = _cases()


@needs_clang
@pytest.mark.parametrize("regime", ["exact", "random"])
def test_gemm_family_known_answers_emulated(lib, regime):
    per = {}
    for c in CASES:
        if regime == "exact" and c.epi == 1:
            continue
        err, ratio = run_case(lib, c, regime, seed=c.M + 7 * c.N + 13 * c.K + c.epi)
        n, e, r = per.get(c.family, (0, 0.0, 0.0))
        per[c.family] = (n + 1, max(e, err), max(r, ratio))
    for fam, (n, e, r) in per.items():
        print(f"emulated {fam}: {n} cases " + ("bit-exact" if regime == "exact" else f"max err {e:.2e}, max err / bound {r:.2f}"))


@needs_clang
@pytest.mark.parametrize("keep", [7, 8])
def test_counted_wait_negative_control(emu_dir, keep):
    """A shim build whose vmcnt(6) leaves `keep` copies in flight: k_gemm_f16_256 then reads operand halves before they land and the
    exact regime must fail -- evidence that the emulated counted wait, and so the passing test above, checks the pipeline's count.
    (M = 256: every row of the late half tile B-1 is stored; with M = 129 only its first row would be, and keep = 7 delays other rows.)"""
    bad = KatLib(build_emu(CLANG, emu_dir, defines=(f"EMU_GEMM_WAIT6_KEEP={keep}",)))
    for K in (128, 256):
        with pytest.raises(AssertionError):
            run_case(bad, Case("256", 0, 0, 256, 256, K), "exact")
