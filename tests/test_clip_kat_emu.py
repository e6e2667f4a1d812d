"""The CLIP-ReID known-answer harness (tests/kat/clip_kat.hip, the device source of boxmot_amd/csrc/clip_kernels.hpp unchanged) on CPU
threads: the emulated MFMA and ds_read_b64_tr_b16 of tests/host_emu/hip_shim.hpp.  The regimes, references, bounds and wrong-reference
controls of tests/clip_kat_common.py on a reduced case list (attention at T in {2, 16, 17, 33, 48, 49, 129} with two heads,
k_clip_attention_t<33> and <129> once, LayerNorm on both code paths, the head, the patches); the device runs the full list
(tests/test_gpu_clip_kat.py).  The emulation's MFMA operand layout and its transposed LDS read are the author's model of the hardware:
this proves the index arithmetic, the masks and the bounds' bite against that model, the device test proves them on gfx950.  The
exponential here is the host's expf (measured below as on the device).  Not a product path."""
import shutil

import pytest

import clip_kat_common as ck

CLANG = shutil.which("clang++", path="/opt/rocm/lib/llvm/bin") or shutil.which("clang++")
pytestmark = pytest.mark.skipif(CLANG is None, reason="needs a host clang with _Float16")


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return ck.ClipKatLib(ck.build_emu(CLANG, tmp_path_factory.mktemp("clip_kat_emu")))


@pytest.fixture(scope="module")
def exp_rel(lib):
    m = ck.measure_expf(lib)
    print(f"emulated BM_EXPF (host expf): max relative error {m:.2e} over [{ck.EXPF_ARG_MIN}, 0]; the bound uses {ck.expf_bound(m):.2e}")
    assert m < 2.0 ** -22
    return ck.expf_bound(m)


def test_patches_emulated(lib):
    n = 0
    for i, (nc, H, W, patch, gh, gw) in enumerate([(1, 32, 32, 16, 2, 2), (3, 128, 64, 16, 8, 4), (1, 50, 20, 16, 3, 1), (3, 24, 16, 8, 3, 2),
                                                   (1, 256, 128, 16, 16, 8)]):
        n += ck.run_patches(lib, nc, H, W, patch, gh, gw, seed=i)
    print(f"emulated k_clip_patches: 5 geometries, {n} halves bit-exact")


def _report(name, res):
    emax = max(r[0] for r in res)
    rmax = max(r[1] for r in res)
    ctl = sorted({c for r in res for c in r[2]})
    print(f"{name}: {len(res)} cases, max err {emax:.2e}, max err / bound {rmax:.4f}; wrong references caught in every case they apply to: "
          f"{', '.join(ctl) if ctl else '(exact regime)'}")
    assert rmax < 1


@pytest.mark.parametrize("D", [128, 256, 768, 1024])
def test_layernorm_f16_emulated(lib, D):
    """both code paths (D = 768: registers; the others: the generic loop) inside the float64 bound AND bit-equal to the fp32 replay of the
    generic loop's arithmetic order; constant rows return fp16(beta), +-1 rows the closed form; row counts off a multiple of 4"""
    res = [ck.run_layernorm(lib, D, rows, kind, seed=D + rows) for rows in (1, 3, 4, 5, 129) for kind in ck.LN_KINDS]
    res += [ck.run_layernorm(lib, D, 5, kind, seed=D) for kind in ("const", "alt")]
    _report(f"emulated k_clip_layernorm_f16 D={D}", res)


@pytest.mark.parametrize("D", [128, 768])
def test_tokens_lnpre_emulated(lib, D):
    res = [ck.run_tokens_lnpre(lib, D, T, n, kind, seed=D + T) for T, n in ((2, 1), (2, 2), (5, 1), (5, 3), (129, 1)) for kind in ck.LN_KINDS]
    res += [ck.run_tokens_lnpre(lib, D, 5, 3, kind, seed=D) for kind in ("const", "alt")]
    _report(f"emulated k_clip_tokens_lnpre D={D}", res)


@pytest.mark.parametrize("regime", ck.ATTN_REGIMES)
def test_attention_emulated(lib, exp_rel, regime):
    """k_clip_attention at T = 2 .. 129 (two heads; three crops at T = 17 and 33), and k_clip_attention_t<33> / <129> bit-identical to it"""
    res = []
    for T in (2, 16, 17, 33, 48, 49, 129):
        for n in ((1, 3) if T in (17, 33) else (1,)):
            qkv, pi = ck.attn_inputs(regime, n, T, 2, seed=100 * T + n)
            bits = ck.attn_launch(lib, qkv, n, T, 2, tmpl=False)
            res.append(ck.check_attention(f"emulated k_clip_attention T={T} n={n}", regime, bits, qkv, pi, n, T, 2, exp_rel))
            if T == 33 or (T == 129 and n == 1):
                tb = ck.attn_launch(lib, qkv, n, T, 2, tmpl=True)
                res.append(ck.check_attention(f"emulated k_clip_attention_t<{T}> n={n}", regime, tb, qkv, pi, n, T, 2, exp_rel))
                assert (tb == bits).all(), f"k_clip_attention_t<{T}> and k_clip_attention differ in {int((tb != bits).sum())} halves [{regime}]"
    _report(f"emulated attention [{regime}]", res)


def test_head_emulated(lib):
    res = [ck.run_head(lib, D, E, T, n, sc, seed=D + E + T + n) for D, E, T, n, sc in ((128, 128, 2, 1, True), (128, 512, 129, 3, True),
                                                                                      (768, 128, 2, 3, False), (768, 512, 2, 8, True),
                                                                                      (128, 128, 129, 8, False))]
    _report("emulated k_clip_head", res)
