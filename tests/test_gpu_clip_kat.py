"""Known-answer tests of the CLIP-ReID kernels around the GEMMs (boxmot_amd/csrc/clip_kernels.hpp), element by element on the device:
tests/kat/clip_kat.hip includes the header unchanged and launches each kernel as clip_engine.hpp does (grid, block, dynamic LDS,
hipFuncSetAttribute for both attention kernels); tests/clip_kat_common.py holds the inputs, the float64 references, the worst-case
bounds, the wrong-reference controls that show the bounds bite, and the poison / guard / determinism checks.

  k_clip_patches           bit-exact; five geometries, and 171 crops of 256 x 128: more than 65 535 blocks' worth, the grid-stride loop
  k_clip_layernorm_f16     D in {128, 256, 768, 1024} x rows in {1, 3, 4, 5, 129, 7 * 129, 1032} x {N(0, 1), mean 1e3, magnitude 1e-3} rows,
                           constant and +-1 rows; the register path (D = 768) and the generic loop both bit-equal to the fp32 replay of
                           the generic loop's stated arithmetic order
  k_clip_tokens_lnpre      the same D and row kinds at T in {2, 5, 129}
  k_clip_attention         T in ATTN_TS (every side of the 16-key and 32-key tile edges up to the 192-token limit and its 80 896-byte LDS
                           request) x heads in {2, 12} x n in {1, 3}, four input regimes (one-hot: bit-exact)
  k_clip_attention_t<129>  heads in {2, 12} x n in {1, 3, 8}; bit-identical to k_clip_attention at T = 129 in every regime
  k_clip_head              D in {128, 768} x E in {128, 512} x T in {2, 129} x n in {1, 3, 8}, out_rows scattered and null
and the refusal of CLP1 blobs outside the engine's limits.  Measured on an MI355X: see the figures in clip_kat_common.py (EXPF_*) and
printed by each test (max err / bound per kernel)."""
import numpy as np
import pytest

import clip_kat_common as ck

pytestmark = pytest.mark.gpu

ATTN_TS = (2, 15, 16, 17, 31, 32, 33, 47, 48, 49, 64, 65, 80, 81, 128, 129, 130, 144, 145, 176, 177, 191, 192)
LN_DS = (128, 256, 768, 1024)
LN_ROWS = (1, 3, 4, 5, 129, 7 * 129, 1032)
TOKEN_SHAPES = ((2, 1), (2, 2), (5, 1), (5, 3), (129, 1), (129, 7), (129, 8))           # (T, n): rows 2, 4, 5, 15, 129, 7 * 129, 1032


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return ck.ClipKatLib(ck.build_gpu(tmp_path_factory.mktemp("clip_kat"), timeout=900))


@pytest.fixture(scope="module")
def exp_rel(lib):
    m = ck.measure_expf(lib)
    print(f"device BM_EXPF (__expf): max relative error {m:.3e} over [{ck.EXPF_ARG_MIN}, 0]; the bound uses {ck.expf_bound(m):.3e}")
    return ck.expf_bound(m)


def _report(name, res):
    emax, rmax = max(r[0] for r in res), max(r[1] for r in res)
    ctl = sorted({c for r in res for c in r[2]})
    print(f"{name}: {len(res)} cases, max err {emax:.2e}, max err / bound {rmax:.4f}; wrong references caught in every case they apply to: "
          f"{', '.join(ctl) if ctl else '(exact regime: every case bit-exact)'}")
    assert rmax < 1


@pytest.mark.fast
def test_device_expf(lib):
    """the one measured constant of the attention bound: __expf against float64 on the arguments that matter.  4 x the figure must stay a
    small part of the 2**-11 the fp16 probabilities carry anyway, or the bound would be measuring the exponential, not the kernel"""
    m = ck.measure_expf(lib)
    print(f"device BM_EXPF (__expf): max relative error {m:.3e} over [{ck.EXPF_ARG_MIN}, 0]; 4 x = {4 * m:.3e}, floor {ck.EXPF_FLOOR:.3e}")
    assert 4 * m < 2.0 ** -14


@pytest.mark.fast
def test_patches_small(lib):
    n = ck.run_patches(lib, 3, 32, 32, 16, 2, 2) + ck.run_patches(lib, 1, 24, 16, 8, 3, 2)
    print(f"k_clip_patches (small): {n} halves bit-exact")


def test_patches(lib):
    tot = 0
    geos = [(256, 128, 16, 16, 8), (32, 32, 16, 2, 2), (128, 64, 16, 8, 4), (50, 20, 16, 3, 1), (24, 16, 8, 3, 2)]
    for i, (H, W, patch, gh, gw) in enumerate(geos):
        for n in (1, 3):
            tot += ck.run_patches(lib, n, H, W, patch, gh, gw, seed=10 * i + n)
    print(f"k_clip_patches: {2 * len(geos)} cases, {tot} halves bit-exact")
    big = ck.run_patches(lib, 171, 256, 128, 16, 16, 8, seed=99)
    assert big // 256 > 65535
    print(f"k_clip_patches, 171 crops of 256 x 128 ({big // 256} > 65535 blocks' worth: the grid-stride loop): {big} halves bit-exact")


@pytest.mark.fast
def test_layernorm_small(lib):
    res = [ck.run_layernorm(lib, D, rows, kind, seed=rows) for D, rows in ((768, 5), (256, 3)) for kind in ck.LN_KINDS + ("const", "alt")]
    _report("k_clip_layernorm_f16 (small)", res)


@pytest.mark.parametrize("D", LN_DS)
def test_layernorm_f16(lib, D):
    res = [ck.run_layernorm(lib, D, rows, kind, seed=D + rows) for rows in LN_ROWS for kind in ck.LN_KINDS]
    res += [ck.run_layernorm(lib, D, rows, kind, seed=D) for rows in (5, 129) for kind in ("const", "alt")]
    _report(f"k_clip_layernorm_f16 D={D} ({'register path' if D == 768 else 'generic loop'}; every case bit-equal to the fp32 replay)", res)


@pytest.mark.fast
def test_tokens_lnpre_small(lib):
    res = [ck.run_tokens_lnpre(lib, 128, 5, 3, kind, seed=1) for kind in ck.LN_KINDS + ("const", "alt")]
    _report("k_clip_tokens_lnpre (small)", res)


@pytest.mark.parametrize("D", LN_DS)
def test_tokens_lnpre(lib, D):
    res = [ck.run_tokens_lnpre(lib, D, T, n, kind, seed=D + T + n) for T, n in TOKEN_SHAPES for kind in ck.LN_KINDS]
    res += [ck.run_tokens_lnpre(lib, D, T, n, kind, seed=D) for T, n in ((5, 3), (129, 1)) for kind in ("const", "alt")]
    _report(f"k_clip_tokens_lnpre D={D}", res)


def _attention(lib, exp_rel, regime, T, n, heads, tmpl, seed):
    qkv, pi = ck.attn_inputs(regime, n, T, heads, seed=seed)
    bits = ck.attn_launch(lib, qkv, n, T, heads, tmpl=tmpl)
    name = f"k_clip_attention_t<{T}>" if tmpl else f"k_clip_attention T={T}"
    return bits, qkv, ck.check_attention(f"{name} heads={heads} n={n}", regime, bits, qkv, pi, n, T, heads, exp_rel)


@pytest.mark.fast
@pytest.mark.parametrize("regime", ck.ATTN_REGIMES)
def test_attention_small(lib, exp_rel, regime):
    res = [_attention(lib, exp_rel, regime, T, 1, 2, False, seed=T)[2] for T in (17, 33, 192)]
    res.append(_attention(lib, exp_rel, regime, 129, 1, 2, True, seed=129)[2])
    _report(f"attention (small) [{regime}]", res)


@pytest.mark.parametrize("heads", [2, 12])
@pytest.mark.parametrize("regime", ck.ATTN_REGIMES)
def test_attention_runtime_t(lib, exp_rel, regime, heads):
    """k_clip_attention: the 12-entry score array and its run-time guards, TP != KP (T in 33..48, 65..80, ...) and the T = 192 LDS request"""
    per_t = []
    for T in ATTN_TS:
        res = [_attention(lib, exp_rel, regime, T, n, heads, False, seed=1000 * T + 10 * heads + n)[2] for n in (1, 3)]
        per_t.append(f"T={T}: {max(r[1] for r in res):.3f}")
        _report(f"k_clip_attention T={T} heads={heads} [{regime}]", res)
    print(f"k_clip_attention heads={heads} [{regime}] max err / bound per T: " + ", ".join(per_t))


@pytest.mark.parametrize("heads", [2, 12])
@pytest.mark.parametrize("regime", ck.ATTN_REGIMES)
def test_attention_t129_and_bit_identity(lib, exp_rel, regime, heads):
    """k_clip_attention_t<129> (V^T fragments by ds_read_b64_tr_b16) in every regime, and bit for bit what k_clip_attention returns at
    T = 129 on the same rows"""
    res = []
    for n in (1, 3, 8):
        bits, qkv, r = _attention(lib, exp_rel, regime, 129, n, heads, True, seed=129000 + 10 * heads + n)
        res.append(r)
        other = ck.attn_launch(lib, qkv, n, 129, heads, tmpl=False)
        assert np.array_equal(bits, other), (f"k_clip_attention_t<129> and k_clip_attention differ in {int((bits != other).sum())} of "
                                             f"{bits.size} halves [{regime}, heads={heads}, n={n}]")
    _report(f"k_clip_attention_t<129> heads={heads} [{regime}] (bit-identical to k_clip_attention in every case)", res)


@pytest.mark.fast
def test_head_small(lib):
    _report("k_clip_head (small)", [ck.run_head(lib, 128, 128, 2, 3, True), ck.run_head(lib, 768, 512, 129, 1, False)])


def test_head(lib):
    res = []
    for D in (128, 768):
        for E in (128, 512):
            for T in (2, 129):
                for n in (1, 3, 8):
                    for sc in (True, False):
                        res.append(ck.run_head(lib, D, E, T, n, sc, seed=D + E + T + n))
    _report("k_clip_head", res)


def _header_only_blob(width, heads, gh, gw):
    from boxmot_amd.clip_weights import HEADER_INTS, MAGIC
    h = np.zeros(HEADER_INTS, np.int32)
    h[:10] = [MAGIC, width, 2, heads, 16, gh, gw, 128, gh * 16, gw * 16]
    return h.view(np.float32).copy()


@pytest.mark.fast
@pytest.mark.parametrize("what,width,heads,gh,gw", [("193 tokens", 128, 2, 16, 12), ("width not a multiple of 128", 192, 3, 16, 8)])
def test_clp1_blob_outside_the_limits_is_refused(what, width, heads, gh, gw):
    """ClipNet's geometry check (clip_engine.hpp) through HipReID and through the C ABI: the message names the limits"""
    from boxmot_amd import _lib
    from boxmot_amd.reid import HipReID
    blob = _header_only_blob(width, heads, gh, gw)
    with pytest.raises(RuntimeError) as e:
        HipReID(blob, max_crops=4)
    assert "multiple of 128" in str(e.value) and "192 tokens" in str(e.value), str(e.value)
    L = _lib.load()
    assert not L.boxmot_hip_reid_create(None, blob.ctypes.data, int(blob.size), 4)
    assert "multiple of 128" in _lib.last_error() and "192 tokens" in _lib.last_error(), _lib.last_error()
