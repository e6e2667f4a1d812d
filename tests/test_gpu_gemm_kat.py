"""Known-answer tests of every fp16 GEMM instantiation the library launches (boxmot_amd/csrc/gemm_f16.hpp), element by element on the
device: tests/kat/gemm_kat.hip includes the header unchanged and launches each kernel as clip_engine.hpp / osnet_wide.hpp do (grid,
block, dynamic LDS, hipFuncSetAttribute); tests/gemm_kat_common.py holds the two input regimes, the fp64 reference, the worst-case
bound of the random regime and the poison / guard / determinism checks.

Instantiations, against the launches of the product:
  k_gemm_f16_256<0, 1, 2>    ClipNet::gemm, N % 256 == 0, K % 64 == 0, M >= 1024      <3, 4>: promised by the header
  k_gemm_f16_glds<0..3, 64>  ClipNet::gemm, K % 64 == 0 otherwise
  k_gemm_f16<0..3, 128>      ClipNet::gemm, K % 64 != 0
  k_gemm_f16_glds<3, 32>     WideOsNet::forward's head (M = crops, ReLU)
  k_gemm_f16_glds<4, 32>     WideOsNet::gemm, N % 128 == 0 (ReLU on / off, residual or none, the X2 / W2 / K2 dual product)
  k_gemm_f16_glds<5 | 6, 32> WideOsNet::gemm's transitions: ReLU + 2 x 2 average pool, image width 32 / 16, one or three crops
  k_gemm_f16<4, 32 | 64 | 96> WideOsNet::gemm, N % 128 != 0
plus both products' dispatch restated in the harness (kat_clip_gemm, kat_wide_gemm) on each side of every branch."""
import pytest

from gemm_kat_common import Case, KatLib, build_gpu, run_case

pytestmark = pytest.mark.gpu

MS = (1, 15, 16, 17, 127, 128, 129, 255, 256, 257, 1023, 1024, 1025, 1032, 7 * 129, 64 * 129)
K256 = (64, 128, 192, 768, 3072)


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return KatLib(build_gpu(tmp_path_factory.mktemp("gemm_kat"), timeout=900))


def _256(epi):
    # N tiles 1..9 against M tiles 1..33: tile totals 1 (M 1), 7 (127 x 1792), 8 (1023 x 512), 9 (17 x 2304; 2049 x 256), 17 (4225 x 256)
    ns = (256, 512, 768, 2304, 1792, 256, 1024, 2048, 256, 512, 512, 768, 256, 1280, 256, 768)
    cs = [Case("256", epi, 0, m, n, K256[i % 5], relu=int(epi in (3, 4) and i % 2), res=epi == 4 and i % 3 != 2)
          for i, (m, n) in enumerate(zip(MS, ns))]
    cs += [Case("256", epi, 0, 2049, 256, 128), Case("256", epi, 0, 4225, 256, 64, relu=int(epi in (3, 4)))]
    if epi == 2:                # configuration 5's projection: 256 crops x 129 tokens, 768 x 3072
        cs.append(Case("256", 2, 0, 256 * 129, 768, 3072))
    return cs


def _glds64(epi):
    ns = (128, 256, 384, 1152, 896, 128, 512, 1024, 128, 256, 512, 384, 128, 640, 128, 384)
    return [Case("glds", epi, 64, m, n, K256[i % 5]) for i, (m, n) in enumerate(zip(MS, ns))]


def _f16_128(epi):
    ks = (32, 96, 160, 224, 800)
    ns = (128, 256, 384, 1152, 896, 128, 512, 1024, 128, 256, 512, 384, 128, 640, 128, 384)
    return [Case("f16", epi, 128, m, n, ks[i % 5], relu=int(epi == 3 and i % 2)) for i, (m, n) in enumerate(zip(MS, ns))]


def _head():
    # M = number of crops, N = the embedding (512), K = c3 of x0.5 / x0.75 / x1.0 and short K
    return [Case("glds", 3, 32, m, 512, k, relu=1) for m, k in ((1, 256), (15, 384), (16, 512), (17, 32), (127, 64), (128, 96),
                                                                   (129, 512), (255, 384), (256, 256), (257, 512))] + \
           [Case("glds", 3, 32, 129, 128 * t, 32, relu=0) for t in (1, 7, 9)]


def _glds4():
    cs = []
    for i, m in enumerate(MS):
        n = 128 * (1 + i % 9)
        k = (32, 64, 96, 128, 256, 384)[i % 6]
        cs.append(Case("glds", 4, 32, m, n, k, relu=i % 2, res=i % 4 < 2))
        cs.append(Case("glds", 4, 32, m, n, k, relu=(i + 1) % 2, res=i % 4 >= 2, K2=(32, 64, 128)[i % 3], bias=i % 5 != 0))
    return cs


def _pool():
    return [Case("glds", 5, 32, n * 64 * 32, c, k, pool_w=32) for n, c, k in ((1, 128, 64), (3, 256, 256), (3, 384, 96))] + \
           [Case("glds", 6, 32, n * 32 * 16, c, k, pool_w=16) for n, c, k in ((1, 256, 256), (3, 384, 384), (3, 128, 32))]


def _f16_4(bn):
    ns = {32: (32, 96, 160), 64: (64, 192, 320), 96: (96, 288, 480)}[bn]
    return [Case("f16", 4, bn, m, ns[i % 3], (32, 64, 96, 128, 256)[i % 5], relu=i % 2, res=i % 3 != 1) for i, m in enumerate(MS)]


def _routes():
    cs = []
    for epi in range(4):       # ClipNet::gemm: each side of M = 1024 and of K % 64
        cs += [Case("clip", epi, 0, 1023, 768, 768), Case("clip", epi, 0, 1024, 768, 768), Case("clip", epi, 0, 1032, 512, 96),
               Case("clip", epi, 0, 7 * 129, 2304, 768), Case("clip", epi, 0, 1025, 384, 64)]
    cs += [Case("wide", 4, 0, 903, n, 64, relu=1, res=True) for n in (32, 64, 96, 128, 160, 192, 288, 384)]
    cs += [Case("wide", 4, 0, 903, 256, 64, relu=1, res=False, K2=128), Case("wide", 5, 0, 2 * 64 * 32, 256, 256, pool_w=32),
           Case("wide", 6, 0, 2 * 32 * 16, 384, 384, pool_w=16)]
    return cs


def _small(kind, epi, param):
    extra = dict(relu=1, res=True) if epi == 4 else {}
    if kind == "256":
        return [Case("256", epi, 0, 257, 512, 192, **extra), Case("256", epi, 0, 1025, 256, 64, **extra)]
    if kind == "glds":
        if epi in (5, 6):
            return [c for c in _pool() if c.epi == epi][:1]
        return [Case("glds", epi, param, 129, 256, 2 * param, **extra), Case("glds", epi, param, 17, 128, param, **extra)]
    return [Case("f16", epi, param, 129, 2 * param, 96, **extra), Case("f16", epi, param, 1, param, 32, **extra)]


FAMILIES = [("256", e, 0, _256(e)) for e in range(5)] + [("glds", e, 64, _glds64(e)) for e in range(4)] + \
           [("f16", e, 128, _f16_128(e)) for e in range(4)] + [("glds", 3, 32, _head()), ("glds", 4, 32, _glds4()),
                                                                ("glds", 5, 32, [c for c in _pool() if c.epi == 5]),
                                                                ("glds", 6, 32, [c for c in _pool() if c.epi == 6])] + \
           [("f16", 4, bn, _f16_4(bn)) for bn in (32, 64, 96)] + [("route", 0, 0, _routes())]


def _run(lib, cases, label):
    out = []
    for regime in ("exact", "random"):
        if regime == "exact" and all(c.epi == 1 for c in cases):
            out.append(f"{label} [exact]: QuickGELU, random regime only")
            continue
        n, emax, rmax = 0, 0.0, 0.0
        for i, c in enumerate(cases):
            if regime == "exact" and c.epi == 1:
                continue
            err, ratio = run_case(lib, c, regime, seed=1000 * i + c.epi)
            n, emax, rmax = n + 1, max(emax, err), max(rmax, ratio)
        out.append(f"{label} [{regime}]: {n} cases " + ("bit-exact" if regime == "exact" else f"max err {emax:.2e}, max err / bound {rmax:.3f}"))
    print("\n".join(out))


@pytest.mark.parametrize("kind,epi,param,cases", [pytest.param(*f, id=f"{f[0]}-{f[1]}-{f[2]}") for f in FAMILIES])
def test_gemm_known_answers(lib, kind, epi, param, cases):
    """every case in both regimes (EPI 1 random only): exact outputs bit-equal, random ones inside the bound, poison overwritten, guard
    rows untouched, no NaN from the poisoned rows beyond M, two launches bit-identical"""
    _run(lib, cases, cases[0].family if kind != "route" else "product dispatch (ClipNet::gemm, WideOsNet::gemm)")


@pytest.mark.parametrize("kind,epi,param", [pytest.param(k, e, p, marks=pytest.mark.fast, id=f"{k}-{e}-{p}")
                                            for k, e, p in (("256", 2, 0), ("glds", 4, 32), ("glds", 5, 32), ("f16", 4, 96), ("glds", 0, 64),
                                                            ("f16", 2, 128))])
def test_gemm_known_answers_small(lib, kind, epi, param):
    """one small case set per kernel kind (the fast tier)"""
    cases = _small(kind, epi, param)
    _run(lib, cases, cases[0].family + " (small)")


def test_product_dispatch_routes(lib):
    """the restated dispatch sends each shape where clip_engine.hpp / osnet_wide.hpp send it (a route test above relies on it)"""
    L = lib.lib
    assert [L.kat_clip_route(m, n, k) for m, n, k in ((1023, 768, 768), (1024, 768, 768), (1024, 384, 768), (4096, 768, 96),
                                                      (10, 768, 100))] == [64, 256, 64, 128, -1]
    assert [L.kat_wide_route(n, k, k2, p) for n, k, k2, p in ((256, 64, 0, 32), (384, 64, 0, 16), (128, 64, 64, 0), (96, 64, 0, 0),
                                                             (320, 64, 0, 0), (160, 64, 0, 0), (96, 64, 32, 0))] == [5, 6, 4, 96, 64, 32, -1]
