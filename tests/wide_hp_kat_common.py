"""Known-answer cases for the fp32-grade wide-OSNet kernels (ReID mode 2 at widths that are multiples of 32:
boxmot_amd/csrc/osnet_wide_hp_kernels.hpp, the packer osnet_wide_hp_pack.hpp) run one kernel at a time through tests/kat/wide_hp_kat.hip:
shared by the device test (test_gpu_wide_hp_kat.py) and its CPU-thread emulation (test_wide_hp_kat_emu.py).  Not a product path.

Layout and operands.  Activations are laid out in the family's "paired" channel order from its definition (inside each block of 32
channels, logical channel 16 p + 4 g + r sits at 8 g + 4 p + r: ``paired_pos``), never from the product's hp_paired_pos.  Every (hi, lo)
input is built as hi = fp16(v), lo = fp16(v - hi) and every reference consumes float64(hi) + float64(lo), so input rounding is no error
source.  Stem and chain weights go to the harness as fp32 in blob order and through the product's wide_pack_hp; the generic GEMM takes
(hi, lo) weight planes [N][K] built here, k columns permuted to the paired order by the definition; ``run_pack`` compares wide_pack_hp's
planes and biases of one small layout with planes built here, bit for bit.

Regimes.
* ``exact``     the indexing and term test, both output planes bit for bit.  Non-zero operands are a (1 + f), |a| in {1, 2}, f in
                {1, 2, 3} * 2**-13: hi = a and lo = a f != 0.  Activations are non-negative, a quarter of them zero; weights mostly positive.
                The expected fp32 value is the THREE-term sum Wh.xh + Wh.xl + Wl.xh in float64 (+ bias, shortcut, ReLU, pool): every term
                is a multiple of 2**-13, so the sum is exact in fp32 in any order while the sum of absolute terms stays below 2**11 -- which
                the builders assert on the reference alone, together with: the FOUR-term product differs in at least half of the owned
                elements of every GEMM case, and at most MAX_ZERO_FRACTION of the owned outputs are zero.  The expected planes are the
                definition's split of that fp32 value.
                k_chain_hp feeds each LightConv's fp32 result to the next 1x1 as a NEW (hi, lo) split, and a layer whose weights have
                lo != 0 multiplies its input's hi by 2**-13 steps: the sum stays exact only while that hi is a short integer.  24 bits do
                not hold that for four layers in a row, so in this regime the records a0, b1, c0, c2, d1, d3 carry lo != 0 weights (every
                depth of a chain at least once -- the 1x1 is ONE loop body for all ten layers) and b0, c1, d0, d2 carry short weights
                with lo = 0 and a bias large enough to make the next layer's hi an integer again; ``chain_inputs`` asserts the exactness
                of every layer's every sum from the operands (``_order_free``).
* ``impulses``  single non-zero elements at placed positions (stem: wide_kat_common's conv rows and columns; chain: corners, wave seams,
                x = 15 / 16, the first and last window row of every band and both sides of every band seam; pooling GEMM: the four
                positions of a 2 x 2 cell on both sides of the seam between two 128-row tiles), channels cycling through the last channel of
                every 16-channel tile first.  Stem and pooling GEMM: exact as well (every output is one three-term sum, or four of them).  Chain:
                an impulse of 4 to 6 on a zero image under the dense regime's weights and positive biases, compared like dense (as
                reid_hp_kat_common's impulses are): the response crosses every seam it sits next to.
* ``dense``     random operands of realistic magnitude against float64 arithmetic on the operands as received, per element against
                band * max|ref64| per crop and tensor; band = 4 x the largest figure measured for the unit (MEASURED: an MI355X and the
                emulation separately), never above reid_hp_kat_common.BAND_CAP = 2e-5.  The gate's sigmoid gets
                wide_kat_common.gate_allowance on top (the same expression as the fp16 kernel's).
In every regime each output pair must be canonical: hi is a nearest fp16 of hi + lo (``canonical``: the identity hi == fp16(fp32(hi) +
fp32(lo)) except that a rounding tie may sit on either neighbour, as the definition's own split puts it).
gap_part is compared with float64 sums of the kernel's own outputs inside (R W + 4) 2**-24 sum |o|, and bit for bit where that sum is exact
in fp32 in any order (`exact`: about a third of the sums; the others exceed 24 bits, R W values of up to 2**10 in steps of 2**-13).

Around every launch (wide_kat_common._protocol): outputs (both planes, gap_part) prefilled with NaN and followed by guards, no NaN among the
owned elements, every launch twice with identical bits, at n = 3 crop 1 alone equal to crop 1 of the batch bit for bit.

Controls (``controls``): wrong references, no kernel runs; each must leave the band or the exact match in every case it applies to.
"""
from __future__ import annotations

import ctypes
import subprocess
from pathlib import Path

import numpy as np

import wide_kat_common as wk
from gemm_kat_common import F16_POISON, F32_POISON, U24
from reid_hp_kat_common import BAND_CAP, FP16_OPERANDS_MIN_BANDS, MAX_ZERO_FRACTION
from wide_kat_common import GUARD, _c, _exact, _protocol, _ptr, _rejects, _within       # _protocol checks through _values; the stem's sheets are wk.stem_sheets (_sheets)

KAT_SRC = Path(__file__).resolve().parent / "kat" / "wide_hp_kat.hip"
REGIMES = ("exact", "impulses", "dense")
LIMIT = 2.0 ** 11                  # sum of absolute terms of an `exact` sum (terms are multiples of 2**-13: 24 bits)
F13 = 2.0 ** -13

# ---------------------------------------------------------------------------------------------------------------------------------
# Measured max|got - ref64| / max|ref64| (per crop and tensor) of the dense regime, largest over every case of the unit, and the
# band = 4 x measured.  "gpu": an MI355X, tests/test_gpu_wide_hp_kat.py; "emu": the CPU-thread emulation on its reduced case list,
# tests/test_wide_hp_kat_emu.py.  A unit without a figure is held to BAND_CAP.  The table at the top of test_gpu_wide_hp_kat.py prints
# measured, band and ratio.
# ---------------------------------------------------------------------------------------------------------------------------------
MEASURED = {
    "gpu": {"stem": 5.631e-07, "gemm": 4.250e-07, "gemm.res": 2.298e-07, "gemm.pool": 1.943e-07, "gemm.f32": 3.232e-07, "chain": 1.034e-06,
            "gate": 2.743e-07, "gap": 6.486e-07},
    "emu": {"stem": 1.247e-06, "gemm": 7.385e-07, "gemm.res": 4.710e-07, "gemm.pool": 3.525e-07, "gemm.f32": 7.578e-07, "chain": 6.284e-07,
            "gate": 1.725e-07, "gap": 6.486e-07},
}
SEEN: dict = {}                    # backend -> unit -> the largest metric this process has seen (noted BEFORE any assertion)


def band(backend: str, unit: str) -> float:
    m = MEASURED[backend].get(unit)
    b = BAND_CAP if m is None else 4 * m
    assert b <= BAND_CAP, f"{unit}: 4 x measured = {b:.2e} exceeds the cap {BAND_CAP:.0e}: a finding to explain, not a constant to raise"
    return b


def report(backend: str):
    for u, m in sorted(SEEN.get(backend, {}).items()):
        have = MEASURED[backend].get(u)
        print(f"MEASURED {backend} {u:10s} {m:.3e}" + (f"   table {have:.3e}, band {4 * have:.3e}, ratio {m / (4 * have):.3f}" if have else "   no table entry yet"))


# ---------------------------------------------------------------------------------------------------------------------------------
# build, ctypes
# ---------------------------------------------------------------------------------------------------------------------------------
def build_gpu(out_dir: Path, extra_flags=(), timeout: float = 900) -> Path:
    """hipcc for gfx950 with the product's flags (__graft_entry__.HIPCC_FLAGS) -> out_dir/libwide_hp_kat.so"""
    from __graft_entry__ import HIPCC_FLAGS

    out = Path(out_dir) / "libwide_hp_kat.so"
    subprocess.run(["hipcc", *HIPCC_FLAGS, *extra_flags, "-o", str(out), str(KAT_SRC)], check=True, timeout=timeout)
    return out


def build_emu(clang: str, out_dir: Path, extra_flags=(), timeout: float = 600) -> Path:
    """the same source on CPU threads (tests/host_emu/hip_shim.hpp), built as wide_kat_common.build_emu builds its harness"""
    out = Path(out_dir) / "libwide_hp_kat_emu.so"
    subprocess.run([clang, "-x", "c++", "-std=c++17", "-O1", "-fPIC", "-shared", "-pthread", "-ffp-contract=off", "-DKAT_EMU",
                    "-DEMU_DEFER_GLDS=1", *extra_flags, "-o", str(out), str(KAT_SRC)], check=True, timeout=timeout)
    return out


class WideHpKatLib:
    """ctypes face of wide_hp_kat.hip's entry points"""

    def __init__(self, path, backend: str):
        self.backend = backend
        self.lib = L = ctypes.CDLL(str(path))
        p, i, l = ctypes.c_void_p, ctypes.c_int, ctypes.c_long
        L.kat_hp_stem.argtypes = [i, p, p, l, i, p, p, p, p, l]
        L.kat_hp_gemm.argtypes = [i, i, i, p, p, l, p, p, p, p, p, l, p, p, l, i, i, i, i, p, p, l, p, p, i]
        L.kat_hp_chain_geo.argtypes = [i, i, i, i, p]
        L.kat_hp_chain.argtypes = [i, i, i, i, p, p, l, i, i, p, p, p, l, p, l]
        L.kat_hp_gate.argtypes = [i, p, p, p, p, p, p, p, p, p, l, i, i, i]
        L.kat_hp_gap.argtypes = [p, p, p, p, l, i, i, i]
        L.kat_hp_pack.argtypes = [p, i, p, l, p, l, p]
        L.kat_hp_layout.argtypes = [p, i, p]
        for f in (L.kat_hp_stem, L.kat_hp_gemm, L.kat_hp_chain_geo, L.kat_hp_chain, L.kat_hp_gate, L.kat_hp_gap):
            f.restype = ctypes.c_int
        L.kat_hp_pack.restype = ctypes.c_long
        L.kat_hp_layout.restype = ctypes.c_long


# ---------------------------------------------------------------------------------------------------------------------------------
# the paired order, (hi, lo) pairs, comparisons
# ---------------------------------------------------------------------------------------------------------------------------------
def paired_pos(C: int) -> np.ndarray:
    """stored position of logical channel c: inside each block of 32, channel 16 p + 4 g + r sits at 8 g + 4 p + r"""
    c = np.arange(C)
    blk, w = c // 32, c % 32
    p, g, r = w // 16, (w % 16) // 4, w % 4
    return 32 * blk + 8 * g + 4 * p + r


def to_paired(a: np.ndarray) -> np.ndarray:
    out = np.empty_like(a)
    out[..., paired_pos(a.shape[-1])] = a
    return out


def from_paired(s: np.ndarray) -> np.ndarray:
    return s[..., paired_pos(s.shape[-1])]


def split(v):
    """the definition: hi = fp16(v), lo = fp16(v - hi) in fp32"""
    v32 = np.asarray(v, np.float32)
    hi = v32.astype(np.float16)
    return hi, (v32 - hi.astype(np.float32)).astype(np.float16)


def join(hi, lo) -> np.ndarray:
    return hi.astype(np.float64) + lo.astype(np.float64)


def hl_form(rng, shape, mags=(1.0, 2.0), p_zero=0.0, p_neg=0.0) -> np.ndarray:
    """a (1 + f): |a| from mags, f in {1, 2, 3} * 2**-13; float64 values that fp32 holds, every non-zero one with lo != 0"""
    v = rng.choice(np.asarray(mags, np.float64), shape) * (1.0 + rng.integers(1, 4, shape) * F13)
    v = np.where(rng.random(shape) < p_neg, -v, v)
    v = np.where(rng.random(shape) < p_zero, 0.0, v)
    h, l = split(v)
    assert np.array_equal(join(h, l), v) and np.all((l != 0) == (v != 0))
    return v


def _bits(a, dt):
    return _c(a, dt).view(np.uint16 if dt == np.float16 else np.uint32).ravel()


def _poisoned(valid: int, f32: bool = False) -> np.ndarray:
    return np.full(valid + GUARD, F32_POISON if f32 else F16_POISON, np.uint32 if f32 else np.uint16)


def _with_tail(bits: np.ndarray, tail: int) -> np.ndarray:
    """an input followed by `tail` NaNs: nothing may read past its last element"""
    out = np.full(bits.size + tail, F16_POISON, np.uint16)
    out[:bits.size] = bits
    return out


def canonical(h: np.ndarray, l: np.ndarray) -> np.ndarray:
    """hi is A nearest fp16 of hi + lo.  The plain identity hi == fp16(fp32(hi) + fp32(lo)) holds for the definition's split except on a tie:
    v = 0x3f2f1001 (one fp32 step past the midpoint of two fp16 numbers) gives hi = the upper one and lo = fp16(v - hi) = exactly minus half
    a step, and fp16(hi + lo) then rounds the midpoint to the EVEN neighbour, the lower one (seen in k_wide_gap_hp's dense case, 1 pair in
    4224).  So a tie passes here when |lo| is exactly half a step of hi, and everything else is held to the identity."""
    h16 = h.astype(np.float16)
    s = h + l
    up = np.nextafter(h16, np.float16(np.inf)).astype(np.float64)
    dn = np.nextafter(h16, np.float16(-np.inf)).astype(np.float64)
    d = np.abs(s - h)
    return (d <= np.abs(s - up)) & (d <= np.abs(s - dn))


def _pair(what: str, o: dict, name: str, shape, paired=True):
    """the two planes of an output as logical-order float64 arrays; asserts the pair is canonical"""
    h, l = o[name + "_h"].reshape(shape), o[name + "_l"].reshape(shape)
    bad = ~canonical(h, l)
    assert not bad.any(), f"{what}: {int(bad.sum())} output pairs are not canonical (hi is no nearest fp16 of hi + lo), first at {tuple(np.argwhere(bad)[0])}"
    return (from_paired(h), from_paired(l)) if paired else (h, l)


def _exact_pair(what: str, gh, gl, want64):
    """both planes bit for bit against the definition's split of the expected value, which fp32 must hold"""
    w32 = want64.astype(np.float32)
    assert np.array_equal(w32.astype(np.float64), want64), f"{what}: the expected value is no fp32 number (a mistake in the case)"
    wh, wl = split(w32)
    _exact(what + " hi plane", gh, wh.astype(np.float64))
    _exact(what + " lo plane", gl, wl.astype(np.float64))


def _zero_fraction(what: str, want64):
    z = float((want64 == 0).mean())
    assert z <= MAX_ZERO_FRACTION, f"{what}: {z:.2f} of the owned outputs are zero (ReLU blind spots), limit {MAX_ZERO_FRACTION}"


def _banded(what: str, backend: str, unit: str, got, ref, crop_axes=None, extra=None):
    """per element against band * max|ref| per crop (crop_axes: the axes that are NOT the crop axis, None: one tensor); notes the measured
    figure before it asserts"""
    scale = np.abs(ref).max(axis=crop_axes, keepdims=True) if crop_axes else np.abs(ref).max()
    scale = np.maximum(scale, 2.0 ** -126)
    err = np.abs(got - ref.reshape(got.shape))
    m = float((err / scale).max())
    if extra is not None:           # an absolute allowance per element on top of the band (the measured figure does not know of it)
        err = np.maximum(err - extra, 0.0)
    d = SEEN.setdefault(backend, {})
    d[unit] = max(d.get(unit, 0.0), m)
    b = band(backend, unit)
    print(f"{what}: max|got - ref64| / max|ref64| = {m:.3e}, band {b:.3e}, ratio {m / b:.3f}")
    over = err > b * scale
    if over.any():
        i = tuple(np.argwhere(over)[0])
        raise AssertionError(f"{what}: {int(over.sum())} of {over.size} outputs outside the band, first at {i}: got {got[i]!r} want {ref.reshape(got.shape)[i]!r} "
                             f"err {err[i]:.3e} > {b:.3e} x {np.broadcast_to(scale, got.shape)[i]:.3e}")
    return m


def _lowbit(a: np.ndarray) -> np.ndarray:
    """the largest power of two that divides each float64 element (inf for 0)"""
    m, e = np.frexp(np.abs(a))
    M = (m * 2.0 ** 53).astype(np.int64)
    low = np.where(M != 0, M & -M, 1).astype(np.float64)
    return np.where(a != 0, np.ldexp(low, e - 53), np.inf)


def _order_free(what: str, abs_sum: np.ndarray, quantum: np.ndarray):
    """an fp32 sum is exact in ANY order when every term is a multiple of `quantum` and the sum of absolute terms is at most 2**24 quanta:
    every partial sum is then such a multiple, too"""
    bad = abs_sum > 2.0 ** 24 * quantum
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} sums are not exact in fp32 in every order (a mistake in the case), first at {tuple(np.argwhere(bad)[0])}"


# ---------------------------------------------------------------------------------------------------------------------------------
# k_gemm_hp<EPI, BN, DB>
# ---------------------------------------------------------------------------------------------------------------------------------
GEMM_M = (1, 3, 127, 128, 129, 257)
GEMM_K = (32, 64, 96)


def gemm_inputs(regime: str, epi: int, M: int, N: int, K: int, seed: int, K2: int = 0, relu: int = 1, bias: bool = True, pool=None, p_neg: float = 0.3):
    """pool = (n, H, W) of the image under EPI 2 / 3 (M = n H W).  Logical-order float64 operands that fp32 holds."""
    rng = np.random.default_rng(seed)
    d = dict(epi=epi, M=M, N=N, K=K, K2=K2, relu=relu, pool=pool, regime=regime)
    if regime == "dense":       # conv1 / conv3 of a calibrated network: activations of order 1 (a quarter zero), weights of order 1 / sqrt(K)
        def act(k):
            return np.where(rng.random((M, k)) < 0.25, 0.0, np.abs(rng.standard_normal((M, k)))).astype(np.float32).astype(np.float64)
        d["X"] = act(K)
        d["W"] = (rng.standard_normal((N, K)) / np.sqrt(K + K2)).astype(np.float32).astype(np.float64)
        if K2:
            d["X2"] = act(K2)
            d["W2"] = (rng.standard_normal((N, K2)) / np.sqrt(K + K2)).astype(np.float32).astype(np.float64)
        b1 = (rng.standard_normal(N) * 0.3).astype(np.float32)
        b2 = (rng.standard_normal(N) * 0.3).astype(np.float32)
        res = act(N) if epi == 1 else None
    else:
        if regime == "impulses":
            d["X"] = np.zeros((M, K))
        else:
            d["X"] = hl_form(rng, (M, K), p_zero=0.25)
        # 30 % negative weights: a few per cent of the pre-activations are negative and most sums stay large enough for the dropped lo.lo
        # term to show in fp32; the pooling cases take 45 %, so that the place of ReLU before the pool shows as well
        d["W"] = hl_form(rng, (N, K), p_neg=p_neg)
        if K2:
            d["X2"] = hl_form(rng, (M, K2), p_zero=0.25)
            d["W2"] = hl_form(rng, (N, K2), p_neg=p_neg)
        frac = rng.integers(0, 4, N) * F13
        b1 = (rng.integers(-6, 7, N) + frac).astype(np.float32)
        b2 = (rng.integers(-3, 4, N) + rng.integers(0, 4, N) * F13).astype(np.float32)
        res = hl_form(rng, (M, N), p_zero=0.25) if epi == 1 else None
        if regime == "impulses":
            b1[:], b2[:] = 0.0, 0.0
    # a block with a downsample carries conv3's and the downsample's biases summed in fp32 (wide_pack_hp)
    d["bias_conv3"] = b1.astype(np.float64) if bias else None
    d["bias"] = ((b1 + b2) if K2 else b1).astype(np.float64) if bias else None
    d["res"] = res
    return d


def gemm_reference(d, terms=3, w_fp16=False, k_logical=False, bias_wo_down=False, pool_rows12=False, relu_after_pool=False, abs_sum=False):
    """logical-order float64 result.  terms: 3 = what the kernel computes exactly (Wh.xh + Wh.xl + Wl.xh), 4 = the product of the operands as
    received, 2 = Wl.xh missing.  The other flags are the controls' mistakes.  abs_sum: the sum of absolute terms instead (the exactness limit)."""
    def prod(X, W):
        xh, xl = (a.astype(np.float64) for a in split(X))
        wh, wl = (a.astype(np.float64) for a in split(W))
        if k_logical:               # the weights' k columns left in logical order against activations stored in the paired order
            xh, xl = to_paired(xh), to_paired(xl)
        if w_fp16:
            wl = np.zeros_like(wl)
        if abs_sum:
            xh, xl, wh, wl = np.abs(xh), np.abs(xl), np.abs(wh), np.abs(wl)
        acc = xh @ wh.T + xl @ wh.T
        if terms >= 3:
            acc += xh @ wl.T
        if terms == 4:
            acc += xl @ wl.T
        return acc
    v = prod(d["X"], d["W"])
    if d["K2"]:
        v = v + prod(d["X2"], d["W2"])
    b = d["bias_conv3"] if bias_wo_down else d["bias"]
    if b is not None:
        v = v + (np.abs(b) if abs_sum else b)
    if d["res"] is not None:
        v = v + d["res"]
    if d["pool"] is None:
        return np.maximum(v, 0.0) + 0.0 if d["relu"] and not abs_sum else v
    n, H, Wi = d["pool"]
    v = v.reshape(n, H, Wi, -1)
    if not relu_after_pool and not abs_sum:
        v = np.maximum(v, 0.0)
    if pool_rows12:                 # rows (1, 2), (3, 4) .. paired instead of (0, 1), (2, 3) ..
        v = np.roll(v, -1, axis=1)
    p = v[:, 0::2, 0::2] + v[:, 0::2, 1::2] + v[:, 1::2, 0::2] + v[:, 1::2, 1::2]
    p = p if abs_sum else 0.25 * p
    if relu_after_pool:
        p = np.maximum(p, 0.0)
    return p.reshape(n * (H // 2) * (Wi // 2), -1) + 0.0


def gemm_check_case(what: str, d):
    """the conditions on an `exact` / `impulses` case, from the reference alone"""
    s = gemm_reference(d, abs_sum=True)
    assert s.max() < LIMIT, f"{what}: sum of absolute terms {s.max()} reaches 2**11 (a mistake in the case)"
    want = gemm_reference(d)
    if d["regime"] == "exact":
        four = gemm_reference(d, terms=4).astype(np.float32).astype(np.float64)
        frac = float((four != want).mean())
        assert frac >= 0.5, f"{what}: the four-term product differs from the three-term sum in only {frac:.2f} of the outputs"
        _zero_fraction(what, want)
    return want


def gemm_launch(lib: WideHpKatLib, d, bn: int, db: int):
    epi, M, N, K, K2 = d["epi"], d["M"], d["N"], d["K"], d["K2"]

    def planes(a, tail=0):          # [rows][k] logical -> (hi, lo) bits, k in the paired order
        h, l = split(to_paired(a))
        return _with_tail(_bits(h, np.float16), tail), _with_tail(_bits(l, np.float16), tail)
    xh, xl = planes(d["X"], GUARD)
    wh, wl = planes(d["W"])
    x2h = x2l = w2h = w2l = None
    if K2:
        x2h, x2l = planes(d["X2"], GUARD)
        w2h, w2l = planes(d["W2"])
    rh = rl = None
    if d["res"] is not None:
        rh, rl = planes(d["res"], GUARD)
    bias = None if d["bias"] is None else _c(d["bias"], np.float32)
    rows = M // 4 if d["pool"] else M
    valid = rows * N
    per = valid // d["pool"][0] if d["pool"] else 0
    oh = _poisoned(valid, epi == 4)
    ol = None if epi == 4 else _poisoned(valid)
    st = lib.lib.kat_hp_gemm(epi, bn, db, _ptr(xh), _ptr(xl), xh.size, _ptr(wh), _ptr(wl), _ptr(bias), _ptr(oh), _ptr(ol), oh.size, _ptr(rh), _ptr(rl),
                             0 if rh is None else rh.size, M, N, K, d["relu"], _ptr(x2h), _ptr(x2l), 0 if x2h is None else x2h.size, _ptr(w2h), _ptr(w2l), K2)
    assert st == 0, f"k_gemm_hp<{epi}, {bn}, {db}> M={M} N={N} K={K} K2={K2}: launch status {st}"
    if epi == 4:
        return {"out": (oh, valid, per)}
    return {"out_h": (oh, valid, per), "out_l": (ol, valid, per)}


def gemm_crop(d, i):
    n, H, Wi = d["pool"]
    r = slice(i * H * Wi, (i + 1) * H * Wi)
    return dict(d, M=H * Wi, pool=(1, H, Wi), X=d["X"][r], res=None)


def gemm_unit(epi: int) -> str:
    return {0: "gemm", 1: "gemm.res", 2: "gemm.pool", 3: "gemm.pool", 4: "gemm.f32"}[epi]


def run_gemm(lib: WideHpKatLib, d, bn: int, db: int, also_db=None):
    """one case through k_gemm_hp<epi, bn, db>; also_db: the same inputs through the other buffering form must give the same bits"""
    epi, N = d["epi"], d["N"]
    what = f"k_gemm_hp<{epi}, {bn}, {db}> M={d['M']} N={N} K={d['K']} K2={d['K2']} relu={d['relu']} bias={d['bias'] is not None} pool={d['pool']} [{d['regime']}]"
    n = d["pool"][0] if d["pool"] else 1
    raw = {}

    def launch(i):
        r = gemm_launch(lib, i, bn, db)
        raw.setdefault("first", r)
        return r
    o = _protocol(what, launch, d, n, gemm_crop)
    if also_db is not None:
        other = gemm_launch(lib, d, bn, also_db)
        for k, v in other.items():
            assert np.array_equal(v[0], raw["first"][k][0]), f"{what}: the DB = {db} and DB = {also_db} forms differ in {k}"
    rows = d["M"] // 4 if d["pool"] else d["M"]
    if epi == 4:
        got = o["out"].reshape(rows, N)
        gh = gl = None
    else:
        gh, gl = _pair(what, o, "out", (rows, N))
        got = gh + gl
    if d["regime"] == "dense":
        ref = gemm_reference(d, terms=4)
        ca = None
        if d["pool"]:
            got, ref, ca = got.reshape(n, -1), ref.reshape(n, -1), 1
        return _banded(what, lib.backend, gemm_unit(epi), got, ref, ca)
    want = gemm_check_case(what, d)
    if epi == 4:
        _exact(what, got, want, f32=True)
    else:
        _exact_pair(what, gh, gl, want)
    return 0.0


def pool_impulse_rows(H: int, Wi: int, n: int):
    """image positions (crop, y, x) of the impulses of a pooling case: the four positions of the 2 x 2 cells next to every seam between two 128-row
    tiles of the GEMM (row m = (crop H + y) Wi + x), at the first, a middle and the last cell column; without a seam, the first and last cell rows"""
    per_tile = 128 // Wi
    ys = set()
    for m in range(per_tile, n * H, per_tile):          # global image row at which a tile starts
        for yy in (m - 2, m - 1, m, m + 1):
            ys.add(yy)
    ys |= {0, 1, n * H - 2, n * H - 1}
    out = []
    for gy in sorted(ys):
        for x0 in (0, Wi // 2 - 2, Wi - 2):
            for dx in (0, 1):
                out.append((gy // H, gy % H, x0 + dx))
    return out


def gemm_pool_inputs(regime: str, epi: int, n: int, H: int, seed: int, K: int = 64, N: int = 128):
    Wi = 32 if epi == 2 else 16
    d = gemm_inputs(regime, epi, n * H * Wi, N, K, seed, pool=(n, H, Wi), p_neg=0.45)
    if regime == "impulses":
        # every impulse row has ONE non-zero k: the outputs of its cell are single products (x 0.25), different per position of the cell
        tiles_last = [16 * t + 15 for t in range(K // 16)]
        order = tiles_last + [k for k in range(K) if k not in tiles_last]
        X = d["X"].reshape(n, H, Wi, K)
        vals = hl_form(np.random.default_rng(seed + 1), (4096,))
        for j, (c, y, x) in enumerate(pool_impulse_rows(H, Wi, n)):
            X[c, y, x, order[j % K]] = vals[j]
    return d


GEMM_INST = tuple((0, bn, db) for bn in (32, 64, 96, 128) for db in (1, 2)) + tuple((e, 128, 2) for e in (1, 2, 3, 4))


def gemm_cases(epi: int, bn: int, Ms=GEMM_M, Ks=GEMM_K):
    """(M, N, K, relu, bias) of the common shapes: every M x K x N in {BN, 2 BN}, ReLU and the bias each on and off"""
    out = []
    for M in Ms:
        for K in Ks:
            for N in (bn, 2 * bn):
                for relu in (0, 1):
                    for bias in (False, True):
                        out.append((M, N, K, relu, bias))
    return out


def run_gemm_common(lib: WideHpKatLib, epi: int, bn: int, db: int, regime: str, Ms=GEMM_M, Ks=GEMM_K, seed: int = 0):
    """the common shapes of one instantiation; <0, BN, 1> also runs <0, BN, 2> on the same inputs: identical bits.  EPI 0 adds the second
    operand pair (K2 in {32, 96} at K != K2) and, at BN = 128, M = 257 x N = 512: unequal tile counts in both directions."""
    for i, (M, N, K, relu, bias) in enumerate(gemm_cases(epi, bn, Ms, Ks)):
        run_gemm(lib, gemm_inputs(regime, epi, M, N, K, seed + i, relu=relu, bias=bias), bn, db, also_db=2 if db == 1 else None)
    if epi == 0:
        for i, (M, K, K2) in enumerate(((129, 64, 32), (257, 32, 96), (3, 96, 32), (128, 64, 96))):
            if M in Ms or len(Ms) == len(GEMM_M):
                run_gemm(lib, gemm_inputs(regime, 0, M, bn, K, seed + 500 + i, K2=K2), bn, db, also_db=2 if db == 1 else None)
    if bn == 128 and len(Ms) == len(GEMM_M):
        run_gemm(lib, gemm_inputs(regime, epi, 257, 512, 64, seed + 600), bn, db, also_db=2 if db == 1 else None)


def run_gemm_pool(lib: WideHpKatLib, epi: int, regime: str, ns=(1, 3), seed: int = 0):
    for H in ((4, 8) if epi == 2 else (8, 16)):
        for n in ns:
            run_gemm(lib, gemm_pool_inputs(regime, epi, n, H, seed + H + n), 128, 2)


# ---------------------------------------------------------------------------------------------------------------------------------
# wide_pack_hp: the GEMM planes and biases of one small layout, bit for bit
# ---------------------------------------------------------------------------------------------------------------------------------
PACK_LAYOUT = ((32, 128, 128, 128), 128)


def run_pack(lib: WideHpKatLib, seed: int = 0):
    """Every GEMM operand of the layout: planes [N][K] with the k columns in the paired order (stored column paired_pos(c) holds logical column
    c), the definition's split; biases as they are, conv3's with the downsample's added in fp32 where the block has one.  Block 0 (32 -> 128)
    has a downsample, the others have none."""
    ch, feat = PACK_LAYOUT
    chv = np.asarray(ch, np.int32)
    lay = np.zeros(58, np.int64)
    total = lib.lib.kat_hp_layout(_ptr(chv), feat, _ptr(lay))
    rng = np.random.default_rng(seed)
    blob = rng.standard_normal(total).astype(np.float32)
    offs = np.zeros(68, np.int64)
    size = lib.lib.kat_hp_pack(_ptr(chv), feat, _ptr(blob), total, None, 0, _ptr(offs))
    assert size > 0, f"wide_pack_hp: status {size}"
    data = np.zeros(size, np.uint8)
    assert lib.lib.kat_hp_pack(_ptr(chv), feat, _ptr(blob), total, _ptr(data), size, _ptr(offs)) == size
    checked = 0

    def planes(name, o_h, o_l, w_off, N, K):
        nonlocal checked
        w = blob[w_off:w_off + N * K].reshape(N, K)
        h, l = split(to_paired(w))
        for plane, o, want in (("hi", o_h, h), ("lo", o_l, l)):
            assert o >= 0 and o % 16 == 0, f"wide_pack_hp {name}: {plane} plane at offset {o}"
            got = data[o:o + N * K * 2].view(np.uint16).reshape(N, K)
            bad = got != want.view(np.uint16)
            assert not bad.any(), f"wide_pack_hp {name}: {int(bad.sum())} of {bad.size} elements of the {plane} plane differ, first at {tuple(np.argwhere(bad)[0])}"
        checked += 1

    def biases(name, o, want):
        got = data[o:o + want.size * 4].view(np.float32)
        assert np.array_equal(got.view(np.uint32), want.astype(np.float32).view(np.uint32)), f"wide_pack_hp {name}: the bias differs"
    downs = 0
    for b in range(6):
        c1w, c1b, c3w, c3b, dnw, dnb, cin, mid = (int(v) for v in lay[8 * b:8 * b + 8])
        cout = 4 * mid
        o = offs[9 * b:9 * b + 9]
        planes(f"block {b} conv1", o[0], o[1], c1w, mid, cin)
        biases(f"block {b} conv1", o[2], blob[c1b:c1b + mid])
        planes(f"block {b} conv3", o[3], o[4], c3w, cout, mid)
        if dnw >= 0:
            downs += 1
            planes(f"block {b} downsample", o[6], o[7], dnw, cout, cin)
            biases(f"block {b} conv3 + downsample", o[5], blob[c3b:c3b + cout] + blob[dnb:dnb + cout])
        else:
            assert o[6] < 0 and o[7] < 0
            biases(f"block {b} conv3", o[5], blob[c3b:c3b + cout])
    assert downs == 1
    t = lay[48:58]
    for i, (name, N, K) in enumerate((("transition 0", ch[1], ch[1]), ("transition 1", ch[2], ch[2]), ("conv5", ch[3], ch[3]), ("fc", feat, ch[3]))):
        planes(name, offs[54 + 3 * i], offs[55 + 3 * i], int(t[2 * i]), N, K)
        biases(name, offs[56 + 3 * i], blob[int(t[2 * i + 1]):int(t[2 * i + 1]) + N])
    return checked


# ---------------------------------------------------------------------------------------------------------------------------------
# k_wide_stem_hp<C0>: conv 7x7 / 2, pad 3 + bias + ReLU + max pool 3x3 / 2, pad 1 on (hi, lo) [n][262][136][4] -> (hi, lo) [n][64 * 32][C0]
# ---------------------------------------------------------------------------------------------------------------------------------
SR, SC = wk.SR, wk.SC


def stem_inputs(c0: int, regime: str, n: int, seed: int):
    rng = np.random.default_rng(seed)
    x = np.zeros((n, SR, SC, 4))
    core = (n, 256, 128, 3)
    if regime == "exact":       # 147 products of at most 2.01 x 2.01 and a bias below 8: far inside the limit
        x[:, 3:259, 3:131, :3] = hl_form(rng, core, p_zero=0.25)
        w = hl_form(rng, (c0, 7, 7, 3), p_neg=0.3)
        bias = (rng.integers(-6, 7, c0) + rng.integers(0, 4, c0) * F13).astype(np.float64)
    elif regime == "dense":     # normalised pixels, a folded-BN 7x7
        x[:, 3:259, 3:131, :3] = rng.standard_normal(core).astype(np.float32)
        w = (rng.standard_normal((c0, 7, 7, 3)) / np.sqrt(147.0)).astype(np.float32).astype(np.float64)
        bias = rng.standard_normal(c0).astype(np.float32).astype(np.float64)
    else:
        # positive weights b (1 + f) with b in eighths, the centre tap the largest: an impulse at padded pixel (2 cy + 3, 2 cx + 3) puts its conv
        # maximum on (cy, cx); every conv value is one three-term sum of a few bits
        w = hl_form(rng, (c0, 7, 7, 3), mags=np.arange(4, 13) / 8.0)
        w[:, 3, 3, :] = hl_form(rng, (c0, 3), mags=np.arange(16, 25) / 8.0)
        bias = np.zeros(c0)
        sheets = wk.stem_sheets()
        use = sheets[:3] if n == 3 else sheets[3:4]
        vals = hl_form(rng, (256,), mags=(1.0, 2.0, 0.5, 4.0))
        k = 0
        for i, sheet in enumerate(use):
            for cy, cx in sheet:
                x[i, 2 * cy + 3, 2 * cx + 3, k % 3] = vals[k]
                k += 1
        assert k > 0
    return dict(n=n, x=x, w=w, bias=bias, regime=regime)


def stem_crop(inp, i):
    return dict(inp, n=1, x=inp["x"][i:i + 1])


def stem_conv(inp, terms=3, ignore_lo=False, abs_sum=False):
    """float64 conv + bias (+ ReLU) on [n][128][64][c0]: terms = 3 the kernel's exact sum, 4 the product of the operands as received"""
    xh, xl = (a.astype(np.float64)[..., :3] for a in split(inp["x"]))
    wh, wl = (a.astype(np.float64) for a in split(inp["w"]))
    if ignore_lo:
        xl = np.zeros_like(xl)
    b = inp["bias"]
    if abs_sum:
        xh, xl, wh, wl, b = np.abs(xh), np.abs(xl), np.abs(wh), np.abs(wl), np.abs(b)
    conv = np.zeros((xh.shape[0], 128, 64, wh.shape[0])) + b
    for ky in range(7):
        for kx in range(7):
            ph, pl = xh[:, ky:ky + 256:2, kx:kx + 128:2], xl[:, ky:ky + 256:2, kx:kx + 128:2]
            conv += ph @ wh[:, ky, kx].T + pl @ wh[:, ky, kx].T + ph @ wl[:, ky, kx].T
            if terms == 4:
                conv += pl @ wl[:, ky, kx].T
    return conv if abs_sum else np.maximum(conv, 0.0) + 0.0


def stem_reference(inp, **kw):
    drop = kw.pop("drop_tile_left", False)
    r = stem_conv(inp, **kw)
    return wk.stem_pool(r, drop).reshape(r.shape[0], 2048, r.shape[3])


def stem_launch(lib: WideHpKatLib, c0: int, inp):
    n = inp["n"]
    xh, xl = split(inp["x"])
    xh, xl = _with_tail(_bits(xh, np.float16), SR * SC * 4), _with_tail(_bits(xl, np.float16), SR * SC * 4)     # one crop's worth of NaNs after the last crop
    valid = n * 2048 * c0
    oh, ol = _poisoned(valid), _poisoned(valid)
    w, bias = _c(inp["w"], np.float32), _c(inp["bias"], np.float32)
    st = lib.lib.kat_hp_stem(c0, _ptr(xh), _ptr(xl), xh.size, n, _ptr(w), _ptr(bias), _ptr(oh), _ptr(ol), oh.size)
    assert st == 0, f"k_wide_stem_hp<{c0}>: launch status {st}"
    return {"out_h": (oh, valid, 2048 * c0), "out_l": (ol, valid, 2048 * c0)}


def run_stem(lib: WideHpKatLib, c0: int, regime: str, n: int, seed: int = 0):
    what = f"k_wide_stem_hp<{c0}> [{regime}] n={n}"
    inp = stem_inputs(c0, regime, n, seed)
    x = inp["x"]
    assert not x[:, :3].any() and not x[:, 259:].any() and not x[:, :, :3].any() and not x[:, :, 131:].any() and not x[..., 3].any()
    assert split(x)[1].any(), "the crops' lo plane is empty"
    o = _protocol(what, lambda i: stem_launch(lib, c0, i), inp, n, stem_crop)
    gh, gl = _pair(what, o, "out", (n, 2048, c0))
    if regime == "dense":
        return _banded(what, lib.backend, "stem", gh + gl, stem_reference(inp, terms=4), (1, 2))
    assert stem_conv(inp, abs_sum=True).max() < LIMIT
    want = stem_reference(inp)
    if regime == "impulses":
        assert (want > 0).any() and (want == 0).any()
    else:
        _zero_fraction(what, want)
    _exact_pair(what, gh, gl, want)
    return 0.0


# ---------------------------------------------------------------------------------------------------------------------------------
# k_gate_sum4_hp<C>: out = sum_b y_b * sigmoid(fc2(relu(fc1(sum_bands gap_part[b] / P)))), y and out (hi, lo) in the paired order, gap_part
# and the gate's weights in logical order
# ---------------------------------------------------------------------------------------------------------------------------------
GATE_CASES = ((128, 1), (512, 4), (136, 2))


def gate_inputs(C: int, P: int, nbands: int, regime: str, n: int, seed: int):
    d = wk.gate_inputs(C, P, nbands, "exact" if regime == "exact" else "random", n, seed)
    rng = np.random.default_rng(seed + 1000)
    if regime == "exact":       # gates are 0, 0.5 or 1: four terms of at most 2.01 each, multiples of 2**-14
        d["x"] = hl_form(rng, (4, n, P, C), p_zero=0.25)
    else:                       # branch outputs: post-ReLU, order 1
        d["x"] = np.where(rng.random((4, n, P, C)) < 0.25, 0.0, np.abs(rng.standard_normal((4, n, P, C)))).astype(np.float32).astype(np.float64)
    d["regime"] = regime
    return d


def gate_crop(inp, i):
    return dict(inp, n=1, x=inp["x"][:, i:i + 1], gap=inp["gap"][:, i:i + 1])


def gate_reference(inp, dg: float = 0.0, swap_gates=False, logical_gate=False, **wrong):
    """out [n][P][C] in float64 on x = hi + lo, and the part of the error the sigmoid's allowance explains: sum_b |x_b| dg.
    Controls: swap_gates exchanges the GATES of branches 1 and 2; logical_gate applies to the value stored at position s the gate of logical
    channel s instead of the channel stored there; wrong: wide_kat_common.gate_values's (mean_over_bands)."""
    g, _, v = wk.gate_values(inp, 0.0, **wrong)
    if swap_gates:
        g = g[[0, 2, 1, 3]]
    if logical_gate:
        g = from_paired(g)          # the value of channel c, stored at paired_pos(c), meets the gate of LOGICAL channel paired_pos(c)
    x = join(*split(inp["x"]))
    out = (x * g[:, :, None, :]).sum(axis=0) + 0.0
    return out, dg * np.abs(x).sum(axis=0), v


def gate_launch(lib: WideHpKatLib, inp):
    n, P, nb = inp["n"], inp["P"], inp["nbands"]
    C = inp["x"].shape[-1]
    yh, yl = split(to_paired(inp["x"]))
    yh, yl = _with_tail(_bits(yh, np.float16), GUARD), _with_tail(_bits(yl, np.float16), GUARD)
    valid = n * P * C
    oh, ol = _poisoned(valid), _poisoned(valid)
    gap = _c(inp["gap"], np.float32)
    f = [_c(inp[k], np.float32) for k in ("fc1_w", "fc1_b", "fc2_w", "fc2_b")]
    st = lib.lib.kat_hp_gate(C, _ptr(yh), _ptr(yl), _ptr(gap), *[_ptr(a) for a in f], _ptr(oh), _ptr(ol), oh.size, P, nb, n)
    assert st == 0, f"k_gate_sum4_hp<{C}>: launch status {st}"
    return {"out_h": (oh, valid, P * C), "out_l": (ol, valid, P * C)}


def run_gate(lib: WideHpKatLib, C: int, P: int, nbands: int, regime: str, n: int, seed: int = 0):
    what = f"k_gate_sum4_hp<{C}> P={P} nbands={nbands} [{regime}] n={n}"
    inp = gate_inputs(C, P, nbands, regime, n, seed)
    o = _protocol(what, lambda i: gate_launch(lib, i), inp, n, gate_crop)
    gh, gl = _pair(what, o, "out", (n, P, C))
    if regime == "exact":
        v = wk.gate_values(inp)[2]
        assert (np.abs(v[v != 0]) >= 200).all() and (v == 0).any() and (v > 0).any() and (v < 0).any()
        g = np.where(v > 0, 1.0, np.where(v < 0, 0.0, 0.5))      # fp32: exp(-200) + 1 = 1, exp(200) = inf and 1 / inf = 0
        want = (inp["x"] * g[:, :, None, :]).sum(axis=0) + 0.0
        _zero_fraction(what, want)
        _exact_pair(what, gh, gl, want)
        return 0.0
    ref, allow, _ = gate_reference(inp, wk.gate_allowance(lib.backend))
    return _banded(what, lib.backend, "gate", gh + gl, ref, (1, 2), extra=allow)


# ---------------------------------------------------------------------------------------------------------------------------------
# k_wide_gap_hp: out[n][c] = split(sum_p (hi + lo)[n][p][c] / P): elementwise in the channel, so the order is whatever the input has
# ---------------------------------------------------------------------------------------------------------------------------------
def run_gap(lib: WideHpKatLib, C: int, P: int, regime: str, n: int, seed: int = 0):
    what = f"k_wide_gap_hp C={C} P={P} [{regime}] n={n}"
    rng = np.random.default_rng(seed)
    if regime == "exact":       # P = 128 values of at most 2.01, multiples of 2**-13: the sum is exact, and so is its quotient by the power of two P
        x = hl_form(rng, (n, P, C), p_zero=0.25)
        assert P & (P - 1) == 0 and np.abs(x).sum(axis=1).max() < LIMIT
    else:
        x = np.where(rng.random((n, P, C)) < 0.25, 0.0, np.abs(rng.standard_normal((n, P, C)))).astype(np.float32).astype(np.float64)

    def launch(inp):
        a = inp["x"]
        h, l = split(a)
        h, l = _with_tail(_bits(h, np.float16), GUARD), _with_tail(_bits(l, np.float16), GUARD)
        valid = a.shape[0] * C
        oh, ol = _poisoned(valid), _poisoned(valid)
        st = lib.lib.kat_hp_gap(_ptr(h), _ptr(l), _ptr(oh), _ptr(ol), oh.size, a.shape[0], P, C)
        assert st == 0, f"{what}: launch status {st}"
        return {"out_h": (oh, valid, C), "out_l": (ol, valid, C)}

    o = _protocol(what, launch, dict(x=x), n, lambda inp, i: dict(x=inp["x"][i:i + 1]))
    gh, gl = _pair(what, o, "out", (n, C), paired=False)
    want = join(*split(x)).sum(axis=1) / P
    if regime == "exact":
        _exact_pair(what, gh, gl, want)
        return 0.0
    return _banded(what, lib.backend, "gap", gh + gl, want, (1,))


# ---------------------------------------------------------------------------------------------------------------------------------
# k_chain_hp<C, W, WR, HALO>: the four LightConv chains a0 | b0 b1 | c0 c1 c2 | d0 d1 d2 d3 of (hi, lo) x1 [n][H W][C] -> (hi, lo) y
# [4][n][H W][C] (paired order) and gap_part fp32 [4][n][bands][C] (logical order)
# ---------------------------------------------------------------------------------------------------------------------------------
CHAIN_INST = ((32, 32, 24, 4), (64, 32, 24, 4), (32, 16, 32, 0), (64, 16, 32, 0), (96, 16, 32, 0), (32, 8, 16, 0), (64, 8, 16, 0), (96, 8, 16, 0),
              (128, 8, 16, 0))


def chain_heights(inst):
    return (16, 48, 64) if inst[3] else (inst[2],)


REC_NAMES = ("a0", "b0", "b1", "c0", "c1", "c2", "d0", "d1", "d2", "d3")
BRANCH_RECS = ((0,), (1, 2), (3, 4, 5), (6, 7, 8, 9))
LO_RECS = (0, 2, 3, 5, 7, 9)                       # `exact`: the records whose 1x1 weights have lo != 0
SHORT_BIAS = {1: 1.25, 4: 2.75, 6: 1.25, 8: 1.75}  # `exact`: bias of the other records in units of the channel's largest depthwise sum


def chain_geo(lib: WideHpKatLib, inst):
    """ChainGeo's (tiles per wave NT, band rows R, LDS bytes) of an instantiation"""
    out = np.zeros(3, np.int32)
    assert lib.lib.kat_hp_chain_geo(*inst, _ptr(out)) == 0, f"k_chain_hp{inst}: not in the instantiation table"
    return int(out[0]), int(out[1]), int(out[2])


def _pw_exact(what: str, cur, W):
    """the 1x1 as the kernel computes it exactly: the definition's split of the fp32 tensor `cur`, three terms; asserts that every sum is
    exact in fp32 in any order from the operands alone"""
    assert np.array_equal(cur.astype(np.float32).astype(np.float64), cur), f"{what}: the layer's input is no fp32 tensor"
    xh, xl = (a.astype(np.float64) for a in split(cur))
    wh, wl = (a.astype(np.float64) for a in split(W))
    T = xh @ wh.T + xl @ wh.T + xh @ wl.T
    S = np.abs(xh) @ np.abs(wh).T + np.abs(xl) @ np.abs(wh).T + np.abs(xh) @ np.abs(wl).T
    lxh, lxl, lwh, lwl = _lowbit(xh), _lowbit(xl), _lowbit(wh), _lowbit(wl)
    q = np.full(T.shape, np.inf)
    for ci in range(W.shape[1]):
        co = np.nonzero(W[:, ci])[0]
        if co.size:
            t = np.minimum(np.minimum(lxh[..., ci, None] * lwh[co, ci], lxl[..., ci, None] * lwh[co, ci]), lxh[..., ci, None] * lwl[co, ci])
            q[..., co] = np.minimum(q[..., co], t)
    _order_free(what + " 1x1", S, q)
    return T


def _dw(T, dw, b, what=None, window=False):
    """depthwise 3x3 (zero padding) + bias + ReLU on [n][rows][W][C]; `what`: assert that the fp32 sum is exact in any order"""
    n, H, Wi, C = T.shape
    Tp = np.pad(T, ((0, 0), (1, 1), (1, 1), (0, 0)))
    acc = np.zeros_like(T) + b
    if what:
        S, q, lT = np.zeros_like(T) + np.abs(b), np.zeros_like(T) + _lowbit(b), _lowbit(Tp)
    for dy in range(3):
        for dx in range(3):
            acc += Tp[:, dy:dy + H, dx:dx + Wi] * dw[:, 3 * dy + dx]
            if what:
                S += np.abs(Tp[:, dy:dy + H, dx:dx + Wi] * dw[:, 3 * dy + dx])
                q = np.minimum(q, lT[:, dy:dy + H, dx:dx + Wi] * _lowbit(dw[:, 3 * dy + dx]))
    if what:
        _order_free(what + " depthwise", S, q)
    return np.maximum(acc, 0.0) + 0.0


def chain_inputs(inst, H: int, regime: str, n: int, seed: int, geo=None):
    """x [n][H][W][C] and ten records {pw [C][C], dw [C][9], b [C]}, all float64 values that fp32 holds.  geo = (NT, R, .): the impulses'
    wave seams"""
    C, Wi, WR, HALO = inst
    rng = np.random.default_rng(seed)
    recs = []
    if regime == "exact":
        x = hl_form(rng, (n, H, Wi, C), p_zero=0.25)
        for li in range(10):
            lo = li in LO_RECS
            neg = li in (0, 2, 5, 9)        # negative weights and taps only in a chain's last layer: a cancelled sum upstream of a lo != 0 layer has no integer hi
            pw = np.zeros((C, C))
            for co in range(C):
                ci = rng.choice(C, 2, replace=False)
                pw[co, ci[0]] = hl_form(rng, (), mags=(1.0,)) if lo else 1.0
                if rng.random() < (0.5 if li in (0, 2) else 0.2):       # the deep chains grow by every second weight: d3 has to stay below 2**11
                    pw[co, ci[1]] = (hl_form(rng, (), mags=(1.0,)) * (-1.0 if neg and rng.random() < 0.4 else 1.0)) if lo else 1.0
            dw = np.zeros((C, 9))
            dw[:, 4] = 1.0
            other = rng.choice([0, 1, 2, 3, 5, 6, 7, 8], C)
            dw[np.arange(C), other] = np.where(rng.random(C) < (0.3 if neg else 0.0), -1.0, 1.0)
            recs.append(dict(pw=pw, dw=dw, b=rng.integers(1, 4, C).astype(np.float64)))
        # the short records' biases come from the data: a multiple of the channel's largest depthwise sum, so that the NEXT layer's hi is an
        # integer (module docstring).  x1 = hi + lo exactly, and every layer below is exact, so float64 is the kernel's arithmetic here
        xx = join(*split(x))
        for br in range(4):
            cur = xx
            for li in BRANCH_RECS[br]:
                r = recs[li]
                T = _pw_exact("", cur, r["pw"])
                if li in SHORT_BIAS:
                    r["b"] = np.ceil(SHORT_BIAS[li] * _dw(T, r["dw"], 0.0).max(axis=(0, 1, 2))) + rng.integers(1, 4, C)
                cur = _dw(T, r["dw"], r["b"])
    else:
        # a calibrated block: activations of order 1 (a quarter zero), 1x1 of order 1 / sqrt(C), folded-BN depthwise taps, positive biases
        for li in range(10):
            recs.append(dict(pw=(rng.standard_normal((C, C)) * (1.3 / np.sqrt(C))).astype(np.float32).astype(np.float64),
                             dw=(rng.standard_normal((C, 9)) / 2.5).astype(np.float32).astype(np.float64),
                             b=(0.05 + 0.3 * np.abs(rng.standard_normal(C))).astype(np.float32).astype(np.float64)))
        if regime == "dense":
            x = np.where(rng.random((n, H, Wi, C)) < 0.25, 0.0, np.abs(rng.standard_normal((n, H, Wi, C)))).astype(np.float32).astype(np.float64)
        else:
            x = np.zeros((n, H, Wi, C))
            last = [16 * t + 15 for t in range(C // 16)]
            order = last + [c for c in range(C) if c not in last]
            for j, (y, xx) in enumerate(chain_impulse_pixels(inst, H, geo)):
                x[j % n, y, xx, order[j % C]] = np.float32(4.0 + 0.37 * (j % 7))
    assert all((r["b"] > 0).all() for r in recs)
    return dict(n=n, H=H, inst=inst, x=x, recs=recs, regime=regime)


def chain_impulse_pixels(inst, H: int, geo):
    """(y, x) of the impulses: the corners; both sides of every wave seam of every band (a wave owns NT tiles of 16 window pixels in row-major
    order); x = 15 / 16 at W = 32; the first and last window row of every band and the rows on both sides of every band seam"""
    C, Wi, WR, HALO = inst
    NT, R, _ = geo
    pix = {(0, 0), (0, Wi - 1), (H - 1, 0), (H - 1, Wi - 1)}
    for band in range(H // R):
        y0 = band * R - HALO
        for w in range(1, 8):
            for q in (w * NT * 16 - 1, w * NT * 16):
                pix.add((y0 + q // Wi, q % Wi))
        for y in (y0, y0 + WR - 1, band * R - 1, band * R, band * R + R - 1, band * R + R):
            pix |= {(y, 1), (y, Wi - 2)}
        if Wi == 32:
            pix |= {(band * R + 1, 15), (band * R + 1, 16), (band * R + R - 2, 15), (band * R + R - 2, 16)}
    return sorted(p for p in pix if 0 <= p[0] < H)


def chain_crop(inp, i):
    return dict(inp, n=1, x=inp["x"][i:i + 1])


def chain_reference(inp, exact=False, swap_recs=None):
    """[4][n][H][W][C] float64.  exact: the kernel's three-term arithmetic on the definition's splits, every sum asserted exact; else float64
    arithmetic on x = hi + lo and the fp32 weights.  swap_recs = (i, j): the control that exchanges two layer records."""
    recs = list(inp["recs"])
    if swap_recs:
        i, j = swap_recs
        recs[i], recs[j] = recs[j], recs[i]
    x = join(*split(inp["x"]))
    outs = []
    for br in range(4):
        cur = x
        for li in BRANCH_RECS[br]:
            r = recs[li]
            what = f"k_chain_hp{inp['inst']} H={inp['H']} [exact] record {REC_NAMES[li]}"
            T = _pw_exact(what, cur, r["pw"]) if exact else cur @ r["pw"].T
            cur = _dw(T, r["dw"], r["b"], what if exact else None)
        outs.append(cur)
    return np.stack(outs)


def chain_windowed(inp, halo: int, rezero=True, gap_with_halo=False):
    """The band structure restated (dense arithmetic): per band a window of R + 2 halo rows, rows outside the image zero on input and (rezero)
    after every layer, nothing known beyond the window.  halo = 4 and rezero is chain_reference; the controls: halo = 3, rezero = False (padding
    rows left at relu(bias)), gap_with_halo (the band sums over the whole window).  Returns (y [4][n][H][W][C], gap [4][n][bands][C])."""
    C, Wi, WR, HALO = inp["inst"]
    H, n, R = inp["H"], inp["n"], WR - 2 * HALO
    halo = halo if HALO else 0
    x = join(*split(inp["x"]))
    xp = np.pad(x, ((0, 0), (halo, halo), (0, 0), (0, 0)))
    y = np.zeros((4, n, H, Wi, C))
    gap = np.zeros((4, n, H // R, C))
    for band in range(H // R):
        rows = np.arange(band * R - halo, band * R + R + halo)
        inside = ((rows >= 0) & (rows < H))[None, :, None, None]
        for br in range(4):
            cur = xp[:, band * R:band * R + R + 2 * halo]
            for li in BRANCH_RECS[br]:
                r = inp["recs"][li]
                cur = _dw(cur @ r["pw"].T, r["dw"], r["b"])
                if rezero:
                    cur = np.where(inside, cur, 0.0)
            y[br, :, band * R:band * R + R] = cur[:, halo:halo + R]
            gap[br, :, band] = (cur if gap_with_halo else cur[:, halo:halo + R]).sum(axis=(1, 2))
    return y, gap


def chain_launch(lib: WideHpKatLib, inp):
    inst, n, H = inp["inst"], inp["n"], inp["H"]
    C, Wi, WR, HALO = inst
    R = WR - 2 * HALO
    xh, xl = split(to_paired(inp["x"]))
    xh, xl = _with_tail(_bits(xh, np.float16), GUARD), _with_tail(_bits(xl, np.float16), GUARD)
    recs = np.concatenate([np.concatenate([r["pw"].ravel(), r["dw"].ravel(), r["b"].ravel()]) for r in inp["recs"]]).astype(np.float32)
    valid, gvalid = 4 * n * H * Wi * C, 4 * n * (H // R) * C
    yh, yl, gap = _poisoned(valid), _poisoned(valid), _poisoned(gvalid, True)
    st = lib.lib.kat_hp_chain(C, Wi, WR, HALO, _ptr(xh), _ptr(xl), xh.size, n, H, _ptr(recs), _ptr(yh), _ptr(yl), yh.size, _ptr(gap), gap.size)
    assert st == 0, f"k_chain_hp{inst} H={H}: launch status {st}"
    # [4][n][..]: crop 1 alone is compared branch by branch in run_chain, not through _protocol's leading-axis slice
    return {"y_h": (yh, valid, 0), "y_l": (yl, valid, 0), "gap": (gap, gvalid, 0)}


def run_chain(lib: WideHpKatLib, inst, H: int, regime: str, n: int, seed: int = 0):
    C, Wi, WR, HALO = inst
    what = f"k_chain_hp{inst} H={H} [{regime}] n={n}"
    geo = chain_geo(lib, inst)
    R, nb = geo[1], H // geo[1]
    assert R == WR - 2 * HALO
    inp = chain_inputs(inst, H, regime, n, seed, geo)
    raw = []

    def launch(i):
        raw.append(chain_launch(lib, i))
        return raw[-1]
    o = _protocol(what, launch, inp, n, chain_crop)
    if n == 3:      # crop 1 alone (the third launch) against crop 1 of the batch, bit for bit: both planes and gap_part, every branch
        for k, per in (("y_h", H * Wi * C), ("y_l", H * Wi * C), ("gap", nb * C)):
            batch, one = raw[0][k][0][:4 * n * per].reshape(4, n, per), raw[2][k][0][:4 * per].reshape(4, per)
            assert np.array_equal(batch[:, 1], one), f"{what}: {k} of crop 1 alone differs from crop 1 of the batch of 3 (crops are not independent)"
    gh, gl = _pair(what, o, "y", (4, n, H, Wi, C))
    got = gh + gl
    gap = o["gap"].reshape(4, n, nb, C)
    # gap_part against float64 sums of the kernel's OWN outputs: the kernel adds R W fp32 values (each within 2**-22 of its stored pair) in
    # some order: (R W + 4) U24 sum |o|; where the sum of the outputs is exact in fp32 in any order (`exact`, small sums) it is bit for bit
    own = got.reshape(4, n, nb, R * Wi, C)
    gsum, gabs = own.sum(axis=3), np.abs(own).sum(axis=3)
    gbnd = (R * Wi + 4) * U24 * gabs + 2.0 ** -149
    if regime == "exact":
        want = chain_reference(inp, exact=True)
        _zero_fraction(what, want)
        _exact_pair(what, gh, gl, want)
        sure = gabs <= 2.0 ** 24 * _lowbit(own).min(axis=3)
        print(f"{what}: gap_part compared bit for bit in {int(sure.sum())} of {sure.size} sums")
        _exact(what + " gap_part (exact sums)", gap[sure], gsum[sure], f32=True)
        gap, gsum, gbnd = gap[~sure], gsum[~sure], gbnd[~sure]
    _within(what + " gap_part", gap, gsum, gbnd)
    if regime == "exact":
        return 0.0
    ref = chain_reference(inp)
    if regime == "impulses":
        assert (inp["x"] != 0).sum() >= 8
    return _banded(what, lib.backend, "chain", got, ref, (2, 3, 4))


# ---------------------------------------------------------------------------------------------------------------------------------
# outside a kernel's contract: -1, nothing launched (no buffer is touched: the dummies are a few elements long)
# ---------------------------------------------------------------------------------------------------------------------------------
def run_rejects(lib: WideHpKatLib):
    h = np.zeros(64, np.uint16)
    f = np.zeros(64, np.float32)
    p = _ptr(h)

    def gemm(epi, bn, db, M, N, K, bias=True, out_l=True, res=False, K2=0):
        big = 1 << 40           # the lengths claim enough: only the shape is wrong
        return lib.lib.kat_hp_gemm(epi, bn, db, p, p, big, p, p, _ptr(f) if bias else None, p, p if out_l else None, big, p if res else None,
                                   p if res else None, big if res else 0, M, N, K, 1, p if K2 else None, p if K2 else None, big if K2 else 0,
                                   p if K2 else None, p if K2 else None, K2)
    bad = {
        "EPI 2, M = 130": gemm(2, 128, 2, 130, 128, 32), "EPI 3, M = 192": gemm(3, 128, 2, 192, 128, 32), "EPI 2 without a bias": gemm(2, 128, 2, 128, 128, 32, bias=False),
        "BN = 48": gemm(0, 48, 2, 128, 96, 32), "N = 96 at BN = 64": gemm(0, 64, 2, 128, 96, 32), "K = 48": gemm(0, 32, 2, 128, 32, 48),
        "K2 = 16": gemm(0, 32, 2, 128, 32, 32, K2=16), "EPI 1 at BN = 64": gemm(1, 64, 2, 128, 64, 32, res=True), "EPI 1 at DB = 1": gemm(1, 128, 1, 128, 128, 32, res=True),
        "EPI 1 without a residual": gemm(1, 128, 2, 128, 128, 32), "EPI 4 with a lo plane": gemm(4, 128, 2, 3, 128, 32), "a second pair under EPI 1": gemm(1, 128, 2, 128, 128, 32, res=True, K2=32),
        "M = 0": gemm(0, 32, 2, 0, 32, 32),
    }
    geo = np.zeros(3, np.int32)
    for inst, H in (((96, 32, 24, 4), 64), ((128, 16, 32, 0), 32), ((32, 8, 16, 4), 16), ((32, 32, 16, 0), 16), ((48, 8, 16, 0), 16), ((32, 32, 24, 4), 24),
                    ((32, 16, 32, 0), 64), ((32, 8, 16, 0), 8)):
        bad[f"k_chain_hp{inst} H={H}"] = lib.lib.kat_hp_chain(*inst, p, p, 1 << 40, 1, H, _ptr(f), p, p, 1 << 40, _ptr(f), 1 << 40)
    for inst in ((96, 32, 24, 4), (128, 16, 32, 0), (32, 8, 16, 4)):
        bad[f"ChainGeo{inst}"] = lib.lib.kat_hp_chain_geo(*inst, _ptr(geo))
    bad["stem width 48"] = lib.lib.kat_hp_stem(48, p, p, 1 << 40, 1, _ptr(f), _ptr(f), p, p, 1 << 40)
    bad["gate width 48"] = lib.lib.kat_hp_gate(48, p, p, _ptr(f), _ptr(f), _ptr(f), _ptr(f), _ptr(f), p, p, 1 << 40, 128, 1, 1)
    wrong = {k: v for k, v in bad.items() if v != -1}
    assert not wrong, f"accepted (or failed otherwise) outside the contract: {wrong}"
    return len(bad)


# ---------------------------------------------------------------------------------------------------------------------------------
# controls: wrong references the comparisons must reject (CPU only, no kernel)
# ---------------------------------------------------------------------------------------------------------------------------------
def _band_any(unit: str) -> float:
    return max(band(b, unit) for b in MEASURED)


def _leaves(what: str, right, wrong, unit: str, crop_axes=None) -> int:
    scale = np.abs(right).max(axis=crop_axes, keepdims=True) if crop_axes else np.abs(right).max()
    return _rejects(what, right, wrong.reshape(right.shape), np.broadcast_to(_band_any(unit) * scale, right.shape))


def _differs(what: str, right, wrong) -> int:
    """exact regimes: expected fp32 values that differ (their planes then differ, too)"""
    out = int((wrong.astype(np.float32) != right.astype(np.float32).reshape(wrong.shape)).sum())
    print(f"CONTROL {what}: {out} of {right.size} expected values differ")
    return out


def controls():
    """{name: elements of the wrong reference outside the band (dense) or different from the exact expectation (exact)}: every value must be > 0
    except those under "same function", which the caller reports"""
    res, same = {}, {}
    for regime in ("exact", "dense"):
        d = gemm_inputs(regime, 0, 129, 128, 64, seed=3, K2=96)
        name = f"k_gemm_hp<0> M=129 N=128 K=64 K2=96 [{regime}]"
        if regime == "exact":
            right = gemm_check_case(name, d)
            judge = lambda w, what: _differs(f"{name}: {what}", right, w)
            res["gemm four terms"] = judge(gemm_reference(d, terms=4), "the four-term product")
        else:
            right = gemm_reference(d, terms=4)
            judge = lambda w, what: _leaves(f"{name}: {what}", right, w, "gemm")
            fp16 = gemm_reference(d, terms=4, w_fp16=True)
            dist = float(np.abs(fp16 - right).max() / (_band_any("gemm") * np.abs(right).max()))
            print(f"CONTROL {name}: weights rounded to fp16 miss by {dist:.1f} bands")
            assert dist >= FP16_OPERANDS_MIN_BANDS, f"{name}: the fp16-weight reference misses by only {dist:.1f} bands"
            res["gemm fp16 weights"] = judge(fp16, "weights rounded to fp16")
        t = 3 if regime == "exact" else 4
        res[f"gemm two terms [{regime}]"] = judge(gemm_reference(d, terms=2), "Wl.xh missing")
        res[f"gemm k logical [{regime}]"] = judge(gemm_reference(d, terms=t, k_logical=True), "k columns in logical order")
        res[f"gemm bias without downsample [{regime}]"] = judge(gemm_reference(d, terms=t, bias_wo_down=True), "conv3's bias without the downsample's")
        for epi in (2, 3):
            d = gemm_pool_inputs(regime, epi, 1, 8, seed=4)
            name = f"k_gemm_hp<{epi}> pool={d['pool']} [{regime}]"
            if regime == "exact":
                right = gemm_check_case(name, d)
                judge = lambda w, what: _differs(f"{name}: {what}", right, w)
            else:
                right = gemm_reference(d, terms=4)
                judge = lambda w, what: _leaves(f"{name}: {what}", right, w, "gemm.pool")
            res[f"gemm<{epi}> pool rows (1, 2) [{regime}]"] = judge(gemm_reference(d, terms=t, pool_rows12=True), "the pool pairing rows (1, 2)")
            res[f"gemm<{epi}> ReLU after the pool [{regime}]"] = judge(gemm_reference(d, terms=t, relu_after_pool=True), "ReLU after the pool")
    # chain
    inst, H = (32, 32, 24, 4), 48
    for regime in ("dense", "impulses"):
        inp = chain_inputs(inst, H, regime, 1, seed=5, geo=(3, 16, 0))
        name = f"k_chain_hp{inst} H={H} [{regime}]"
        right = chain_reference(inp)
        y4, g4 = chain_windowed(inp, 4)
        assert np.abs(y4 - right).max() <= 1e-12 * np.abs(right).max(), "chain_windowed(halo = 4) is not chain_reference"
        judge = lambda w, what: _leaves(f"{name}: {what}", right, w, "chain", (2, 3, 4))
        res[f"chain padding rows at relu(bias) [{regime}]"] = judge(chain_windowed(inp, 4, rezero=False)[0], "padding rows left at relu(bias)")
        res[f"chain records exchanged [{regime}]"] = judge(chain_reference(inp, swap_recs=(7, 8)), "records d1 and d2 exchanged")
        res[f"chain 3-row halo [{regime}]"] = judge(chain_windowed(inp, 3)[0], "a 3-row halo")
        R = 16
        own = right.reshape(4, 1, H // R, R * 32, 32)
        gb = (R * 32 + 4) * U24 * np.abs(own).sum(axis=3) + 2.0 ** -149
        res[f"chain gap_part with halo rows [{regime}]"] = _rejects(f"{name}: gap_part including halo rows", g4, chain_windowed(inp, 4, gap_with_halo=True)[1], gb)
    inp = chain_inputs(inst, H, "exact", 1, seed=8)
    right = chain_reference(inp, exact=True)
    res["chain records exchanged [exact]"] = _differs(f"k_chain_hp{inst} H={H} [exact]: records a0 and b1 exchanged", right, chain_reference(inp, swap_recs=(0, 2)))
    # gate
    for regime in ("exact", "dense"):
        inp = gate_inputs(32, 136, 2, regime, 1, seed=7)
        name = f"k_gate_sum4_hp<32> P=136 nbands=2 [{regime}]"
        if regime == "exact":
            right = gate_reference(inp)[0]
            judge = lambda w, what: _differs(f"{name}: {what}", right, w)
        else:
            right, allow, _ = gate_reference(inp, wk.gate_allowance("gpu"))
            judge = lambda w, what: _rejects(f"{name}: {what}", right, w, _band_any("gate") * np.abs(right).max(axis=(1, 2), keepdims=True) + allow)
        res[f"gate gates exchanged [{regime}]"] = judge(gate_reference(inp, swap_gates=True)[0], "gates of branches 1 and 2 exchanged")
        res[f"gate logical position [{regime}]"] = judge(gate_reference(inp, logical_gate=True)[0], "gate read at the logical position")
        res[f"gate mean over nbands P [{regime}]"] = judge(gate_reference(dict(inp, P=136 * 2))[0], "mean divided by nbands P")
    # stem
    inp = stem_inputs(32, "dense", 1, 6)
    name = "k_wide_stem_hp<32> [dense] n=1"
    right = stem_reference(inp, terms=4)
    res["stem tile-left neighbour dropped"] = _leaves(f"{name}: left neighbour at conv columns 16, 32, 48 dropped", right, stem_reference(inp, terms=4, drop_tile_left=True), "stem", (1, 2))
    res["stem lo plane ignored"] = _leaves(f"{name}: the crops' lo plane ignored", right, stem_reference(inp, terms=4, ignore_lo=True), "stem", (1, 2))
    res["same function"] = same
    return res
