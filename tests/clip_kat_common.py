"""Known-answer cases for the CLIP-ReID kernels around the GEMMs (boxmot_amd/csrc/clip_kernels.hpp: k_clip_patches, k_clip_tokens_lnpre,
k_clip_layernorm_f16, k_clip_attention, k_clip_attention_t<T>, k_clip_head) run through tests/kat/clip_kat.hip: shared by the device test
(test_gpu_clip_kat.py) and its CPU-thread emulation (test_clip_kat_emu.py).  Not a product path.

Every reference is float64 numpy on the kernel's own (already rounded) inputs.  Every bound is a per-element worst case derived from the
reference's quantities and the number formats alone (u = 2**-24, the fp32 unit roundoff; half an fp16 ulp for an fp16 store), written next to the
code that evaluates it; the one measured number is the relative error of the attention's exponential (EXPF_*, below).

Around every launch, as in gemm_kat_common.py: the output allocation is prefilled with the NaN poison patterns and followed by guard rows;
every element the kernel owns must come back finite, every other one must still be poison (guard rows, and for the head the rows not
named in out_rows); activation inputs are followed by poison rows (a read past the last valid row turns outputs into NaN); each launch
runs twice and must return identical bits.

A bound that anything passes proves nothing, so every bounded regime also evaluates deliberately WRONG references against the kernel's
output (``*_wrong_references``): each must leave the bound of the true reference for at least one element of every case it is applied to.
"""
from __future__ import annotations

import ctypes
import subprocess
from pathlib import Path

import numpy as np

from gemm_kat_common import F16_POISON, F32_POISON, U24

KAT_SRC = Path(__file__).resolve().parent / "kat" / "clip_kat.hip"
GUARD = 8                       # guard rows after every output
LN_EPS = 1e-5

# The attention's exponential, BM_EXPF: __expf on the device (v_exp_f32 of x * log2(e): the product is rounded to fp32, so the relative
# error grows with |x|), expf in the emulation.  Its relative error is not derivable from the source: measure_expf() measures it against
# float64 over the arguments the cases produce (every x in [-17.4, 0]: a probability below 2**-25 is an fp16 zero and is bounded
# absolutely instead), the tests print it, and the bound uses max(4 * measured, EXPF_FLOOR).
#   measured on an MI355X (tests/test_gpu_clip_kat.py::test_device_expf): 9.343e-07, so the device bound uses 4 x = 3.737e-06 (the floor
#   is 2**-21 = 4.768e-07); in the emulation (glibc expf): 5.95e-08, where the floor applies.  Either is small beside the half fp16 ulp
#   (up to 4.9e-04 relative) every probability carries.
#   Largest max err / bound on the device, per kernel: k_clip_layernorm_f16 0.9995 (the fp16 store dominates: the bound is half an fp16
#   ulp plus ~1e-4), k_clip_tokens_lnpre 0.068, k_clip_attention 0.994 (uniform) / 0.737 (normal) / 0.609 (peaked),
#   k_clip_attention_t<129> 0.992 / 0.656 / 0.582, k_clip_head 0.008 (its bound is the any-order worst case of three fp32 reductions).
EXPF_FLOOR = 2.0 ** -21
EXPF_MEASURED_DEVICE = 9.343e-07
EXPF_ARG_MIN = -17.4


def build_gpu(out_dir: Path, timeout: float = 600) -> Path:
    """hipcc for gfx950 with the product's flags (__graft_entry__.HIPCC_FLAGS) -> out_dir/libclip_kat.so"""
    from __graft_entry__ import HIPCC_FLAGS

    out = Path(out_dir) / "libclip_kat.so"
    subprocess.run(["hipcc", *HIPCC_FLAGS, "-o", str(out), str(KAT_SRC)], check=True, timeout=timeout)
    return out


def build_emu(clang: str, out_dir: Path, timeout: float = 600) -> Path:
    """the same source on CPU threads (tests/host_emu/hip_shim.hpp), built as gemm_kat_common.build_emu builds its harness"""
    out = Path(out_dir) / "libclip_kat_emu.so"
    subprocess.run([clang, "-x", "c++", "-std=c++17", "-O1", "-fPIC", "-shared", "-pthread", "-ffp-contract=off", "-DKAT_EMU",
                    "-DEMU_DEFER_GLDS=1", "-o", str(out), str(KAT_SRC)], check=True, timeout=timeout)
    return out


class ClipKatLib:
    """ctypes face of clip_kat.hip's entry points"""

    def __init__(self, path):
        self.lib = L = ctypes.CDLL(str(path))
        P, I, G = ctypes.c_void_p, ctypes.c_int, ctypes.c_long
        L.kat_clip_patches.argtypes = [P, G, P, G, I, I, I, I, I, I]
        L.kat_clip_tokens_lnpre.argtypes = [P, G, P, P, P, P, P, G, G, I, I]
        L.kat_clip_layernorm.argtypes = [P, G, P, P, P, G, G, I]
        L.kat_clip_attention.argtypes = [P, G, P, G, I, I, I, I]
        L.kat_clip_attention_t.argtypes = [I, P, G, P, G, I, I, I]
        L.kat_clip_head.argtypes = [P, G, P, P, P, P, P, P, P, P, G, P, I, I, I, I]
        L.kat_expf.argtypes = [P, P, G]
        for f in (L.kat_clip_patches, L.kat_clip_tokens_lnpre, L.kat_clip_layernorm, L.kat_clip_attention, L.kat_clip_attention_t,
                  L.kat_clip_head, L.kat_expf):
            f.restype = ctypes.c_int


# ---------------------------------------------------------------------------------------------------------------------------------
# plumbing: poison, guard rows, two launches
# ---------------------------------------------------------------------------------------------------------------------------------
def _poison(shape, f32: bool) -> np.ndarray:
    return np.full(shape, F32_POISON, np.uint32) if f32 else np.full(shape, F16_POISON, np.uint16)


def _rows_then_poison(a: np.ndarray, extra: int) -> np.ndarray:
    """the rows of `a` (fp32 or fp16) followed by `extra` poison rows, as raw bits"""
    f32 = a.dtype == np.float32
    out = _poison((a.shape[0] + extra, a.shape[1]), f32)
    out[:a.shape[0]] = np.ascontiguousarray(a).view(np.uint32 if f32 else np.uint16)
    return out


def _twice(label: str, launch):
    """launch() -> (status, raw output bits), run twice: both 0 and bit-identical"""
    st, C = launch()
    assert st == 0, f"{label}: launch status {st}"
    st2, C2 = launch()
    assert st2 == 0, f"{label}: second launch status {st2}"
    assert np.array_equal(C, C2), f"{label}: two launches on the same inputs differ"
    return C


def _owned(label: str, C: np.ndarray, owned_rows: np.ndarray) -> np.ndarray:
    """C: raw bits [rows][cols].  Rows in the boolean mask `owned_rows` must be finite everywhere (so: overwritten), all others still
    poison.  Returns the owned rows as float64."""
    f32 = C.dtype == np.uint32
    poison = F32_POISON if f32 else F16_POISON
    rest = C[~owned_rows]
    assert np.all(rest == poison), (f"{label}: a row the kernel does not own was written: row "
                                    f"{int(np.flatnonzero(~owned_rows)[np.argwhere(rest != poison)[0][0]])}")
    got = C[owned_rows].view(np.float32 if f32 else np.float16).astype(np.float64)
    bad = ~np.isfinite(got)
    assert not bad.any(), f"{label}: {int(bad.sum())} outputs not finite (unwritten, or poison rows read), first at {tuple(np.argwhere(bad)[0])}"
    return got


def _first_rows(total: int, n: int) -> np.ndarray:
    m = np.zeros(total, bool)
    m[:n] = True
    return m


def _inside(label: str, got, want, bnd):
    err = np.abs(got - want)
    over = err > bnd
    if over.any():
        i = tuple(np.argwhere(over)[0])
        raise AssertionError(f"{label}: {int(over.sum())} of {over.size} outputs outside the bound, first at {i}: got {got[i]!r} want "
                             f"{want[i]!r}, err {err[i]:.3e} > {bnd[i]:.3e}")
    return float(err.max()), float((err / bnd).max())


def _caught(label: str, got, bnd, wrong: dict):
    """every deliberately wrong reference must leave the bound somewhere"""
    for name, w in wrong.items():
        assert (np.abs(got - w) > bnd).any(), f"{label}: the wrong reference '{name}' stays inside the bound everywhere: the bound does not bite"
    return sorted(wrong)


# ---------------------------------------------------------------------------------------------------------------------------------
# k_clip_patches: bit-exact
# ---------------------------------------------------------------------------------------------------------------------------------
def run_patches(lib: ClipKatLib, n: int, H: int, W: int, patch: int, gh: int, gw: int, seed: int = 0) -> int:
    """fp16(crop[...]) gathered in (ky, kx, c) order, bit for bit; returns the number of elements compared"""
    label = f"k_clip_patches n={n} {H}x{W} patch {patch} grid {gh}x{gw}"
    rng = np.random.default_rng(seed)
    crops = rng.random((n, H, W, 3), dtype=np.float32) * np.float32(2) - np.float32(1)
    flat = _rows_then_poison(crops.reshape(n * H, W * 3), patch)             # one more patch row of poison pixels
    rows, K = n * gh * gw, patch * patch * 3
    C0 = _poison((rows + GUARD, K), False)

    def launch():
        C = C0.copy()
        return lib.lib.kat_clip_patches(flat.ctypes.data, flat.size, C.ctypes.data, C.nbytes, n, H, W, patch, gh, gw), C

    C = _twice(label, launch)
    _owned(label, C, _first_rows(rows + GUARD, rows))
    want = crops[:, :gh * patch, :gw * patch].reshape(n, gh, patch, gw, patch, 3).transpose(0, 1, 3, 2, 4, 5).reshape(rows, K).astype(np.float16)
    wrong = C[:rows] != want.view(np.uint16)
    assert not wrong.any(), f"{label}: {int(wrong.sum())} of {wrong.size} halves differ from fp16(crop), first at {tuple(np.argwhere(wrong)[0])}"
    return int(wrong.size)


# ---------------------------------------------------------------------------------------------------------------------------------
# LayerNorm: the float64 reference, its bound, and the fp32 replay of k_clip_layernorm_f16's arithmetic
# ---------------------------------------------------------------------------------------------------------------------------------
def ln_reference(v, gamma, beta, ddof: int = 0, eps: float = LN_EPS):
    v = v.astype(np.float64)
    d = v - v.mean(-1, keepdims=True)
    var = (d * d).sum(-1, keepdims=True) / (v.shape[-1] - ddof)
    return d / np.sqrt(var + eps) * gamma.astype(np.float64) + beta.astype(np.float64)


def ln_bound(v, gamma, beta):
    """(float64 LayerNorm of the fp32 rows v, worst-case |error| of an fp32 evaluation), u = 2**-24:
      mean      a sum of D terms in ANY order is within (D - 1) u sum|x| of the exact one, the division by D adds u:
                |mean^ - mean| <= dm = D u mean|x|
      centring  d^ = fl(x - mean^): |d^ - d| <= dd = dm + u (|d| + dm)
      variance  |d^**2 - d**2| <= e2 = dd (2 |d| + dd); the squares round (u each), the second any-order sum of D terms and the division:
                |var^ - var| <= dv = (D + 2) u (var + mean(e2)) + mean(e2)
      rstd      r = (var + eps) ** -0.5: |r^ - r| / r <= rr = dv / (2 (var + eps - dv)) + 3 u   (the add, the square root, the reciprocal)
      affine    y^ = fl(fl(fl(d^ r^) g) + b): |d^ r^ - d r| <= dd r (1 + rr) + |d| r rr, two roundings on the product, one on the sum
    """
    v, g, b = v.astype(np.float64), np.abs(gamma.astype(np.float64)), beta.astype(np.float64)
    D = v.shape[-1]
    mean = v.mean(-1, keepdims=True)
    d = v - mean
    var = (d * d).mean(-1, keepdims=True)
    r = 1.0 / np.sqrt(var + LN_EPS)
    y = d * r * gamma.astype(np.float64) + b
    dm = D * U24 * np.abs(v).mean(-1, keepdims=True)
    dd = dm + U24 * (np.abs(d) + dm)
    e2 = (dd * (2 * np.abs(d) + dd)).mean(-1, keepdims=True)
    dv = (D + 2) * U24 * (var + e2) + e2
    assert (dv < 0.5 * (var + LN_EPS)).all(), "the inputs make the variance itself uncertain: no meaningful bound"
    rr = dv / (2 * (var + LN_EPS - dv)) + 3 * U24
    bnd = (dd * r * (1 + rr) + np.abs(d) * r * rr) * g * (1 + 2 * U24) + 2 * U24 * np.abs(d) * r * g
    bnd = bnd + U24 * (np.abs(y) + bnd)
    return y, bnd


def half_ulp16(x):
    """the largest error of rounding a value of magnitude <= x to fp16 (round to nearest even): half the spacing of fp16 at x, 2**-25 for
    the subnormals"""
    return 2.0 ** (np.floor(np.log2(np.maximum(x, 2.0 ** -14))) - 11)


def f16_store(y, bnd):
    """the bound after an fp16 store: the stored value is within bnd of y, so its rounding error is at most half_ulp16(|y| + bnd)"""
    return bnd + half_ulp16(np.abs(y) + bnd)


def _wave_sum(v):
    """clip_wave_sum: v += shfl_xor(v, 32), 16, 8, 4, 2, 1 on [rows][64] fp32: every lane ends with the same value"""
    idx = np.arange(64)
    for m in (32, 16, 8, 4, 2, 1):
        v = v + v[:, idx ^ m]
    return v[:, 0]


def ln_replay_f32(x: np.ndarray, gamma: np.ndarray, beta: np.ndarray) -> np.ndarray:
    """k_clip_layernorm_f16's GENERIC loop, operation by operation in fp32 (the library is built without FMA contraction; +, -, *, /
    and sqrt are correctly rounded on both sides): lane l of the row's wavefront owns the 4-column groups at c = 4 l + 256 i;
      s_l  = ((0 + g_0) + g_1) + ..   with g_i = ((x[c] + x[c + 1]) + x[c + 2]) + x[c + 3], groups beyond D skipped
      mean = wave_sum(s) / D          the xor butterfly 32, 16, 8, 4, 2, 1
      ss_l = (((0 + d0 d0) + d1 d1) + d2 d2) + d3 d3 + ..  over the same groups in the same order, d = x - mean
      rstd = 1 / sqrt(wave_sum(ss) / D + 1e-5f)
      out  = fp16((((x - mean) * rstd) * gamma) + beta)
    The D == 768 register path is documented as the same operations in the same order: its output must equal this replay bit for bit,
    and so must the generic loop's at every other D (which is what shows that the replay IS the generic loop).  Returns fp16 bits."""
    assert x.dtype == np.float32 and x.shape[1] % 4 == 0
    rows, D = x.shape
    ni = -(-D // 256)
    xp = np.zeros((rows, ni * 256), np.float32)
    xp[:, :D] = x
    g4 = xp.reshape(rows, ni, 64, 4)
    valid = (np.arange(ni * 256) < D).reshape(ni, 64, 4)[:, :, 0]
    s = np.zeros((rows, 64), np.float32)
    for i in range(ni):
        s = np.where(valid[i], s + (((g4[:, i, :, 0] + g4[:, i, :, 1]) + g4[:, i, :, 2]) + g4[:, i, :, 3]), s)
    mean = (_wave_sum(s) / np.float32(D))[:, None]
    ss = np.zeros((rows, 64), np.float32)
    for i in range(ni):
        for j in range(4):
            d = g4[:, i, :, j] - mean
            ss = np.where(valid[i], ss + d * d, ss)
    rstd = (np.float32(1) / np.sqrt(_wave_sum(ss) / np.float32(D) + np.float32(LN_EPS)))[:, None]
    y = ((x - mean) * rstd) * gamma[None, :] + beta[None, :]
    assert y.dtype == np.float32
    return y.astype(np.float16).view(np.uint16)


LN_KINDS = ("random", "bigmean", "small")


def ln_rows(kind: str, rows: int, D: int, rng) -> np.ndarray:
    """fp32 input rows: N(0, 1); mean 1e3 and unit spread; magnitude 1e-3; a constant small integer per row; alternating +-1"""
    if kind == "random":
        return rng.standard_normal((rows, D), np.float32)
    if kind == "bigmean":
        return (rng.standard_normal((rows, D), np.float32) + np.float32(1e3)).astype(np.float32)
    if kind == "small":
        return rng.standard_normal((rows, D), np.float32) * np.float32(1e-3)
    if kind == "const":
        return np.repeat(((np.arange(rows) % 7) - 3).astype(np.float32)[:, None], D, 1)
    if kind == "alt":
        return (np.where(np.arange(D) % 2 == 0, 1.0, -1.0)[None, :] * np.where(np.arange(rows) % 2 == 0, 1.0, -1.0)[:, None]).astype(np.float32)
    raise ValueError(kind)


def ln_gain_bias(D: int, rng):
    """as random_clipreid_state_dict(gain_randomised=True) draws them: gains U(0.4, 2.5), biases N(0, 0.3)"""
    return rng.uniform(0.4, 2.5, D).astype(np.float32), (rng.standard_normal(D) * 0.3).astype(np.float32)


def ln_wrong_references(kind: str, v, gamma, beta) -> dict:
    """the LayerNorm controls.  `D - 1` is applied to the N(0, 1) rows: on the mean-1e3 rows the bound itself (the cancellation in x - mean:
    D u 1e3 ~ 5e-2 per unit of spread) is wider than the 1 / (2 D) the divisor moves the result by, on the 1e-3 rows eps = 1e-5 dilutes a
    variance of 1e-6 tenfold, and on constant rows the variance is 0 under either divisor.  eps = 1e-6 is applied where eps matters (the
    1e-3 rows).  gamma <-> beta everywhere."""
    w = {"gamma and beta swapped": ln_reference(v, beta, gamma)}
    if kind == "random":
        w["variance over D - 1"] = ln_reference(v, gamma, beta, ddof=1)
    if kind == "small":
        w["eps 1e-6"] = ln_reference(v, gamma, beta, eps=1e-6)
    return w


def _ln_known_answers(label, kind, got, v, gamma, beta, f16: bool):
    if kind == "const":         # the sum of D equal small integers and its quotient by D are exact: d = 0 and the output is beta itself
        want = np.broadcast_to(beta.astype(np.float16).astype(np.float64) if f16 else beta.astype(np.float64), got.shape)
        assert np.array_equal(got, want), f"{label}: a constant row must return beta exactly, {int((got != want).sum())} elements differ"
    if kind == "alt":           # mean 0, variance 1: +-gamma / sqrt(1 + 1e-5) + beta (within the bound, checked by the caller against this too)
        return v.astype(np.float64) * gamma.astype(np.float64) / np.sqrt(1 + LN_EPS) + beta.astype(np.float64)
    return None


def run_layernorm(lib: ClipKatLib, D: int, rows: int, kind: str, seed: int = 0):
    """k_clip_layernorm_f16 on `rows` rows of `kind`.  Returns (max err, max err / bound, names of the controls caught)."""
    label = f"k_clip_layernorm_f16 D={D} rows={rows} [{kind}]"
    rng = np.random.default_rng(seed)
    x = ln_rows(kind, rows, D, rng)
    gamma, beta = ln_gain_bias(D, rng)
    X = _rows_then_poison(x, 4)
    C0 = _poison((rows + GUARD, D), False)

    def launch():
        C = C0.copy()
        return lib.lib.kat_clip_layernorm(X.ctypes.data, X.shape[0], gamma.ctypes.data, beta.ctypes.data, C.ctypes.data, C.nbytes, rows, D), C

    C = _twice(label, launch)
    got = _owned(label, C, _first_rows(rows + GUARD, rows))
    y, b32 = ln_bound(x, gamma, beta)
    bnd = f16_store(y, b32)
    stats = _inside(label, got, y, bnd)
    alt = _ln_known_answers(label, kind, got, x, gamma, beta, True)
    if alt is not None:
        _inside(label + " closed form", got, alt, bnd)
    # both code paths against the stated arithmetic order: the generic loop (D != 768) and the register path (D == 768), bit for bit
    replay = ln_replay_f32(x, gamma, beta)
    diff = C[:rows] != replay
    assert not diff.any(), (f"{label}: {int(diff.sum())} of {diff.size} halves differ from the fp32 replay of the generic loop "
                            f"({'register path' if D == 768 else 'generic loop'}), first at {tuple(np.argwhere(diff)[0])}")
    return (*stats, _caught(label, got, bnd, ln_wrong_references(kind, x, gamma, beta)))


def run_tokens_lnpre(lib: ClipKatLib, D: int, T: int, n: int, kind: str, seed: int = 0):
    """k_clip_tokens_lnpre: x[crop][0] = LN(cls + pos[0]), x[crop][1 + p] = LN(pe[crop][p] + pos[1 + p]).  The fp32 sum src + pos is one
    correctly rounded addition, evaluated three times by the kernel: the reference is the float64 LayerNorm of that fp32 sum."""
    label = f"k_clip_tokens_lnpre D={D} T={T} n={n} [{kind}]"
    rng = np.random.default_rng(seed)
    rows = n * T
    allv = ln_rows(kind, rows, D, rng).reshape(n, T, D)
    pos = (rng.standard_normal((T, D)) * (1e-4 if kind == "small" else 0.1)).astype(np.float32)
    if kind in ("const", "alt"):
        pos = np.full((T, D), 0 if kind == "alt" else 1, np.float32)      # keeps the sums exact integers
    pe = np.ascontiguousarray(allv[:, 1:].reshape(n * (T - 1), D))
    cls = np.ascontiguousarray(allv[0, 0])                 # one class embedding for every crop
    v = np.empty((n, T, D), np.float32)
    v[:, 0] = cls + pos[0]
    v[:, 1:] = allv[:, 1:] + pos[None, 1:]
    v = v.reshape(rows, D)
    gamma, beta = ln_gain_bias(D, rng)
    PE = _rows_then_poison(pe, 4)
    C0 = _poison((rows + GUARD, D), True)

    def launch():
        C = C0.copy()
        return lib.lib.kat_clip_tokens_lnpre(PE.ctypes.data, PE.shape[0], cls.ctypes.data, pos.ctypes.data, gamma.ctypes.data,
                                             beta.ctypes.data, C.ctypes.data, C.nbytes, rows, T, D), C

    C = _twice(label, launch)
    got = _owned(label, C, _first_rows(rows + GUARD, rows))
    y, bnd = ln_bound(v, gamma, beta)
    stats = _inside(label, got, y, bnd)
    alt = _ln_known_answers(label, kind, got, v, gamma, beta, False)
    if alt is not None:
        _inside(label + " closed form", got, alt, bnd)
    return (*stats, _caught(label, got, bnd, ln_wrong_references(kind, v, gamma, beta)))


# ---------------------------------------------------------------------------------------------------------------------------------
# attention
# ---------------------------------------------------------------------------------------------------------------------------------
ATTN_REGIMES = ("onehot", "uniform", "normal", "peaked")
ONEHOT_GAP = 24


def attn_inputs(regime: str, n: int, T: int, heads: int, seed: int = 0):
    """q | k | v rows fp16 [n T][3 D] (D = 64 heads), and for `onehot` the key pi[crop][head][i] query i matches.
      onehot   k_j = 2 code_j, q_i = 4 code_pi(i), code = random +-1 rows of length 64 per (crop, head): logit(i, j) = dot(code_pi(i), code_j),
               64 at the match and (checked here, re-drawn otherwise) at most 64 - 24 elsewhere.  pi is a permutation, so some query
               matches key 0 and some key T - 1.  v random.
      uniform  q = 0 (k random), v small integers: every probability 1
      normal   N(0, 1.5**2)
      peaked   q, k ~ N(0, 6): logit standard deviation 6, what the sharp-attention weights produce; v ~ N(0, 1)"""
    rng = np.random.default_rng(seed)
    D = 64 * heads
    x = np.zeros((n, T, 3, heads, 64), np.float64)
    pi = None
    if regime == "onehot":
        pi = np.zeros((n, heads, T), np.int64)
        for c in range(n):
            for h in range(heads):
                for _ in range(1000):
                    code = rng.choice(np.array([-1.0, 1.0]), (T, 64))
                    gram = code @ code.T
                    np.fill_diagonal(gram, -64)
                    if gram.max() <= 64 - ONEHOT_GAP:
                        break
                else:
                    raise RuntimeError(f"no code set with a gap of {ONEHOT_GAP} at T = {T}")
                pi[c, h] = rng.permutation(T)
                x[c, :, 0, h] = 4 * code[pi[c, h]]
                x[c, :, 1, h] = 2 * code
        x[:, :, 2] = rng.standard_normal((n, T, heads, 64))
    elif regime == "uniform":
        x[:, :, 1] = rng.standard_normal((n, T, heads, 64))
        x[:, :, 2] = rng.integers(-8, 9, (n, T, heads, 64))
    elif regime == "normal":
        x[:] = rng.standard_normal(x.shape) * 1.5
    elif regime == "peaked":
        x[:, :, :2] = rng.standard_normal((n, T, 2, heads, 64)) * np.sqrt(6.0)
        x[:, :, 2] = rng.standard_normal((n, T, heads, 64))
    else:
        raise ValueError(regime)
    return np.ascontiguousarray(x.reshape(n * T, 3 * D).astype(np.float16)), pi


def _qkv64(qkv, n, T, heads):
    x = qkv.astype(np.float64).reshape(n, T, 3, heads, 64)
    return x[:, :, 0], x[:, :, 1], x[:, :, 2]


def attn_reference(qkv, n: int, T: int, heads: int, exp_rel: float):
    """float64 softmax(q k^T / 8) v on the fp16 inputs, [n T][D], and the worst-case |error| of the kernels' evaluation.  Per query,
    with s_k the exact logits, m their maximum, p_k = exp(s_k - m), S = sum p_k, N = sum p_k v_k, o = N / S:
      logits    64 fp16 x fp16 products (exact in fp32) accumulated in fp32 on the matrix pipe, any order, twice the textbook as for the
                GEMMs: |s^_k - s_k| <= ds_k = 2 (64 + 2) u sum_d |q_d| |k_d| / 8 (the scale by 1 / 8 is exact).  The kernel subtracts ITS
                maximum m^: the common factor exp(m - m^) cancels between N^ and S^.  a_k = fl(s^_k - m^) adds u |s_k - m|.
      exp       p^_k = exp(a_k) (1 + e), |e| <= exp_rel (measured, see EXPF_FLOOR): relative perturbation of p_k
                    x_k = expm1(ds_k + u |s_k - m|) + exp_rel;   x_k = 1 for a key with p_k < 2**-24 (an fp16 zero or next to it, its
                    argument below the measured range: all of it uncertain -- it is at most 2**-24 of the sum)
      S^        the UNROUNDED fp32 p^_k summed in fp32, T terms any order:      |S^ - S| <= sum_k p_k (x_k + (T + 2) u)
      N^        fp16(p^_k): half an fp16 ulp AT p^_k <= p_k (1 + x_k) (2**-11 relative at most, 2**-25 absolute in the subnormals), the
                products accumulated in fp32 over the KP key slots:
                    |N^ - N| <= sum_k (p_k x_k + half_ulp16(p_k (1 + x_k)) + 2 (KP + 2) u p_k) |v_k|
      o^        |N^ / S^ - N / S| <= (|N^ - N| + |o| |S^ - S|) / (S - |S^ - S|), then the reciprocal and the product (u each), then
                the fp16 store
    """
    q, k, v = _qkv64(qkv, n, T, heads)
    s = np.einsum("nqhd,nkhd->nhqk", q, k) * 0.125
    mag = np.einsum("nqhd,nkhd->nhqk", np.abs(q), np.abs(k)) * 0.125
    a = s.max(-1, keepdims=True) - s
    p = np.exp(-a)
    S = p.sum(-1)
    o = np.einsum("nhqk,nkhd->nhqd", p, v) / S[..., None]
    xk = np.where(p < 2.0 ** -24, 1.0, np.expm1(2 * (64 + 2) * U24 * mag + U24 * a) + exp_rel)
    KP = -(-T // 32) * 32
    dN = np.einsum("nhqk,nkhd->nhqd", p * xk + half_ulp16(p * (1 + xk)) + 2 * (KP + 2) * U24 * p, np.abs(v))
    dS = (p * (xk + (T + 2) * U24)).sum(-1)
    assert (dS < 0.5 * S).all()
    b = (dN + np.abs(o) * dS[..., None]) / (S - dS)[..., None]
    b = b + 2 * U24 * (np.abs(o) + b)
    b = f16_store(o, b)
    back = lambda t: np.ascontiguousarray(t.transpose(0, 2, 1, 3)).reshape(n * T, 64 * heads)
    return back(o), back(b)


def attn_wrong_references(regime: str, qkv, n: int, T: int, heads: int) -> dict:
    """The attention controls, each a float64 softmax(.) v with ONE thing wrong.  Which regime takes which:
      scale 1 / sqrt(63)        normal, peaked   (uniform: q = 0, every logit is 0 under any scale)
      last valid key dropped    uniform, normal, peaked
      a zero pad key added      uniform, normal  (a key with logit 0 and v = 0 in the softmax; peaked: the maximum logit of every query is
                                above ~12, so a leaked zero logit weighs exp(-12) ~ 6e-6 of the sum -- less than half an fp16 ulp of the
                                output: not separable by ANY bound that admits the fp16 store)
      V keys swapped            normal, peaked   (keys 16..19 <-> 32..35 in V only; T < 36 has no such keys: 0..3 <-> 16..19 for
                                20 <= T < 36, key 0 <-> key T - 1 below; uniform: a mean does not see the order of its terms)
      softmax in fp16           peaked           (logits and probabilities rounded to fp16, the denominator summed from the rounded ones).
                                The one shape dropped: T = 2 -- two logits a standard deviation of 8.5 apart leave one probability at 1
                                for almost every query, and rounding the logits does not move a probability of 1
    """
    q, k, v = _qkv64(qkv, n, T, heads)
    back = lambda t: np.ascontiguousarray(t.transpose(0, 2, 1, 3)).reshape(n * T, 64 * heads)

    def sm(scale=0.125, keys=slice(None), pad=False, vv=v, half=False):
        s = np.einsum("nqhd,nkhd->nhqk", q, k[:, keys]) * scale
        if pad:
            s = np.concatenate([s, np.zeros(s.shape[:-1] + (1,))], -1)
        if half:
            s = s.astype(np.float16).astype(np.float64)
        p = np.exp(s - s.max(-1, keepdims=True))
        if half:
            p = p.astype(np.float16).astype(np.float64)
        S = p.sum(-1, keepdims=True)
        if pad:
            p = p[..., :-1]
        return back(np.einsum("nhqk,nkhd->nhqd", p, vv[:, keys]) / S)

    w = {}
    if regime in ("normal", "peaked"):
        w["scale 1/sqrt(63)"] = sm(scale=1 / np.sqrt(63.0))
        perm = np.arange(T)
        if T >= 36:
            perm[16:20], perm[32:36] = np.arange(32, 36), np.arange(16, 20)
        elif T >= 20:
            perm[0:4], perm[16:20] = np.arange(16, 20), np.arange(0, 4)
        else:
            perm[0], perm[T - 1] = T - 1, 0
        w["V keys swapped"] = sm(vv=v[:, perm])
    w["last key dropped"] = sm(keys=slice(0, T - 1))
    if regime in ("uniform", "normal"):
        w["zero pad key added"] = sm(pad=True)
    if regime == "peaked" and T > 2:
        w["softmax in fp16"] = sm(half=True)
    return w


def attn_launch(lib: ClipKatLib, qkv, n: int, T: int, heads: int, tmpl: bool):
    """runs k_clip_attention (tmpl False) or k_clip_attention_t<T> twice; the row after crop n - 1's token T - 1 is poison (and 7 more);
    returns the raw fp16 bits of the [n T] owned rows after the poison / guard / determinism checks"""
    D = 64 * heads
    label = f"{'k_clip_attention_t<%d>' % T if tmpl else 'k_clip_attention T=%d' % T} heads={heads} n={n}"
    X = _rows_then_poison(qkv, 8)
    rows = n * T
    C0 = _poison((rows + GUARD, D), False)

    def launch():
        C = C0.copy()
        if tmpl:
            return lib.lib.kat_clip_attention_t(T, X.ctypes.data, X.shape[0], C.ctypes.data, C.nbytes, n, D, heads), C
        return lib.lib.kat_clip_attention(X.ctypes.data, X.shape[0], C.ctypes.data, C.nbytes, n, T, D, heads), C

    C = _twice(label, launch)
    _owned(label, C, _first_rows(rows + GUARD, rows))
    return C[:rows]


def check_attention(label: str, regime: str, bits, qkv, pi, n: int, T: int, heads: int, exp_rel: float):
    """`bits`: a kernel's output (attn_launch).  onehot: row i of (crop, head) equals v[pi(i)] bit for bit -> (0, 0, []); uniform: the exact
    mean within 4 u (the reciprocal of T, the product, margin) and the fp16 store; normal / peaked: attn_reference's bound.  Returns
    (max err, max err / bound, controls caught)."""
    label = f"{label} [{regime}]"
    D = 64 * heads
    if regime == "onehot":
        v = qkv.view(np.uint16).reshape(n, T, 3, heads, 64)[:, :, 2]
        want = np.stack([np.stack([v[c, pi[c, h], h] for h in range(heads)], 1) for c in range(n)]).reshape(n * T, D)
        wrong = bits != want
        assert not wrong.any(), (f"{label}: {int(wrong.sum())} of {wrong.size} halves differ from v[pi(i)], first at row, column "
                                 f"{tuple(np.argwhere(wrong)[0])}")
        return 0.0, 0.0, []
    got = bits.view(np.float16).astype(np.float64)
    if regime == "uniform":
        want = np.repeat(_qkv64(qkv, n, T, heads)[2].mean(1, keepdims=True), T, 1).reshape(n * T, D)
        bnd = f16_store(want, 4 * U24 * np.abs(want))
    else:
        want, bnd = attn_reference(qkv, n, T, heads, exp_rel)
    stats = _inside(label, got, want, bnd)
    return (*stats, _caught(label, got, bnd, attn_wrong_references(regime, qkv, n, T, heads)))


def expf_probe_args() -> np.ndarray:
    """the arguments the attention cases hand to BM_EXPF that matter to a bound: fp32 values in [EXPF_ARG_MIN, 0] -- a dense grid, and the
    s - max of one peaked and one normal case"""
    xs = [np.linspace(EXPF_ARG_MIN, 0, 1 << 18)]
    for regime in ("normal", "peaked"):
        qkv, _ = attn_inputs(regime, 1, 192, 2, seed=5)
        q, k, _ = _qkv64(qkv, 1, 192, 2)
        s = (np.einsum("nqhd,nkhd->nhqk", q, k) * 0.125).astype(np.float32)
        a = (s - s.max(-1, keepdims=True)).ravel()
        xs.append(a[a >= EXPF_ARG_MIN])
    return np.ascontiguousarray(np.concatenate(xs).astype(np.float32))


def measure_expf(lib: ClipKatLib) -> float:
    """max relative error of BM_EXPF against float64 over expf_probe_args()"""
    x = expf_probe_args()
    y = np.full(x.shape, np.nan, np.float32)
    assert lib.lib.kat_expf(x.ctypes.data, y.ctypes.data, x.size) == 0
    ref = np.exp(x.astype(np.float64))
    assert np.isfinite(y).all()
    return float((np.abs(y.astype(np.float64) - ref) / ref).max())


def expf_bound(measured: float) -> float:
    return max(4 * measured, EXPF_FLOOR)


# ---------------------------------------------------------------------------------------------------------------------------------
# k_clip_head
# ---------------------------------------------------------------------------------------------------------------------------------
def head_reference(xc, P, variant: str | None = None, with_bound: bool = True):
    """xc: the class-token rows fp32 [n][D]; P: dict of ln gamma / beta, proj [D][E], bn_scale / bn_shift [D], bnp_scale / bnp_shift [E].
    float64 ln_post -> folded BatchNorm | projection -> folded BatchNorm -> concat -> L2, and the worst-case |error|:
      v     ln_post: ln_bound (bv)
      f1    fl(fl(v s1) + t1):  bv |s1| + u (|v s1| + |f1|)
      a     a SERIAL fp32 sum over D of fl(v_c P_ce): |a^ - a| <= bv . |P| + D u (|v| + bv) . |P|
      f2    fl(fl(a s2) + t2):  ba |s2| + u (|a s2| + |f2|)
      tot   sum f**2 over D + E terms (squares round, any order): bt = sum (2 |f| bf + bf**2) (1 + (D + E + 2) u) + (D + E + 2) u tot
      inv   tot ** -0.5: relative ri = bt / (2 (tot - bt)) + 3 u
      out   fl(f^ inv^): bf inv (1 + ri) + |f inv| (ri + u)
    variants (wrong references): 'no projection BN shift', 'L2 norm over the first D only'"""
    g = lambda k: P[k].astype(np.float64)
    D, E = P["proj"].shape
    v, bv = ln_bound(xc, P["gamma"], P["beta"])
    if not with_bound:
        bv = np.zeros_like(v)
    f1 = v * g("bn_scale") + g("bn_shift")
    b1 = bv * np.abs(g("bn_scale")) + U24 * (np.abs(v * g("bn_scale")) + np.abs(f1))
    a = v @ g("proj")
    ba = bv @ np.abs(g("proj")) + D * U24 * ((np.abs(v) + bv) @ np.abs(g("proj")))
    t2 = 0.0 if variant == "no projection BN shift" else g("bnp_shift")
    f2 = a * g("bnp_scale") + t2
    b2 = ba * np.abs(g("bnp_scale")) + U24 * (np.abs(a * g("bnp_scale")) + np.abs(f2))
    f, bf = np.concatenate([f1, f2], 1), np.concatenate([b1, b2], 1)
    tot = ((f[:, :D] if variant == "L2 norm over the first D only" else f) ** 2).sum(1, keepdims=True)
    e = (2 * np.abs(f) * bf + bf * bf).sum(1, keepdims=True)
    bt = e * (1 + (D + E + 2) * U24) + (D + E + 2) * U24 * tot
    ri = bt / (2 * (tot - bt)) + 3 * U24
    inv = 1.0 / np.sqrt(tot)
    out = f * inv
    return out, bf * inv * (1 + ri) + np.abs(out) * (ri + U24)


def run_head(lib: ClipKatLib, D: int, E: int, T: int, n: int, scattered: bool, seed: int = 0):
    """k_clip_head on n crops; out_rows scattered (non-monotone, with gaps, in an allocation of 2 n + 3 rows + guard) or null.  Every row
    of x except the class tokens is poison: the head reads x[crop][0] only.  Returns (max err, max err / bound, controls caught)."""
    label = f"k_clip_head D={D} E={E} T={T} n={n} out_rows={'scattered' if scattered else 'null'}"
    rng = np.random.default_rng(seed)
    xc = (rng.standard_normal((n, D)) * 1.3 + 0.2).astype(np.float32)
    X = _poison((n * T + 4, D), True)
    X[np.arange(n) * T] = xc.view(np.uint32)
    gamma, beta = ln_gain_bias(D, rng)
    bn = lambda m: (1.0 / np.sqrt(rng.uniform(0.02, 0.2, m)), rng.standard_normal(m) * 0.05)      # folded: scale, -mean * scale
    (s1, m1), (s2, m2) = bn(D), bn(E)
    P = dict(gamma=gamma, beta=beta, proj=(rng.standard_normal((D, E)) * D ** -0.5).astype(np.float32),
             bn_scale=s1.astype(np.float32), bn_shift=(-m1 * s1).astype(np.float32),
             bnp_scale=s2.astype(np.float32), bnp_shift=(-m2 * s2).astype(np.float32))
    P = {k: np.ascontiguousarray(a) for k, a in P.items()}
    total = (2 * n + 3 if scattered else n) + GUARD
    if scattered:
        rows = rng.permutation(2 * n + 3)[:n].astype(np.int32)
        if n >= 2 and np.all(np.diff(rows) > 0):
            rows = np.ascontiguousarray(rows[::-1])
    else:
        rows = np.arange(n, dtype=np.int32)
    C0 = _poison((total, D + E), True)

    def launch():
        C = C0.copy()
        return lib.lib.kat_clip_head(X.ctypes.data, X.shape[0], P["gamma"].ctypes.data, P["beta"].ctypes.data, P["proj"].ctypes.data,
                                     P["bn_scale"].ctypes.data, P["bn_shift"].ctypes.data, P["bnp_scale"].ctypes.data,
                                     P["bnp_shift"].ctypes.data, C.ctypes.data, total, rows.ctypes.data if scattered else None, n, T, D, E), C

    C = _twice(label, launch)
    owned = np.zeros(total, bool)
    owned[rows] = True
    _owned(label, C, owned)
    got = C[rows].view(np.float32).astype(np.float64)          # in crop order
    want, bnd = head_reference(xc, P)
    stats = _inside(label, got, want, bnd)
    # ||out|| = (1 + theta) ** -0.5 (1 + 2 u) (1 + u), |theta| <= (D + E + 1) u: the fp32 sum of squares the kernel normalises by, the
    # square root and reciprocal, and the final product per element
    nb = ((D + E) / 2 + 8) * U24
    norms = np.sqrt((got * got).sum(1))
    assert (np.abs(norms - 1) <= nb).all(), f"{label}: row norms off 1 by {np.abs(norms - 1).max():.3e} > {nb:.3e}"
    wrong = {k: head_reference(xc, P, k, with_bound=False)[0] for k in ("no projection BN shift", "L2 norm over the first D only")}
    return (*stats, _caught(label, got, bnd, wrong))
