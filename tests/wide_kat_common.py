"""Known-answer cases for the fp16 wide-OSNet kernels (ReID mode 1: boxmot_amd/csrc/osnet_wide_kernels.hpp, the stem packer of
osnet_wide_pack.hpp) run one kernel at a time through tests/kat/wide_kat.hip: shared by the device test (test_gpu_wide_kat.py) and its
CPU-thread emulation (test_wide_kat_emu.py).  Not a product path.

Regimes (every reference is float64 arithmetic on the operands as the kernel receives them):

* ``exact``     small integers: every intermediate is an integer that fp16 holds (|v| <= 2048) and every fp32 sum stays below 2**24, so the
                expected output is ``np.float16(float64 result)`` whatever the summation order.  The indexing test.  For the gate the
                pre-activations are 0 or +-200, where the fp32 sigmoid is exactly 0.5, 1 or 0 (exp overflows to inf, 1 / inf = 0).
* ``impulses``  a few non-zero input elements far enough apart that no output sees two of them, positive weights, zero bias: the output is
                the kernel's footprint, and every value is a single product that fp32 holds exactly, so the comparison is bit for bit too.
* ``random``    normal operands rounded to fp16 (fp32 where the kernel takes fp32), compared with the float64 result of the ROUNDED operands
                inside a deterministic per-element worst-case bound that holds for any fp32 summation order (derivations beside each
                reference below), so it never flakes.  U24 = 2**-24 is fp32's unit round-off, 2**-11 fp16's.

Around every launch (``_protocol``): every output allocation is prefilled with a NaN pattern and followed by guard elements that must still
hold it; no output may be NaN; every launch runs twice and must give the same bits; at n = 3 crop 1 runs alone as well and must equal crop
1 of the batch bit for bit.  The stem's input carries the 3-pixel zero border and the zero X channel of k_crop_resize_rgbx and NaNs after
the last crop.

The gate's sigmoid uses __expf on the device, whose error nobody has derived: MEASURED holds the largest |g - sigmoid64(v)| seen over
pre-activations in [-8, 8] (``measure_gate``), the bound allows 4 x that, and 4 x measured must stay below 2**-11 (the fp16 rounding it sits
under) -- otherwise it is a finding, not a constant to raise.

Controls (``controls``): the same comparisons must REJECT deliberately wrong references on the random inputs; no kernel runs.
"""
from __future__ import annotations

import ctypes
import subprocess
from pathlib import Path

import numpy as np

from gemm_kat_common import F16_POISON, F32_POISON, U24

ROOT = Path(__file__).resolve().parent.parent
KAT_SRC = Path(__file__).resolve().parent / "kat" / "wide_kat.hip"
U11 = 2.0 ** -11
F16_FLOOR = 2.0 ** -25             # half a step of fp16's subnormals
REGIMES = ("exact", "impulses", "random")

# largest |gate - sigmoid64| of k_gate_sum4 over 768 pre-activations in [-8, 8] (measure_gate subtracts the expected gate inside the kernel's
# own sum, so the fp16 store does not hide the figure).  "gpu": an MI355X, __expf; "emu": the CPU-thread emulation, libm's expf -- the
# same figure: the largest error sits at a gate near 1, where exp(-v) is small and the roundings of 1 + e and of the division (IEEE on
# both) decide.  The bound uses 4 x the figure (gate_allowance).  Through out = fp16(g) alone both show 2.439e-04, the fp16 rounding of g.
MEASURED = {
    "gpu": {"gate_dg": 8.524e-08},
    "emu": {"gate_dg": 8.524e-08},
}
DG_CAP = U11
SEEN: dict = {}                    # backend -> kernel -> largest error / bound ratio this process has seen


def gate_allowance(backend: str) -> float:
    m = MEASURED[backend]["gate_dg"]
    a = DG_CAP if m is None else 4 * m
    assert a <= DG_CAP, f"k_gate_sum4: 4 x measured gate error = {a:.3e} exceeds 2**-11: a finding to report, not a constant to raise"
    return a


def _note(backend: str, kernel: str, ratio: float):
    d = SEEN.setdefault(backend, {})
    d[kernel] = max(d.get(kernel, 0.0), ratio)


def report(backend: str):
    for k, r in sorted(SEEN.get(backend, {}).items()):
        print(f"RATIO {backend} {k:16s} largest error / bound so far {r:.3f}")


# ---------------------------------------------------------------------------------------------------------------------------------
# build, ctypes
# ---------------------------------------------------------------------------------------------------------------------------------
def build_gpu(out_dir: Path, timeout: float = 600) -> Path:
    """hipcc for gfx950 with the product's flags (__graft_entry__.HIPCC_FLAGS) -> out_dir/libwide_kat.so"""
    from __graft_entry__ import HIPCC_FLAGS

    out = Path(out_dir) / "libwide_kat.so"
    subprocess.run(["hipcc", *HIPCC_FLAGS, "-o", str(out), str(KAT_SRC)], check=True, timeout=timeout)
    return out


def build_emu(clang: str, out_dir: Path, timeout: float = 600) -> Path:
    """the same source on CPU threads (tests/host_emu/hip_shim.hpp), built as gemm_kat_common.build_emu builds its harness"""
    out = Path(out_dir) / "libwide_kat_emu.so"
    subprocess.run([clang, "-x", "c++", "-std=c++17", "-O1", "-fPIC", "-shared", "-pthread", "-ffp-contract=off", "-DKAT_EMU",
                    "-DEMU_DEFER_GLDS=1", "-o", str(out), str(KAT_SRC)], check=True, timeout=timeout)
    return out


class WideKatLib:
    """ctypes face of wide_kat.hip's entry points"""

    def __init__(self, path, backend: str):
        self.backend = backend
        self.lib = L = ctypes.CDLL(str(path))
        p, i, l = ctypes.c_void_p, ctypes.c_int, ctypes.c_long
        L.kat_wide_stem.argtypes = [i, p, l, i, p, p, p, l]
        L.kat_wide_light.argtypes = [i, p, p, p, p, p, l, p, l, i, i, i, i]
        L.kat_wide_gate.argtypes = [i, p, p, p, p, p, p, p, p, p, p, l, i, i, i]
        L.kat_wide_gap.argtypes = [p, p, l, i, i, i]
        L.kat_wide_l2.argtypes = [p, p, l, p, i, i]
        for f in (L.kat_wide_stem, L.kat_wide_light, L.kat_wide_gate, L.kat_wide_gap, L.kat_wide_l2):
            f.restype = ctypes.c_int


def _ptr(a):
    return None if a is None else a.ctypes.data


def _c(a, dt):
    return np.ascontiguousarray(a, dtype=dt)


# ---------------------------------------------------------------------------------------------------------------------------------
# the protocol around a launch
# ---------------------------------------------------------------------------------------------------------------------------------
GUARD = 64


def _poisoned(valid: int, f32: bool) -> np.ndarray:
    return np.full(valid + GUARD, F32_POISON if f32 else F16_POISON, np.uint32 if f32 else np.uint16)


def _values(what: str, raw: np.ndarray, valid: int) -> np.ndarray:
    """the guard after `valid` elements still holds the pattern, no NaN before it; returns the float64 values"""
    f32 = raw.dtype == np.uint32
    poison = F32_POISON if f32 else F16_POISON
    g = raw[valid:]
    assert g.size >= GUARD and np.all(g == poison), f"{what}: guard after the output written, first at element {valid + int(np.argwhere(g != poison)[0][0])}"
    v = raw[:valid].view(np.float32 if f32 else np.float16).astype(np.float64)
    bad = np.isnan(v)
    assert not bad.any(), f"{what}: {int(bad.sum())} NaN outputs (unwritten, or poison read), first at element {int(np.argwhere(bad)[0][0])}"
    return v


def _protocol(what: str, launch, inp: dict, n: int, crop_of):
    """launch(inp) -> {name: (raw bits, valid elements, elements per crop)}.  Twice (identical bits), guards and NaNs, and at n = 3 crop 1
    alone against crop 1 of the batch.  Returns {name: float64 values}."""
    a, b = launch(inp), launch(inp)
    out = {}
    for k, (raw, valid, per) in a.items():
        assert np.array_equal(raw, b[k][0]), f"{what}: two launches on the same inputs differ in {k}"
        out[k] = _values(f"{what} {k}", raw, valid)
    if n == 3:
        one = launch(crop_of(inp, 1))
        for k, (raw, valid, per) in one.items():
            _values(f"{what} {k} (crop 1 alone)", raw, valid)
            if per:
                same = np.array_equal(raw[:per], a[k][0][per:2 * per])
                assert same, f"{what}: {k} of crop 1 alone differs from crop 1 of the batch of 3 (crops are not independent)"
    return out


def _exact(what: str, got: np.ndarray, want64: np.ndarray, f32: bool = False):
    want = want64.astype(np.float32 if f32 else np.float16).astype(np.float64).reshape(got.shape)
    wrong = got != want
    if wrong.any():
        i = tuple(np.argwhere(wrong)[0])
        raise AssertionError(f"{what}: {int(wrong.sum())} of {wrong.size} outputs differ from the exact result, first at {i}: got {got[i]!r} want {want[i]!r}")
    return 0.0, 0.0


def _within(what: str, got: np.ndarray, want: np.ndarray, bnd: np.ndarray):
    want, bnd = want.reshape(got.shape), bnd.reshape(got.shape)
    err = np.abs(got - want)
    over = err > bnd
    if over.any():
        i = tuple(np.argwhere(over)[0])
        raise AssertionError(f"{what}: {int(over.sum())} of {over.size} outputs outside the bound, first at {i}: got {got[i]!r} want {want[i]!r} "
                             f"err {err[i]:.3e} > {bnd[i]:.3e}")
    return float(err.max()), float((err / bnd).max())


def _rejects(what: str, right: np.ndarray, wrong: np.ndarray, bnd: np.ndarray) -> int:
    """a control: the elements of a deliberately wrong reference the band around the right one rejects (an in-band output of the kernel
    is within bnd of `right`, so an element where |wrong - right| > 2 bnd cannot pass both)"""
    out = int((np.abs(wrong - right) > 2 * bnd).sum())
    print(f"CONTROL {what}: {out} of {right.size} elements outside the band")
    return out


def _sheets(wanted, clash, max_sheets):
    """first-fit of the wanted impulse positions into sheets (one sheet = one crop) so that no two of a sheet clash"""
    sheets = []
    for w in wanted:
        for s in sheets:
            if not any(clash(w, o) for o in s):
                s.append(w)
                break
        else:
            sheets.append([w])
    assert len(sheets) <= max_sheets, f"{len(sheets)} impulse sheets, {max_sheets} crops to hold them"
    return sheets + [[] for _ in range(max_sheets - len(sheets))]


# ---------------------------------------------------------------------------------------------------------------------------------
# k_wide_stem<C0>: conv 7x7 / 2, pad 3 + bias + ReLU + max pool 3x3 / 2, pad 1 on [n][262][136][4] -> [n][64 * 32][C0]
# ---------------------------------------------------------------------------------------------------------------------------------
SR, SC = 262, 136
STEM_ROWS = (0, 1, 7, 8, 64, 126, 127)            # conv rows / columns the impulses' conv maxima fall on: the first and last, the seams
STEM_COLS = (0, 1, 15, 16, 31, 32, 47, 48, 62, 63)     # of the 16-pixel tiles (DPP rows) and of the 8-row bands, just inside the borders


def stem_sheets():
    # two impulses may share no 7 x 7 window: conv positions 4 apart are input pixels 8 apart
    wanted = [(cy, cx) for cy in STEM_ROWS for cx in STEM_COLS]
    return _sheets(wanted, lambda a, b: abs(a[0] - b[0]) < 4 and abs(a[1] - b[1]) < 4, 4)


def stem_inputs(c0: int, regime: str, n: int, seed: int):
    rng = np.random.default_rng(seed)
    x = np.zeros((n, SR, SC, 4), np.float16)
    core = (n, 256, 128, 3)
    if regime == "exact":       # |sum| <= 147 * 4 + 64: integers fp16 holds
        x[:, 3:259, 3:131, :3] = rng.integers(-2, 3, core)
        w = rng.integers(-2, 3, (c0, 7, 7, 3)).astype(np.float32)
        bias = rng.integers(-64, 65, c0).astype(np.float32)
    elif regime == "random":    # fp32 weights: the packer's rounding to fp16 is under test too
        x[:, 3:259, 3:131, :3] = rng.standard_normal(core, np.float32)
        w = (rng.standard_normal((c0, 7, 7, 3), np.float32) / np.float32(np.sqrt(147.0))).astype(np.float32)
        bias = rng.standard_normal(c0, np.float32)
    else:
        # positive weights, the centre tap the largest: an impulse at padded pixel (2 cy + 3, 2 cx + 3) puts its conv maximum on (cy, cx);
        # power-of-two pixel values, so that every conv value is one exact product
        w = rng.uniform(0.5, 1.5, (c0, 7, 7, 3)).astype(np.float16).astype(np.float32)
        w[:, 3, 3, :] = rng.uniform(2.0, 3.0, (c0, 3)).astype(np.float16)
        bias = np.zeros(c0, np.float32)
        sheets = stem_sheets()
        use = sheets[:3] if n == 3 else sheets[3:4]
        k = 0
        for i, sheet in enumerate(use):
            for cy, cx in sheet:
                x[i, 2 * cy + 3, 2 * cx + 3, k % 3] = (1.0, 2.0, 0.5, 4.0)[k % 4]
                k += 1
        assert k > 0
    return dict(n=n, x=x, w=w, bias=bias)


def stem_crop(inp, i):
    return dict(inp, n=1, x=inp["x"][i:i + 1])


def stem_pool(r: np.ndarray, drop_tile_left: bool = False) -> np.ndarray:
    """3 x 3 / 2 max pool, pad 1, of non-negative [n][128][64][c] (a missing neighbour reads as 0); drop_tile_left: the control that loses the left
    neighbour where it lives in the previous 16-pixel tile (conv columns 16, 32, 48)"""
    rp = np.pad(r, ((0, 0), (1, 0), (1, 0), (0, 0)))
    out = np.zeros((r.shape[0], 64, 32, r.shape[3]))
    for dy in range(3):
        for dx in range(3):
            v = rp[:, dy:dy + 128:2, dx:dx + 64:2]
            if drop_tile_left and dx == 0:
                v = v.copy()
                v[:, :, [8, 16, 24]] = 0.0
            out = np.maximum(out, v)
    return out


def stem_conv(inp, with_bound=True):
    """float64 conv + bias + ReLU on [n][128][64][c0] and its bound.  Bound: the products of fp16 operands are exact in fp32; K = 147 of them
    and the bias are summed in fp32 in some order: (K + 1) U24 (sum |a||b| + |bias|); ReLU is 1-Lipschitz; the store rounds to fp16:
    2**-11 |ref|, or half a subnormal step."""
    x = inp["x"].astype(np.float64)[..., :3]
    w = inp["w"].astype(np.float16).astype(np.float64)           # the packer rounds to nearest even
    b = inp["bias"].astype(np.float64)
    conv = np.zeros((x.shape[0], 128, 64, w.shape[0])) + b
    mag = np.zeros_like(conv) + np.abs(b)
    for ky in range(7):
        for kx in range(7):
            p = x[:, ky:ky + 256:2, kx:kx + 128:2]
            conv += p @ w[:, ky, kx].T
            if with_bound:
                mag += np.abs(p) @ np.abs(w[:, ky, kx]).T
    r = np.maximum(conv, 0.0) + 0.0
    return r, U11 * r + 148 * U24 * mag + F16_FLOOR


def stem_reference(inp, with_bound=True):
    """pooled reference [n][2048][c0] and bound: max is monotone, so a pooled value moves by at most the largest bound in its window"""
    r, bnd = stem_conv(inp, with_bound)
    n, c0 = r.shape[0], r.shape[3]
    return stem_pool(r).reshape(n, 2048, c0), stem_pool(bnd).reshape(n, 2048, c0)


def stem_launch(lib: WideKatLib, c0: int, inp):
    n = inp["n"]
    x = np.full(n * SR * SC * 4 + SR * SC * 4, F16_POISON, np.uint16)        # one crop's worth of NaNs after the last crop
    x[:n * SR * SC * 4] = _c(inp["x"], np.float16).view(np.uint16).ravel()
    valid = n * 2048 * c0
    out = _poisoned(valid, False)
    w, bias = _c(inp["w"], np.float32), _c(inp["bias"], np.float32)
    st = lib.lib.kat_wide_stem(c0, _ptr(x), x.size, n, _ptr(w), _ptr(bias), _ptr(out), out.size)
    assert st == 0, f"k_wide_stem<{c0}>: launch status {st}"
    return {"out": (out, valid, 2048 * c0)}


def run_stem(lib: WideKatLib, c0: int, regime: str, n: int, seed: int = 0):
    what = f"k_wide_stem<{c0}> [{regime}] n={n}"
    inp = stem_inputs(c0, regime, n, seed)
    assert not inp["x"][:, :3].any() and not inp["x"][:, 259:].any() and not inp["x"][:, :, :3].any() and not inp["x"][:, :, 131:].any()
    assert not inp["x"][..., 3].any()
    got = _protocol(what, lambda i: stem_launch(lib, c0, i), inp, n, stem_crop)["out"].reshape(n, 2048, c0)
    want, bnd = stem_reference(inp, regime == "random")
    if regime != "random":
        if regime == "impulses":
            assert (want > 0).any() and (want == 0).any()
        return _exact(what, got, want)
    e, r = _within(what, got, want, bnd)
    _note(lib.backend, f"k_wide_stem<{c0}>", r)
    print(f"{what}: max error {e:.3e}, max error / bound {r:.3f}")
    return e, r


# ---------------------------------------------------------------------------------------------------------------------------------
# k_light_fused<C>: 1x1 (linear, fp16 result in LDS) -> depthwise 3x3 + bias + ReLU, bands of 8 rows; band sums of the fp16 outputs
# ---------------------------------------------------------------------------------------------------------------------------------
LIGHT_CASES = ((64, 64, 32), (32, 64, 32), (96, 32, 16), (128, 32, 16), (128, 16, 8), (96, 16, 8), (32, 16, 8))     # (C, H, W)


def light_groups(C: int, W: int) -> int:
    """light_map's row groups at 256 threads"""
    tpr, ng = W * C // 8, 1
    while ng * 2 <= 4 and ng * 2 * tpr <= 256:
        ng *= 2
    return ng


def light_sheets(C: int, H: int, W: int):
    rpg = 8 // light_groups(C, W)
    rows = {0, 7, 8, H - 1}
    for band0 in (0, H - 8):                       # both sides of every row-group split, in the first and the last band
        for g in range(1, 8 // rpg):
            rows |= {band0 + g * rpg - 1, band0 + g * rpg}
    cols = sorted({0, W - 1, W // 2})
    chans = (0, 7, 8, C - 1, 15, 16, 31, C // 2)
    wanted, k = [], 0
    for y in sorted(rows):
        for x in cols:
            wanted.append((y, x, chans[k % len(chans)]))
            k += 1
    # no output pixel (a 3 x 3 window) may see two impulses
    return _sheets(wanted, lambda a, b: abs(a[0] - b[0]) < 3 and abs(a[1] - b[1]) < 3, 4)


def light_inputs(C: int, H: int, W: int, regime: str, n: int, seed: int):
    rng = np.random.default_rng(seed)
    if regime == "exact":       # each 1x1 output: at most 8 terms of magnitude 1; |depthwise sum| <= 9 * 2 * 8 + 8; band sums < 2**24
        x = rng.integers(-1, 2, (n, H, W, C)).astype(np.float16)
        pw = np.zeros((C, C), np.float16)
        for co in range(C):
            pw[co, rng.choice(C, 8, replace=False)] = rng.choice([-1.0, 1.0], 8)
        dw = rng.integers(-2, 3, (C, 9)).astype(np.float32)
        bias = rng.integers(-8, 9, C).astype(np.float32)
    elif regime == "random":
        x = rng.standard_normal((n, H, W, C), np.float32).astype(np.float16)
        pw = (rng.standard_normal((C, C), np.float32) / np.float32(np.sqrt(C))).astype(np.float16)
        dw = (rng.standard_normal((C, 9), np.float32) / np.float32(3.0)).astype(np.float32)
        bias = (rng.standard_normal(C, np.float32) * np.float32(0.5)).astype(np.float32)
    else:
        # the 1x1 of one non-zero input is ONE product (exact in fp32, then the same fp16 rounding as the reference's), the nine taps are
        # distinct powers of two and every window sees one impulse: each output is an fp16 value times a power of two, exactly
        x = np.zeros((n, H, W, C), np.float16)
        pw = rng.uniform(0.5, 1.5, (C, C)).astype(np.float16)
        dw = np.tile(2.0 ** (np.arange(9) - 4), (C, 1)).astype(np.float32)
        bias = np.zeros(C, np.float32)
        sheets = light_sheets(C, H, W)
        use = sheets[:3] if n == 3 else (sheets[3:4] if sheets[3] else sheets[:1])
        k = 0
        for i, sheet in enumerate(use):
            for y, xx, c in sheet:
                x[i, y, xx, c] = (1.0, 1.5, 2.0, 3.0, 0.75)[k % 5]
                k += 1
        assert k > 0
    return dict(n=n, x=x, pw=pw, dw=dw, bias=bias)


def light_crop(inp, i):
    return dict(inp, n=1, x=inp["x"][i:i + 1])


def light_reference(inp, with_bound=True, halo_zero=False, wrap=False, no_round=False):
    """float64 reference [n][H][W][C] and bound.  The 1x1 result is rounded to fp16 as the kernel stores it in LDS (not with no_round: a
    control), the depthwise 3x3 is float64.
    Bound: the kernel's intermediate T' differs from the reference's T = fp16(exact) by its fp32 accumulation error pushed through one
    fp16 rounding.  Rounding is monotone and T, T' lie on the fp16 grid, so |T' - T| <= e + one fp16 step at T, with
    e = (C + 1) U24 sum |x||pw| (C exact products summed in fp32, any order): dT = e + 2**-10 |T| + 2**-24 (the subnormal step).
    The nine taps: sum |w_k| dT_k; the fp32 products and the ten additions (bias included): 10 U24 (sum |w_k||T_k| + |bias|); ReLU is
    1-Lipschitz; the store: 2**-11 (|ref| + everything before), or half a subnormal step.  A reference below its bound may come out as 0.
    Controls: halo_zero reads the row above / below every band as zero; wrap takes column neighbours modulo W instead of zero."""
    x, pw = inp["x"].astype(np.float64), inp["pw"].astype(np.float64)
    dw, bias = inp["dw"].astype(np.float64), inp["bias"].astype(np.float64)
    n, H, W, C = x.shape
    T = x @ pw.T
    if not no_round:
        T = T.astype(np.float16).astype(np.float64)
    dT = ((C + 1) * U24 * (np.abs(x) @ np.abs(pw).T) + 2.0 ** -10 * np.abs(T) + U24) if with_bound else np.zeros_like(T)

    def tile(a):                # [n][bands][10][W + 2][C]: every band with its halo rows and the two outside columns
        a = np.pad(a, ((0, 0), (1, 1), (0, 0), (0, 0)))
        t = np.stack([a[:, r0:r0 + 10] for r0 in range(0, H, 8)], axis=1)
        if halo_zero:
            t = t.copy()
            t[:, :, 0] = 0.0
            t[:, :, 9] = 0.0
        return np.pad(t, ((0, 0), (0, 0), (0, 0), (1, 1), (0, 0)), mode="wrap" if wrap else "constant")

    tT, tD = tile(T), tile(dT)
    acc = np.zeros((n, H // 8, 8, W, C)) + bias
    mag = np.zeros_like(acc) + np.abs(bias)
    prop = np.zeros_like(acc)
    for dy in range(3):
        for dx in range(3):
            wk = dw[:, 3 * dy + dx]
            acc += tT[:, :, dy:dy + 8, dx:dx + W] * wk
            if with_bound:
                mag += np.abs(tT[:, :, dy:dy + 8, dx:dx + W] * wk)
                prop += tD[:, :, dy:dy + 8, dx:dx + W] * np.abs(wk)
    ref = (np.maximum(acc, 0.0) + 0.0).reshape(n, H, W, C)
    b = (prop + 10 * U24 * mag).reshape(n, H, W, C)
    return ref, b + U11 * (ref + b) + F16_FLOOR


def light_launch(lib: WideKatLib, inp, use_gap: bool):
    x = _c(inp["x"], np.float16)
    n, H, W, C = x.shape
    valid, gvalid = n * H * W * C, n * (H // 8) * C
    out, gap = _poisoned(valid, False), _poisoned(gvalid, True)
    pw, dw, bias = _c(inp["pw"], np.float16), _c(inp["dw"], np.float32), _c(inp["bias"], np.float32)
    st = lib.lib.kat_wide_light(C, _ptr(x), _ptr(pw), _ptr(dw), _ptr(bias), _ptr(out), out.size, _ptr(gap), gap.size, int(use_gap), n, H, W)
    assert st == 0, f"k_light_fused<{C}> H={H} W={W}: launch status {st}"
    if not use_gap:
        assert np.all(gap == F32_POISON), f"k_light_fused<{C}> H={H} W={W}: gap_part written although the kernel got a null pointer"
        return {"out": (out, valid, H * W * C)}
    return {"out": (out, valid, H * W * C), "gap": (gap, gvalid, (H // 8) * C)}


def run_light(lib: WideKatLib, case, regime: str, n: int, seed: int = 0):
    C, H, W = case
    what = f"k_light_fused<{C}> H={H} W={W} [{regime}] n={n}"
    inp = light_inputs(C, H, W, regime, n, seed)
    o = _protocol(what, lambda i: light_launch(lib, i, True), inp, n, light_crop)
    bare = light_launch(lib, inp, False)["out"][0]
    got = o["out"].reshape(n, H, W, C)
    assert np.array_equal(bare[:got.size].view(np.float16).astype(np.float64).reshape(got.shape), got) and np.all(bare[got.size:] == F16_POISON), \
        f"{what}: the outputs with and without gap_part differ"
    # the band sums against the kernel's OWN fp16 outputs: exact in float64; 8 W terms summed in fp32: 8 W U24 sum |o|
    own = got.reshape(n, H // 8, 8 * W, C)
    gsum, gbnd = own.sum(axis=2), 8 * W * U24 * np.abs(own).sum(axis=2) + 2.0 ** -149
    gap = o["gap"].reshape(n, H // 8, C)
    want, bnd = light_reference(inp, regime == "random")
    if regime != "random":
        if regime == "impulses":
            assert (want > 0).any() and (want == 0).any()
        _exact(what, got, want)
        if regime == "exact":
            _exact(what + " gap_part", gap, gsum, f32=True)
        else:
            _within(what + " gap_part", gap, gsum, gbnd)
        return 0.0, 0.0
    e, r = _within(what, got, want, bnd)
    ge, gr = _within(what + " gap_part", gap, gsum, gbnd)
    _note(lib.backend, f"k_light_fused<{C}>", r)
    _note(lib.backend, "light gap_part", gr)
    print(f"{what}: max error {e:.3e}, max error / bound {r:.3f}; gap_part {ge:.3e}, {gr:.3f}")
    return e, r


# ---------------------------------------------------------------------------------------------------------------------------------
# k_gate_sum4<C>: out = sum_b x_b * sigmoid(fc2(relu(fc1(sum_bands gap_part[b] / P))))
# ---------------------------------------------------------------------------------------------------------------------------------
def gate_inputs(C: int, P: int, nbands: int, regime: str, n: int, seed: int):
    rng = np.random.default_rng(seed)
    hid = C // 16
    if regime == "exact":
        # integer means in -2 .. 2 from band sums that differ per branch, crop, band and channel; integer fc1; fc2 in multiples of 200, so
        # that every pre-activation is 0 or at least 200 in magnitude: the fp32 sigmoid is exactly 0.5, 1 or 0.  |out| <= 4 * 64
        x = rng.integers(-64, 65, (4, n, P, C)).astype(np.float16)
        mean = rng.integers(-2, 3, (4, n, C))
        gap = rng.integers(-1000, 1001, (4, n, nbands, C))
        gap[:, :, -1] = mean * P - gap[:, :, :-1].sum(axis=2)
        gap = gap.astype(np.float32)
        fc1_w = np.zeros((hid, C), np.float32)
        for k in range(hid):
            fc1_w[k, rng.choice(C, 4, replace=False)] = rng.choice([-1.0, 1.0], 4)
        fc1_b = rng.integers(-2, 3, hid).astype(np.float32)
        fc2_w = (200 * rng.integers(-1, 2, (C, hid))).astype(np.float32)
        fc2_b = (200 * rng.integers(-1, 2, C)).astype(np.float32)
    else:
        x = rng.standard_normal((4, n, P, C), np.float32).astype(np.float16)
        gap = (rng.standard_normal((4, n, nbands, C), np.float32) * np.float32(P / nbands)).astype(np.float32) + np.float32(0.5 * P / nbands)
        fc1_w = (rng.standard_normal((hid, C), np.float32) / np.float32(np.sqrt(C))).astype(np.float32)
        fc1_b = (rng.standard_normal(hid, np.float32) * np.float32(0.1)).astype(np.float32)
        fc2_w = (rng.standard_normal((C, hid), np.float32) * np.float32(2.0 / np.sqrt(hid))).astype(np.float32)
        fc2_b = rng.standard_normal(C, np.float32)
    return dict(n=n, P=P, nbands=nbands, x=x, gap=gap, fc1_w=fc1_w, fc1_b=fc1_b, fc2_w=fc2_w, fc2_b=fc2_b)


def gate_crop(inp, i):
    return dict(inp, n=1, x=inp["x"][:, i:i + 1], gap=inp["gap"][:, i:i + 1])


def gate_values(inp, dg: float = 0.0, swap=False, mean_over_bands=False):
    """float64 gates [4][n][C] and their bound.  fp32 throughout in the kernel:
      mean   nbands - 1 additions and the division: (nbands + 1) U24 sum |gap| / P
      fc1    C products, C additions onto the bias: carried error sum |w| dmean + (C + 2) U24 (|b| + sum |w||mean|); ReLU is 1-Lipschitz
      fc2    the same with HID terms
      gate   the sigmoid's slope is at most 1 / 4: dv / 4, plus `dg` for exp, the addition and the division at an exact argument
    Controls: swap exchanges the band sums of branches 1 and 2; mean_over_bands divides by nbands instead of P."""
    gp = inp["gap"].astype(np.float64)
    if swap:
        gp = gp[[0, 2, 1, 3]]
    P, nb = inp["P"], inp["nbands"]
    div = nb if mean_over_bands else P
    f1w, f1b = inp["fc1_w"].astype(np.float64), inp["fc1_b"].astype(np.float64)
    f2w, f2b = inp["fc2_w"].astype(np.float64), inp["fc2_b"].astype(np.float64)
    hid, C = f1w.shape
    mean = gp.sum(axis=2) / div
    dmean = (nb + 1) * U24 * np.abs(gp).sum(axis=2) / div
    pre = f1b + mean @ f1w.T
    dh = dmean @ np.abs(f1w).T + (C + 2) * U24 * (np.abs(f1b) + np.abs(mean) @ np.abs(f1w).T)
    h = np.maximum(pre, 0.0)
    v = f2b + h @ f2w.T
    dv = dh @ np.abs(f2w).T + (hid + 2) * U24 * (np.abs(f2b) + h @ np.abs(f2w).T)
    with np.errstate(over="ignore"):
        g = 1.0 / (1.0 + np.exp(-v))
    return g, dv / 4 + dg, v


def gate_reference(inp, dg: float = 0.0, **wrong):
    """out [n][P][C] and bound: sum_b |x_b| dg_b; four fp32 products and three additions: 4 U24 sum |x_b| g_b; the fp16 store"""
    g, dgv, _ = gate_values(inp, dg, **wrong)
    x = inp["x"].astype(np.float64)
    out = (x * g[:, :, None, :]).sum(axis=0) + 0.0
    b = (np.abs(x) * dgv[:, :, None, :]).sum(axis=0) + 4 * U24 * (np.abs(x) * g[:, :, None, :]).sum(axis=0)
    return out, b + U11 * (np.abs(out) + b) + F16_FLOOR


def gate_launch(lib: WideKatLib, inp):
    x = [_c(inp["x"][b], np.float16) for b in range(4)]
    n, P, C = x[0].shape
    valid = n * P * C
    out = _poisoned(valid, False)
    gap = _c(inp["gap"], np.float32)
    f = [_c(inp[k], np.float32) for k in ("fc1_w", "fc1_b", "fc2_w", "fc2_b")]
    st = lib.lib.kat_wide_gate(C, *[_ptr(a) for a in x], _ptr(gap), *[_ptr(a) for a in f], _ptr(out), out.size, P, inp["nbands"], n)
    assert st == 0, f"k_gate_sum4<{C}>: launch status {st}"
    return {"out": (out, valid, P * C)}


def run_gate(lib: WideKatLib, C: int, P: int, nbands: int, regime: str, n: int, seed: int = 0):
    what = f"k_gate_sum4<{C}> P={P} nbands={nbands} [{regime}] n={n}"
    inp = gate_inputs(C, P, nbands, regime, n, seed)
    got = _protocol(what, lambda i: gate_launch(lib, i), inp, n, gate_crop)["out"].reshape(n, P, C)
    if regime == "exact":
        v = gate_values(inp)[2]
        assert (np.abs(v[v != 0]) >= 200).all() and (v == 0).any() and (v > 0).any() and (v < 0).any()
        g = np.where(v > 0, 1.0, np.where(v < 0, 0.0, 0.5))      # fp32: exp(-200) + 1 = 1, exp(200) = inf and 1 / inf = 0
        return _exact(what, got, (inp["x"].astype(np.float64) * g[:, :, None, :]).sum(axis=0) + 0.0)
    want, bnd = gate_reference(inp, gate_allowance(lib.backend))
    e, r = _within(what, got, want, bnd)
    _note(lib.backend, f"k_gate_sum4<{C}>", r)
    print(f"{what}: max error {e:.3e}, max error / bound {r:.3f}")
    return e, r


def measure_gate(lib: WideKatLib, n: int = 1):
    """The gate alone, C = 128, P = 128, two bands: branch b's mean is 1 in channel 0 and fc1 passes it on, so its pre-activation in
    channel c is the fp32 number fc2_w[c][0] (spread over [-8, 8], no arithmetic error before the sigmoid); the other branches' are 0 and
    their gates 1 / (1 + exp(-0)) = 0.5.
      coarse  x_b = 1, the others 0 (out = fp16(g_b)): asserted within 2**-11 g + the allowance of sigmoid64, every branch
      fine    an fp16 output cannot resolve the gate's error, so the expected gate is subtracted before the store: x_b = 1024, a second
              branch holds -2048 q1 with q1 = fp16(sigmoid64) and a LATER branch x2 = fp16(-2048 (sigmoid64 - q1)) =: -2048 q2.  The
              kernel adds the branches in index order: 1024 g_b and -1024 q1 are exact products whose sum is exact (neighbours in
              fp16), then -1024 q2 arrives and out = fp16(1024 (g_b - q1 - q2)), a number of a few 1e-4 at most whose fp16 rounding is
              below 1e-10 of g.  g_b = out / 1024 + q1 + q2 in float64.  Branches 0 .. 2 (the third term has to come last), two
              grids of 128 pre-activations each.
    Returns the largest |g_b - sigmoid64| of the fine runs."""
    C, P, nb, hid = 128, 128, 2, 8
    worst = coarse = 0.0
    allow = gate_allowance(lib.backend)
    fc1_w = np.zeros((hid, C), np.float32)
    fc1_w[0, 0] = 1.0
    for b in range(4):
        for grid in range(2):
            v32 = (-8.0 + 16.0 * (np.arange(C) + b / 4.0 + grid / 8.0) / C).astype(np.float32)
            if b == 0 and grid == 0:
                v32[:3] = (-8.0, 8.0, 0.0)
            fc2_w = np.zeros((C, hid), np.float32)
            fc2_w[:, 0] = v32
            gap = np.zeros((4, n, nb, C), np.float32)
            gap[b, :, :, 0] = P / nb
            inp = dict(n=n, P=P, nbands=nb, gap=gap, fc1_w=fc1_w, fc1_b=np.zeros(hid, np.float32), fc2_w=fc2_w, fc2_b=np.zeros(C, np.float32))
            g64 = 1.0 / (1.0 + np.exp(-v32.astype(np.float64)))
            what = f"k_gate_sum4<{C}> gate of branch {b}, grid {grid}"
            x = np.zeros((4, n, P, C), np.float16)
            x[b] = 1.0
            inp["x"] = x
            got = _protocol(what + " (coarse)", lambda i: gate_launch(lib, i), inp, n, gate_crop)["out"].reshape(n, P, C)
            _within(what + " (coarse)", got, np.broadcast_to(g64, got.shape), np.broadcast_to(U11 * g64 + F16_FLOOR + allow, got.shape))
            coarse = max(coarse, float(np.abs(got - g64).max()))
            if b == 3:
                continue
            b1, b2 = ((1, 2), (0, 2), (0, 3))[b]
            q1 = g64.astype(np.float16).astype(np.float64)
            x2 = (-2048.0 * (g64 - q1)).astype(np.float16)
            q2 = x2.astype(np.float64) / -2048.0
            x = np.zeros((4, n, P, C), np.float16)
            x[b] = 1024.0
            x[b1] = (-2048.0 * q1).astype(np.float16)
            x[b2] = x2
            assert np.array_equal(x[b1, 0, 0].astype(np.float64), -2048.0 * q1)
            inp["x"] = x
            got = _protocol(what + " (fine)", lambda i: gate_launch(lib, i), inp, n, gate_crop)["out"].reshape(n, P, C)
            assert np.abs(got).max() < 1.0, f"{what}: the residual 1024 (g - q1 - q2) = {np.abs(got).max()} is no residual"
            worst = max(worst, float(np.abs(got / 1024.0 + q1 + q2 - g64).max()))
    have = MEASURED[lib.backend]["gate_dg"]
    print(f"MEASURED {lib.backend} gate_dg {worst:.3e} (through fp16(g) alone: {coarse:.3e})" +
          (f"   table {have:.3e}, allowance {4 * have:.3e}, ratio {worst / (4 * have):.3f}" if have else "   no table entry yet"))
    assert 4 * worst <= DG_CAP, f"4 x the measured gate error {worst:.3e} exceeds 2**-11"
    assert worst <= allow, f"the gate's error {worst:.3e} exceeds the allowance {allow:.3e} (4 x MEASURED)"
    return worst


# ---------------------------------------------------------------------------------------------------------------------------------
# k_wide_gap: out[n][c] = fp16(sum_p in[n][p][c] / P);  k_wide_l2: out[row(n)] = v[n] / |v[n]|
# ---------------------------------------------------------------------------------------------------------------------------------
def run_gap(lib: WideKatLib, C: int, P: int, regime: str, n: int, seed: int = 0):
    what = f"k_wide_gap C={C} P={P} [{regime}] n={n}"
    rng = np.random.default_rng(seed)
    if regime == "exact":       # |sum| <= 8 P = 1024: an integer fp16 holds, and so is its quotient by the power of two P
        x = rng.integers(-8, 9, (n, P, C)).astype(np.float16)
    else:
        x = (rng.standard_normal((n, P, C), np.float32) + np.float32(0.5)).astype(np.float16)

    def launch(inp):
        a = _c(inp["x"], np.float16)
        out = _poisoned(a.shape[0] * C, False)
        st = lib.lib.kat_wide_gap(_ptr(a), _ptr(out), out.size, a.shape[0], P, C)
        assert st == 0, f"{what}: launch status {st}"
        return {"out": (out, a.shape[0] * C, C)}

    got = _protocol(what, launch, dict(x=x), n, lambda inp, i: dict(x=inp["x"][i:i + 1]))["out"].reshape(n, C)
    x64 = x.astype(np.float64)
    want = x64.sum(axis=1) / P
    if regime == "exact":
        return _exact(what, got, want)
    # P - 1 additions and the division in fp32: (P + 1) U24 sum |x| / P; then the fp16 store
    b = (P + 1) * U24 * np.abs(x64).sum(axis=1) / P
    e, r = _within(what, got, want, b + U11 * (np.abs(want) + b) + F16_FLOOR)
    _note(lib.backend, "k_wide_gap", r)
    print(f"{what}: max error {e:.3e}, max error / bound {r:.3f}")
    return e, r


def run_l2(lib: WideKatLib, F: int, regime: str, n: int, scatter: bool, seed: int = 0):
    what = f"k_wide_l2 F={F} [{regime}] n={n}{' scattered' if scatter else ''}"
    rng = np.random.default_rng(seed)
    if regime == "exact":       # 4**j entries of +-2**e per row: the squares and their sum are powers of two, the norm 2**(j + e), the quotients +-2**-j
        v = np.zeros((n, F), np.float32)
        for i in range(n):
            cnt = 4 ** (i % 4)
            v[i, rng.choice(F, cnt, replace=False)] = rng.choice([-1.0, 1.0], cnt) * 2.0 ** ((i % 5) - 2)
    else:                       # no all-zero row: the kernel and the reference both divide by zero there
        v = rng.standard_normal((n, F), np.float32)
        v[:, ::3] = 0.0
        v[:, 1] = 1.0
    table = 2 * n + 3 if scatter else n
    rows = rng.permutation(table)[:n].astype(np.int32) if scatter else None

    def launch(inp):
        a = _c(inp["v"], np.float32)
        out = _poisoned(table * F, True)
        st = lib.lib.kat_wide_l2(_ptr(a), _ptr(out), out.size, _ptr(rows), a.shape[0], F)
        assert st == 0, f"{what}: launch status {st}"
        return {"out": (out, 0, 0)}             # the table is checked row by row below

    a, b = launch(dict(v=v))["out"][0], launch(dict(v=v))["out"][0]
    assert np.array_equal(a, b), f"{what}: two launches on the same inputs differ"
    assert np.all(a[table * F:] == F32_POISON), f"{what}: guard after the table written"
    tab = a[:table * F].reshape(table, F)
    dest = rows if scatter else np.arange(n)
    rest = np.setdiff1d(np.arange(table), dest)
    assert np.all(tab[rest] == F32_POISON), f"{what}: rows outside out_rows written: {rest[np.any(tab[rest] != F32_POISON, axis=1)]}"
    got = tab[dest].view(np.float32).astype(np.float64)
    assert not np.isnan(got).any(), f"{what}: NaN outputs in rows {np.argwhere(np.isnan(got).any(axis=1)).ravel()}"
    v64 = v.astype(np.float64)
    want = v64 / np.sqrt((v64 * v64).sum(axis=1, keepdims=True))
    if regime == "exact":
        return _exact(what, got, want, f32=True)
    # F squares (one rounding each) and F - 1 additions of non-negative terms: the sum is within (F + 1) U24 relative, its root within half
    # of that plus the root's own rounding, the quotient one more: |ref| U24 ((F + 1) / 2 + 2), doubled for the second-order terms
    e, r = _within(what, got, want, np.abs(want) * U24 * ((F + 1) / 2 + 2) * 2 + 2.0 ** -149)
    _note(lib.backend, "k_wide_l2", r)
    print(f"{what}: max error {e:.3e}, max error / bound {r:.3f}")
    return e, r


# ---------------------------------------------------------------------------------------------------------------------------------
# controls: wrong references the comparisons must reject (CPU only, no kernel)
# ---------------------------------------------------------------------------------------------------------------------------------
def controls():
    """{name: elements of the wrong reference outside the band}.  `light unrounded` holds one count per regime: the caller reports them
    and asserts nothing about them."""
    res = {}
    inp = light_inputs(32, 16, 8, "random", 1, 5)
    right, bnd = light_reference(inp)
    name = "k_light_fused<32> H=16 W=8 [random] n=1"
    res["light halo rows zeroed"] = _rejects(f"{name}: halo row of every band zeroed", right, light_reference(inp, halo_zero=True)[0], bnd)
    res["light columns wrapped"] = _rejects(f"{name}: column neighbours wrapped", right, light_reference(inp, wrap=True)[0], bnd)
    unrounded = {}
    for regime in REGIMES:
        i2 = light_inputs(32, 16, 8, regime, 1, 5)
        r2, b2 = light_reference(i2, regime == "random")
        w2 = light_reference(i2, False, no_round=True)[0]
        if regime == "random":
            unrounded[regime] = _rejects(f"k_light_fused<32> H=16 W=8 [{regime}] n=1: intermediate not rounded to fp16", r2, w2, b2)
        else:
            unrounded[regime] = int((r2.astype(np.float16) != w2.astype(np.float16)).sum())
            print(f"CONTROL k_light_fused<32> H=16 W=8 [{regime}] n=1: intermediate not rounded to fp16: {unrounded[regime]} of {r2.size} elements differ "
                  f"from the exact expectation")
    res["light unrounded"] = unrounded
    inp = stem_inputs(32, "random", 1, 6)
    conv, cb = stem_conv(inp)
    right, bnd = stem_pool(conv), stem_pool(cb)
    name = "k_wide_stem<32> [random] n=1"
    res["stem tile-left neighbour dropped"] = _rejects(f"{name}: left neighbour at conv columns 16, 32, 48 dropped", right, stem_pool(conv, True), bnd)
    # conv rounded to fp16 BEFORE the ReLU and the pool: rounding is monotone and keeps 0, so it commutes with both -- the same outputs
    early = stem_pool(np.maximum(conv.astype(np.float16).astype(np.float64), 0.0))
    res["stem relu on fp16"] = int((early.astype(np.float16) != right.astype(np.float16)).sum())
    print(f"CONTROL {name}: conv, then ReLU on fp16: {res['stem relu on fp16']} of {right.size} fp16 outputs differ (an equivalent order, not an error)")
    inp = gate_inputs(32, 128, 2, "random", 1, 7)
    right, bnd = gate_reference(inp, gate_allowance("gpu"))
    name = "k_gate_sum4<32> P=128 nbands=2 [random] n=1"
    res["gate branches swapped"] = _rejects(f"{name}: band sums of branches 1 and 2 swapped", right, gate_reference(inp, swap=True)[0], bnd)
    res["gate mean over nbands"] = _rejects(f"{name}: mean over nbands instead of P", right, gate_reference(inp, mean_over_bands=True)[0], bnd)
    return res
