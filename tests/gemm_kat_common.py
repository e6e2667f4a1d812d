"""Known-answer cases for the fp16 GEMM family (boxmot_amd/csrc/gemm_f16.hpp) run through tests/kat/gemm_kat.hip: shared by the device
test (test_gpu_gemm_kat.py) and its CPU-thread emulation (test_gemm_kat_emu.py).  Not a product path.

A case is one launch of one kernel instantiation at (M, N, K) with its epilogue options.  Two input regimes:

* ``exact``: small integers in fp16 (bias, residual and the EPI 2 prefill integers too).  Every partial sum is an integer below 2**24,
  so the fp32 accumulation is exact whatever its order and the expected output is the fp64 product: fp32 outputs equal it, fp16
  outputs equal ``np.float16(exact)`` (the one RNE rounding the kernel's store does).  QuickGELU (EPI 1) is not in this regime.
* ``random``: normal operands rounded to fp16, compared with the fp64 product of the rounded operands within a deterministic
  per-element worst-case bound (``bound`` below): it holds for any summation order with fp32 roundings, so it never flakes.

Around every launch: the output allocation is prefilled with a NaN bit pattern and followed by guard rows (up to the next 256-row tile
boundary and 8 more) that must still hold it afterwards (rows >= M are skipped on store); X (and X2, the residual) carry NaN rows after
row M - 1 up to that boundary (rows >= M are clamped on load, so no output may be NaN); each launch runs twice and must give the same
bits.
"""
from __future__ import annotations

import ctypes
import subprocess
from dataclasses import dataclass
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
KAT_SRC = Path(__file__).resolve().parent / "kat" / "gemm_kat.hip"
F16_POISON = np.uint16(0x7E5A)              # a quiet NaN no arithmetic produces
F32_POISON = np.uint32(0x7FC05A5A)
U24 = 2.0 ** -24


def build_gpu(out_dir: Path, timeout: float = 600) -> Path:
    """hipcc for gfx950 with the product's flags (__graft_entry__.HIPCC_FLAGS) -> out_dir/libgemm_kat.so"""
    from __graft_entry__ import HIPCC_FLAGS

    out = Path(out_dir) / "libgemm_kat.so"
    subprocess.run(["hipcc", *HIPCC_FLAGS, "-o", str(out), str(KAT_SRC)], check=True, timeout=timeout)
    return out


def build_emu(clang: str, out_dir: Path, defines=(), timeout: float = 600) -> Path:
    """the same source on CPU threads (fiber mode, global -> LDS copies deferred to the waits: tests/host_emu/hip_shim.hpp)"""
    tag = "_".join(d.replace("=", "") for d in defines) or "base"
    out = Path(out_dir) / f"libgemm_kat_emu_{tag}.so"
    subprocess.run([clang, "-x", "c++", "-std=c++17", "-O1", "-fPIC", "-shared", "-pthread", "-ffp-contract=off", "-DKAT_EMU",
                    "-DEMU_DEFER_GLDS=1", *[f"-D{d}" for d in defines], "-o", str(out), str(KAT_SRC)], check=True, timeout=timeout)
    return out


class KatLib:
    """ctypes face of gemm_kat.hip's entry points"""

    _COMMON = [ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p,
               ctypes.c_long, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int]
    _EXT = [ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p, ctypes.c_int, ctypes.c_int]

    def __init__(self, path):
        self.lib = ctypes.CDLL(str(path))
        L = self.lib
        L.kat_gemm_f16.argtypes = [ctypes.c_int, ctypes.c_int] + self._COMMON
        L.kat_gemm_glds.argtypes = [ctypes.c_int, ctypes.c_int] + self._COMMON + self._EXT
        L.kat_gemm_256.argtypes = [ctypes.c_int] + self._COMMON
        L.kat_clip_gemm.argtypes = [ctypes.c_int] + self._COMMON
        L.kat_wide_gemm.argtypes = self._COMMON + self._EXT
        L.kat_clip_route.argtypes = [ctypes.c_long, ctypes.c_int, ctypes.c_int]
        L.kat_wide_route.argtypes = [ctypes.c_int] * 4
        for f in (L.kat_gemm_f16, L.kat_gemm_glds, L.kat_gemm_256, L.kat_clip_gemm, L.kat_wide_gemm, L.kat_clip_route, L.kat_wide_route):
            f.restype = ctypes.c_int


@dataclass(frozen=True)
class Case:
    kind: str           # "f16" (k_gemm_f16<epi, param>), "glds" (k_gemm_f16_glds<epi, param>), "256" (k_gemm_f16_256<epi>),
    epi: int            # "clip" (ClipNet::gemm's dispatch, epi 0..3), "wide" (WideOsNet::gemm's dispatch: epi 4, or 5 / 6 with pool_w)
    param: int
    M: int
    N: int
    K: int
    relu: int = 0
    res: bool = False
    bias: bool = True
    K2: int = 0
    pool_w: int = 0

    @property
    def family(self) -> str:
        if self.kind == "256":
            return f"k_gemm_f16_256<{self.epi}>"
        if self.kind in ("f16", "glds"):
            return f"k_gemm_f16{'_glds' if self.kind == 'glds' else ''}<{self.epi}, {self.param}>"
        return f"{self.kind} route (EPI {self.epi})"

    @property
    def f32_out(self) -> bool:
        return self.epi in (2, 3)

    @property
    def out_rows(self) -> int:
        return self.M // 4 if self.epi in (5, 6) else self.M

    def __str__(self):
        extra = "".join([" relu" if self.relu else "", " res" if self.res else "", "" if self.bias else " nobias",
                         f" K2={self.K2}" if self.K2 else "", f" pool{self.pool_w}" if self.pool_w else ""])
        return f"{self.family} M={self.M} N={self.N} K={self.K}{extra}"


def _pad_rows(M: int) -> int:
    return -(-M // 256) * 256


def _f16_with_poison_rows(a: np.ndarray, M: int) -> np.ndarray:
    """fp16 rows 0 .. M - 1 of `a`, then NaN rows up to the next 256-row boundary"""
    out = np.empty((_pad_rows(M), a.shape[1]), np.float16)
    out[:M] = a[:M]
    out[M:].view(np.uint16)[:] = F16_POISON
    return np.ascontiguousarray(out)


def make_inputs(c: Case, regime: str, seed: int):
    rng = np.random.default_rng(seed)
    kt = c.K + c.K2
    if regime == "exact":
        # |partial sum| <= kt a^2 + 64 (bias) + 64 (residual) < 2**22 (fp32 outputs: + the 2**16 prefill) -- integers, exact in fp32;
        # fp16 outputs get smaller operands so that their typical values straddle fp16's exact-integer range (2048) without overflowing
        a = min(32, int(np.sqrt(2 ** 22 / kt))) if c.f32_out else min(16, max(2, int(np.sqrt(3e5 / kt))))
        gen = lambda shape, amp: rng.integers(-amp, amp + 1, shape).astype(np.float16)
        X, W = gen((c.M, c.K), a), gen((c.N, c.K), a)
        X2, W2 = (gen((c.M, c.K2), a), gen((c.N, c.K2), a)) if c.K2 else (None, None)
        bias = rng.integers(-64, 65, c.N).astype(np.float32) if c.bias else None
        res = gen((c.M, c.N), 64) if c.res else None
        c0 = rng.integers(-2 ** 16, 2 ** 16 + 1, (c.M, c.N)).astype(np.float32) if c.epi == 2 else None
    else:
        sc = np.float32(1.0 / np.sqrt(kt))
        X = rng.standard_normal((c.M, c.K), np.float32).astype(np.float16)
        W = (rng.standard_normal((c.N, c.K), np.float32) * sc).astype(np.float16)
        X2 = rng.standard_normal((c.M, c.K2), np.float32).astype(np.float16) if c.K2 else None
        W2 = (rng.standard_normal((c.N, c.K2), np.float32) * sc).astype(np.float16) if c.K2 else None
        bias = rng.standard_normal(c.N, np.float32) if c.bias else None
        res = rng.standard_normal((c.M, c.N), np.float32).astype(np.float16) if c.res else None
        c0 = (rng.standard_normal((c.M, c.N), np.float32) * 4) if c.epi == 2 else None
    return dict(X=X, W=W, X2=X2, W2=W2, bias=bias, res=res, c0=c0)


def reference(c: Case, inp, with_bound: bool = True):
    """(fp64 expected output before the store's rounding, worst-case bound of the random regime: accumulation, epilogue and store --
    or 0 without `with_bound`), both on the kernel's output grid"""
    X, W = inp["X"].astype(np.float64), inp["W"].astype(np.float64)
    acc = X @ W.T
    mag = np.abs(X) @ np.abs(W).T if with_bound else np.zeros_like(acc)
    if c.K2:
        X2, W2 = inp["X2"].astype(np.float64), inp["W2"].astype(np.float64)
        acc += X2 @ W2.T
        if with_bound:
            mag += np.abs(X2) @ np.abs(W2).T
    if inp["bias"] is not None:
        acc += inp["bias"].astype(np.float64)
        mag += np.abs(inp["bias"].astype(np.float64))
    if inp["res"] is not None and c.epi == 4:
        acc += inp["res"].astype(np.float64)
        mag += np.abs(inp["res"].astype(np.float64))
    # accumulation: K + K2 products summed in fp32 (the bias / residual adds included), any order, twice the textbook (K - 1) u
    accb = 2 * (c.K + c.K2 + 2) * U24 * mag
    relu = c.relu or c.epi in (5, 6)
    if c.epi == 1:
        out = acc / (1.0 + np.exp(-1.702 * acc))
        # QuickGELU is 1.1-Lipschitz; expf of an argument rounded to fp32 and the reciprocal / quotient: a few fp32 ulps
        b = 1.2 * accb + 4 * U24 * (np.abs(acc) * (1 + np.abs(acc)) + np.abs(out))
    else:
        out = np.maximum(acc, 0.0) if relu and c.epi in (3, 4, 5, 6) else acc
        b = accb
    if c.epi in (5, 6):
        # ReLU then the 2 x 2 average over (image row pair, column pair): pixel m = (crop * H + y) * W + x -> [(crop * H + y) / 2 * W / 2 + x / 2]
        w = c.pool_w
        pool = lambda a: a.reshape(c.M // (2 * w), 2, w // 2, 2, c.N).sum(axis=(1, 3)).reshape(c.M // 4, c.N) * 0.25
        out, b = pool(out), pool(b) + 3 * U24 * pool(np.abs(out))
    if c.epi == 2:
        out = inp["c0"].astype(np.float64) + out
        b = b + 2 * U24 * np.abs(out)
    if not c.f32_out:
        b = b + 2.0 ** -11 * (np.abs(out) + b) + 2.0 ** -25      # the fp16 store: half an fp16 ulp (and half a subnormal step)
    return out, b


def _ptr(a):
    return None if a is None else a.ctypes.data


def launch(lib: KatLib, c: Case, inp):
    """one launch; returns (status, the whole output allocation as raw bits [rows + guard][N])"""
    M, N = c.M, c.N
    rows = c.out_rows + (8 if c.pool_w else (_pad_rows(M) - M) + 8)
    if c.f32_out:
        C = np.full((rows, N), F32_POISON, np.uint32)
        if c.epi == 2:
            C[:M] = inp["c0"].view(np.uint32)
    else:
        C = np.full((rows, N), F16_POISON, np.uint16)
    X = _f16_with_poison_rows(inp["X"], M)
    W = np.ascontiguousarray(inp["W"])
    res = _f16_with_poison_rows(inp["res"], M) if inp["res"] is not None else None
    X2 = _f16_with_poison_rows(inp["X2"], M) if c.K2 else None
    W2 = np.ascontiguousarray(inp["W2"]) if c.K2 else None
    bias = inp["bias"]
    common = [_ptr(X), X.shape[0], _ptr(W), _ptr(bias), _ptr(C), C.nbytes, _ptr(res), 0 if res is None else res.shape[0], M, N, c.K, c.relu]
    ext = [_ptr(X2), 0 if X2 is None else X2.shape[0], _ptr(W2), c.K2, c.pool_w]
    L = lib.lib
    if c.kind == "f16":
        st = L.kat_gemm_f16(c.epi, c.param, *common)
    elif c.kind == "glds":
        st = L.kat_gemm_glds(c.epi, c.param, *common, *ext)
    elif c.kind == "256":
        st = L.kat_gemm_256(c.epi, *common)
    elif c.kind == "clip":
        st = L.kat_clip_gemm(c.epi, *common)
    elif c.kind == "wide":
        st = L.kat_wide_gemm(*common, *ext)
    else:
        raise ValueError(c.kind)
    return st, C


def run_case(lib: KatLib, c: Case, regime: str, seed: int = 0):
    """Runs `c` twice in `regime` and checks everything the module docstring lists.  Returns (max error, max of error / bound -- 0 / 0
    for the exact regime) or raises AssertionError naming the first violation."""
    inp = make_inputs(c, regime, seed)
    st, C = launch(lib, c, inp)
    assert st == 0, f"{c}: launch status {st}"
    st2, C2 = launch(lib, c, inp)
    assert st2 == 0, f"{c}: second launch status {st2}"
    assert np.array_equal(C, C2), f"{c} [{regime}]: two launches on the same inputs differ"
    R = c.out_rows
    poison = F32_POISON if c.f32_out else F16_POISON
    assert np.all(C[R:] == poison), f"{c} [{regime}]: rows >= {R} (guard band) written: first at row {R + int(np.argwhere(C[R:] != poison)[0][0])}"
    got = (C[:R].view(np.float32) if c.f32_out else C[:R].view(np.float16)).astype(np.float64)
    bad = np.isnan(got)
    assert not bad.any(), f"{c} [{regime}]: {int(bad.sum())} NaN outputs (unwritten or poison rows read), first at {tuple(np.argwhere(bad)[0])}"
    want, bnd = reference(c, inp, with_bound=regime != "exact")
    if regime == "exact":
        want = want if c.f32_out else want.astype(np.float16).astype(np.float64)
        wrong = got != want
        assert not wrong.any(), (f"{c} [exact]: {int(wrong.sum())} of {wrong.size} outputs differ from the exact result, first at "
                                 f"{tuple(np.argwhere(wrong)[0])}: got {got[tuple(np.argwhere(wrong)[0])]} want {want[tuple(np.argwhere(wrong)[0])]}")
        return 0.0, 0.0
    err = np.abs(got - want)
    over = err > bnd
    assert not over.any(), (f"{c} [random]: {int(over.sum())} outputs outside the bound, first at {tuple(np.argwhere(over)[0])}: "
                            f"err {err[tuple(np.argwhere(over)[0])]:.3e} > {bnd[tuple(np.argwhere(over)[0])]:.3e}")
    return float(err.max()), float((err / bnd).max())
