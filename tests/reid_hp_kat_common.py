"""Known-answer cases for the fp32-grade OSNet-x0.25 kernels (ReID mode 2, boxmot_amd/csrc/reid_hp.hpp and k_stem_resize_fused_hp of
reid_fused.hpp), every kernel launched ALONE through tests/kat/reid_hp_kat.hip: shared by the device test (test_gpu_reid_hp_kat.py) and
its CPU-thread emulation (test_reid_hp_kat_emu.py).  Not a product path.

Units (UNITS below): the crop kernel, the two stems, the stage-0 EMIT / RECON pair with its two fp32 hand-over tensors, the four other
OSBlock instantiations and the head.  Every reference is float64 torch on the float64 state dict, built from oracle/osnet.py's _conv_bn,
_bn and F.* (osblock64 restates oracle.osnet._osblock with its intermediate tensors exposed and one thing optionally WRONG; with nothing
wrong it returns _osblock's result bit for bit, which test_reid_hp_kat_emu.py asserts).

Inputs are built directly, not taken from the chain: an fp32 tensor v is split hi = fp16(v), lo = fp16(v - hi) in numpy, packed into the
lane-group-major layout from its definition (reid_hp.hpp:13-14: channel c = 16 ct + 4 g + r of a pixel sits at g (C / 4) + 4 ct + r),
and the reference consumes float64(hi) + float64(lo): input rounding is not an error source.  Three regimes per block unit and stem:
  dense     random non-negative activations with the magnitude the real chain has at that stage (one oracle forward of the same state
            dict: the rms of the stage's non-zero activations), a quarter of them zero
  impulses  zero except 2 x the chain's largest activation at placed pixels: the four corners, both sides of every seam between two
            waves' row strips (kat_hp_nwaves: H / NWAVES rows per wave), in stage 0 both sides of the x = 15 / 16 seam between the two
            16-pixel half rows; the channels cycle through the LAST channel of every 16-channel tile first
  blank     an all-zero crop: the bias-only response, every gate a constant

Metric and band: per crop and tensor max|got - ref64| / max|ref64|, evaluated per element against band * max|ref64| so that a failure
names unit, case, crop, (y, x), channel, got, want and error.  The bands (MEASURED, band()) are 4 x the largest value measured over every case of
the unit and weight kind, the margin tests/test_gpu_reid_precision.py uses; none may exceed BAND_CAP = 2e-5 (plain fp32 torch sits at
5.8e-7 on this metric; the (hi, lo) design promises fp32 grade).

A band that anything passes proves nothing, so every bounded case also evaluates deliberately WRONG references; each must leave the band
of the true reference somewhere in every case it applies to (the comment above block_wrong_references and _check_stem's docstring say which cases those are and why).

Around every launch: outputs prefilled with NaN poison and followed by a guard crop; owned elements come back finite, the guard (and the
head rows not named in out_rows) stays poison; each launch runs twice, identical bits; `count` as a null pointer, == n, == n - 1 and == 0
with the crops at or beyond count NaN on input (DEAD16, a payload other than the outputs' poison) and still poison on output (hand-over tensors included); crop i of an n = 3 launch
bit-identical to the same crop launched alone.
"""
from __future__ import annotations

import ctypes
import functools
import subprocess
from pathlib import Path

import numpy as np
import torch
import torch.nn.functional as F

from clip_kat_common import _caught, _first_rows, _owned, _twice
from gemm_kat_common import F16_POISON, F32_POISON

KAT_SRC = Path(__file__).resolve().parent / "kat" / "reid_hp_kat.hip"
BAND_CAP = 2e-5
FP16_OPERANDS_MIN_BANDS = 10            # the fp16-operand reference must miss by at least this many bands
MAX_ZERO_FRACTION = 0.65
WEIGHT_KINDS = ("init", "calib0", "calib1")
REGIMES = ("dense", "impulses", "blank")
STEM_ROWS, STEM_COLS = 262, 136         # one RGBX plane of a crop: 256 x 128 with a 3-pixel border
FRAME_W, FRAME_H = 641, 480
# tests/test_reid_emu.py's list: general, clipped at the frame's corner, empty, identity-sized (128 x 256), the whole frame, clipped at the
# far corner, two more general ones
BOXES = np.array([[30.2, 40.7, 90.1, 200.3], [-20, -10, 40, 60], [100, 100, 100, 150], [10, 10, 138, 266], [0, 0, 641, 480],
                  [600.4, 430.2, 700, 500], [50, 20, 200, 330], [300, 5, 420, 300]], dtype=np.float32)

# ---------------------------------------------------------------------------------------------------------------------------------
# Measured max|got - ref64| / max|ref64| per unit and weight kind (init = reference_init_state_dict, calib = random_osnet_state_dict
# seeds 0 and 1), largest over every case of the unit, and the band = 4 x measured.  "gpu": an MI355X, tests/test_gpu_reid_hp_kat.py;
# "emu": the CPU-thread emulation on its reduced case list, tests/test_reid_hp_kat_emu.py.  The table at the top of
# test_gpu_reid_hp_kat.py prints measured, band and ratio.
# ---------------------------------------------------------------------------------------------------------------------------------
MEASURED = {
    "gpu": {
        "stem": {"init": 6.037e-07, "calib": 5.090e-07},
        "stem_fused": {"init": 3.158e-07, "calib": 3.977e-07},
        "pair.x2s": {"init": 2.371e-07, "calib": 5.394e-07},
        "pair.x1s": {"init": 3.676e-07, "calib": 6.151e-07},
        "pair": {"init": 6.563e-07, "calib": 9.995e-07},
        "conv3.0": {"init": 3.353e-07, "calib": 5.463e-07},
        "conv3.1": {"init": 6.654e-07, "calib": 9.397e-07},
        "conv4.0": {"init": 3.713e-07, "calib": 7.041e-07},
        "conv4.1": {"init": 1.374e-07, "calib": 6.223e-07},
        "head": {"init": 1.752e-06, "calib": 1.589e-06},
    },
    "emu": {
        "stem": {"init": 9.488e-07, "calib": 9.557e-07},
        "stem_fused": {"init": 7.739e-07, "calib": 9.436e-07},
        "pair.x2s": {"init": 3.098e-07, "calib": 6.305e-07},
        "pair.x1s": {"init": 4.940e-07, "calib": 8.935e-07},
        "pair": {"init": 6.100e-07, "calib": 1.295e-06},
        "conv3.0": {"init": 6.501e-07, "calib": 9.712e-07},
        "conv3.1": {"init": 6.628e-07, "calib": 9.606e-07},
        "conv4.0": {"init": 6.665e-07, "calib": 1.048e-06},
        "conv4.1": {"init": 1.584e-07, "calib": 8.191e-07},
        "head": {"init": 1.768e-06, "calib": 9.120e-07},
    },
}


SEEN: dict = {}            # backend -> unit -> init | calib -> the largest metric this process has seen (noted BEFORE any assertion)


def note(backend: str, unit: str, kind: str, m: float):
    d = SEEN.setdefault(backend, {}).setdefault(unit, {})
    c = "init" if kind == "init" else "calib"
    d[c] = max(d.get(c, 0.0), m)


def band(backend: str, unit: str, kind: str) -> float:
    """4 x the measured figure of (unit, init | calib); never above BAND_CAP.  A unit without a measurement yet is held to the cap."""
    m = MEASURED[backend].get(unit, {}).get("init" if kind == "init" else "calib")
    b = BAND_CAP if m is None else 4 * m
    assert b <= BAND_CAP, f"{unit} [{kind}]: 4 x measured = {b:.2e} exceeds the cap {BAND_CAP:.0e}: a finding to explain, not a constant to raise"
    return b


# ---------------------------------------------------------------------------------------------------------------------------------
# build, ctypes
# ---------------------------------------------------------------------------------------------------------------------------------
def build_gpu(out_dir: Path, extra_flags=(), timeout: float = 900) -> Path:
    """hipcc for gfx950 with the product's flags (__graft_entry__.HIPCC_FLAGS) -> out_dir/libreid_hp_kat.so"""
    from __graft_entry__ import HIPCC_FLAGS

    out = Path(out_dir) / "libreid_hp_kat.so"
    subprocess.run(["hipcc", *HIPCC_FLAGS, *extra_flags, "-o", str(out), str(KAT_SRC)], check=True, timeout=timeout)
    return out


def build_emu(clang: str, out_dir: Path, extra_flags=(), timeout: float = 600) -> Path:
    """the same source on CPU threads (tests/host_emu/hip_shim.hpp), built as clip_kat_common.build_emu builds its harness"""
    out = Path(out_dir) / "libreid_hp_kat_emu.so"
    subprocess.run([clang, "-x", "c++", "-std=c++17", "-O1", "-fPIC", "-shared", "-pthread", "-ffp-contract=off", "-DKAT_EMU",
                    "-DEMU_DEFER_GLDS=1", *extra_flags, "-o", str(out), str(KAT_SRC)], check=True, timeout=timeout)
    return out


class ReidHpKatLib:
    """ctypes face of reid_hp_kat.hip's entry points"""

    def __init__(self, path, backend: str):
        self.backend = backend
        self.lib = L = ctypes.CDLL(str(path))
        P, I, G = ctypes.c_void_p, ctypes.c_int, ctypes.c_long
        L.kat_hp_crop.argtypes = [P, I, I, P, P, P, G, I, I]
        L.kat_hp_stem.argtypes = [P, G, P, P, G, P, P, G, I, I]
        L.kat_hp_stem_fused.argtypes = [P, G, P, I, I, P, P, P, G, I, I]
        L.kat_hp_stage0_pair.argtypes = [P, G, P, P, G, P, P, G, P, P, G, I, I]
        L.kat_hp_block.argtypes = [I, P, G, P, P, G, P, P, G, I, I]
        L.kat_hp_head.argtypes = [P, G, P, P, G, P, G, P, I, I]
        L.kat_hp_nwaves.argtypes = [I]
        for f in (L.kat_hp_crop, L.kat_hp_stem, L.kat_hp_stem_fused, L.kat_hp_stage0_pair, L.kat_hp_block, L.kat_hp_head, L.kat_hp_nwaves):
            f.restype = ctypes.c_int

    def nwaves(self, stage: int) -> int:
        return int(self.lib.kat_hp_nwaves(stage))


# ---------------------------------------------------------------------------------------------------------------------------------
# weights, chain magnitudes
# ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def weights(kind: str):
    """(float64 state dict, packed blob, {stage name: (rms of the non-zero activations, largest activation)} of one oracle forward)"""
    from boxmot_amd.reid_weights import pack_osnet, random_osnet_state_dict, reference_init_state_dict
    from oracle.crops import get_crops
    from oracle.osnet import osnet_forward

    sd = reference_init_state_dict("osnet_x0_25", 0) if kind == "init" else random_osnet_state_dict("osnet_x0_25", int(kind[-1]))
    sd = {k: v.detach() for k, v in sd.items() if torch.is_tensor(v)}
    blob = np.ascontiguousarray(pack_osnet(sd))
    _, st = osnet_forward({k: v.float() for k, v in sd.items()}, torch.from_numpy(get_crops(BOXES[:1], frame())), return_stages=True)
    mags = {}
    for name, t in st.items():
        a = t.numpy()
        mags[name] = (float(np.sqrt((a[a != 0] ** 2).mean())), float(a.max()))
    return {k: v.double() for k, v in sd.items()}, blob, mags


def fp16_operands(sd):
    """wrong reference (a): every convolution / linear weight rounded to fp16 (the arithmetic stays float64)"""
    return {k: (v.half().double() if k.endswith(".weight") and v.ndim in (2, 4) else v) for k, v in sd.items()}


@functools.lru_cache(maxsize=None)
def frame() -> np.ndarray:
    return np.random.default_rng(5).integers(0, 255, (FRAME_H, FRAME_W, 3), dtype=np.uint8)


# ---------------------------------------------------------------------------------------------------------------------------------
# the (hi, lo) lane-group-major layout, from its definition
# ---------------------------------------------------------------------------------------------------------------------------------
def l_position(C: int) -> np.ndarray:
    """position of channel c inside a pixel's C halves: c = 16 ct + 4 g + r -> g (C / 4) + 4 ct + r (the identity for C = 16)"""
    c = np.arange(C)
    return (c % 16) // 4 * (C // 4) + 4 * (c // 16) + c % 4


def split_hl(v: np.ndarray):
    """fp32 -> (hi, lo) fp16 and the float64 value hi + lo the kernels are handed"""
    assert v.dtype == np.float32
    hi = v.astype(np.float16)
    lo = (v - hi.astype(np.float32)).astype(np.float16)
    return hi, lo, hi.astype(np.float64) + lo.astype(np.float64)


def pack_hl(v: np.ndarray):
    """natural fp32 [n][P][C] -> (hi bits, lo bits) uint16 [n][P * C] in the L layout, and float64 hi + lo in natural order"""
    hi, lo, v64 = split_hl(v)
    pos = l_position(v.shape[-1])
    out = []
    for a in (hi, lo):
        L = np.empty_like(a)
        L[..., pos] = a
        out.append(np.ascontiguousarray(L.view(np.uint16).reshape(v.shape[0], -1)))
    return out[0], out[1], v64


def unpack_hl(h_bits: np.ndarray, l_bits: np.ndarray, C: int) -> np.ndarray:
    """raw uint16 [n][P * C] planes in the L layout -> float64 hi + lo, natural [n][P][C]"""
    pos = l_position(C)
    n = h_bits.shape[0]
    f = lambda b: np.ascontiguousarray(b).view(np.float16).reshape(n, -1, C)[..., pos].astype(np.float64)
    return f(h_bits) + f(l_bits)


def unpack_handover(bits: np.ndarray) -> np.ndarray:
    """the stage-0 hand-over tensors, raw uint32 [n][2048 * 16]: per crop [tile = 128][lane = 64][4] fp32 (reid_hp.hpp:356-359: wave w's
    tile i is tile w NT + i of the crop), lane = 16 g + l16 holds channels 4 g .. 4 g + 3 of pixel 16 tile + l16 -> natural [n][2048][16]"""
    n = bits.shape[0]
    a = np.ascontiguousarray(bits).view(np.float32).reshape(n, 128, 4, 16, 4)
    return a.transpose(0, 1, 3, 2, 4).reshape(n, 2048, 16).astype(np.float64)


# ---------------------------------------------------------------------------------------------------------------------------------
# float64 references
# ---------------------------------------------------------------------------------------------------------------------------------
def _nchw(x: np.ndarray, H: int, W: int) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(x)).reshape(x.shape[0], H, W, x.shape[-1]).permute(0, 3, 1, 2)


def _nat(t: torch.Tensor) -> np.ndarray:
    return t.permute(0, 2, 3, 1).reshape(t.shape[0], -1, t.shape[1]).numpy()


def light64(sd, p, x, replicate=False):
    """oracle.osnet._light; replicate: wrong reference (b), the depthwise 3x3 with replicate instead of zero padding"""
    from oracle.osnet import _bn
    c = x.shape[1]
    x = F.conv2d(x, sd[p + ".conv1.weight"])
    if replicate:
        x = F.conv2d(F.pad(x, (1, 1, 1, 1), mode="replicate"), sd[p + ".conv2.weight"], None, 1, 0, 1, c)
    else:
        x = F.conv2d(x, sd[p + ".conv2.weight"], None, 1, 1, 1, c)
    return F.relu(_bn(sd, p + ".bn", x))


def gate64(sd, p, x, one_short=False):
    """oracle.osnet._gate; one_short: wrong reference (c), the crop-wide sum misses one pixel (the last) and is still divided by H W -- what
    a reduction that drops a lane computes"""
    g = F.adaptive_avg_pool2d(x, 1)
    if one_short:
        g = g - x[:, :, -1:, -1:] / (x.shape[2] * x.shape[3])
    g = F.relu(F.conv2d(g, sd[p + ".fc1.weight"], sd[p + ".fc1.bias"]))
    g = torch.sigmoid(F.conv2d(g, sd[p + ".fc2.weight"], sd[p + ".fc2.bias"]))
    return x * g


def osblock64(sd, p, x, wrong=None):
    """oracle.osnet._osblock with its intermediates: (x2 = the gated branch sum, out).  wrong: None, "replicate" (b), "gate" (c),
    "shortcut" (d: the identity / downsample branch dropped)"""
    from oracle.osnet import BRANCH_DEPTHS, _conv_bn
    x1 = _conv_bn(sd, p + ".conv1", x, relu=True)
    x2 = None
    for name, depth in BRANCH_DEPTHS:
        t = x1
        for k in range(depth):
            t = light64(sd, f"{p}.{name}" if depth == 1 else f"{p}.{name}.{k}", t, wrong == "replicate")
        t = gate64(sd, p + ".gate", t, wrong == "gate")
        x2 = t if x2 is None else x2 + t
    x3 = _conv_bn(sd, p + ".conv3", x2, relu=False)
    identity = _conv_bn(sd, p + ".downsample", x, relu=False) if (p + ".downsample.conv.weight") in sd else x
    return x2, F.relu(x3 if wrong == "shortcut" else x3 + identity)


def transition64(sd, p, x, wrong=None):
    """conv 1x1 + BN + ReLU + 2 x 2 average pool (osnet.py:380-405); wrong "pool": (f), the pool taken before the ReLU"""
    from oracle.osnet import _conv_bn
    if wrong == "pool":
        return F.relu(F.avg_pool2d(_conv_bn(sd, p, x, relu=False), 2, 2))
    return F.avg_pool2d(_conv_bn(sd, p, x, relu=True), 2, 2)


class BlockUnit:
    """one block unit: which kernels, the geometry, the chain stage its dense inputs imitate, its reference"""

    def __init__(self, name, stage, cin, blocks, trans, blk, src):
        self.name, self.stage, self.cin, self.blocks, self.trans, self.blk, self.src = name, stage, cin, blocks, trans, blk, src
        self.H, self.W = 64 >> stage, 32 >> stage
        self.P = self.H * self.W
        self.cout = (64, 96, 128)[stage]
        self.out_px = self.P // 4 if trans else self.P
        self.out_W = self.W // 2 if trans else self.W
        self.identity = cin == self.cout            # the last block's shortcut is the input itself

    def tensors(self):
        """name -> (pixels, channels, image width) of every tensor the unit returns"""
        t = {"out": (self.out_px, self.cout, self.out_W)}
        if self.blk is None:
            t = {"x2s": (2048, 16, 32), "x1s": (2048, 16, 32), **t}
        return t

    def reference(self, sd, x64: np.ndarray, wrong=None) -> dict:
        """natural float64 [n][P][C] tensors.  The pair (reid_hp.hpp:337-359 and the EMIT epilogue :1188-1208): `link.x2s` receives x2[i][ct],
        conv2.0's gated branch sum BEFORE conv3; `x1s` receives relu(conv1 of conv2.1 applied to the in-register conv2.0 output), which
        RECON reads back as its conv1 result (X1_MEM) while it rebuilds conv2.0's output per tile from x2s for its identity shortcut."""
        from oracle.osnet import _conv_bn
        x = _nchw(x64, self.H, self.W)
        out = {}
        with torch.no_grad():
            for k, p in enumerate(self.blocks):
                last = k == len(self.blocks) - 1
                # (d) drops the shortcut of the LAST block run (for the pair's x1s: of conv2.0, see wrong_references)
                x2, y = osblock64(sd, p, x, wrong if (wrong != "shortcut" or last) else None)
                if self.blk is None and k == 0:
                    if wrong == "shortcut0":
                        x2, y = osblock64(sd, p, x, "shortcut")
                    out["x2s"] = _nat(x2)
                    out["x1s"] = _nat(_conv_bn(sd, self.blocks[1] + ".conv1", y, relu=True))
                x = y
            if self.trans:
                x = transition64(sd, self.trans, x, wrong)
        out["out"] = _nat(x)
        return out


UNITS = {
    "pair": BlockUnit("pair", 0, 16, ("conv2.0", "conv2.1"), "conv2.2.0", None, "maxpool"),
    "conv3.0": BlockUnit("conv3.0", 1, 64, ("conv3.0",), None, 2, "conv2.2"),
    "conv3.1": BlockUnit("conv3.1", 1, 96, ("conv3.1",), "conv3.2.0", 3, "conv3.0"),
    "conv4.0": BlockUnit("conv4.0", 2, 96, ("conv4.0",), None, 4, "conv3.2"),
    "conv4.1": BlockUnit("conv4.1", 2, 128, ("conv4.1",), None, 5, "conv4.0"),
}


def stem_reference(sd, x64: np.ndarray, wrong=None) -> np.ndarray:
    """x64: normalised crops float64 [n][256][128][3] -> conv 7x7 s2 p3 + BN + ReLU + max pool 3 s2 p1, natural [n][2048][16].
    wrong "pad0": (e), the pool's padding 0 instead of -inf; "shift": the pool window without its padding row / column (rows and columns
    2 o .. 2 o + 2 instead of 2 o - 1 .. 2 o + 1)"""
    from oracle.osnet import _conv_bn
    with torch.no_grad():
        y = _conv_bn(sd, "conv1", torch.from_numpy(np.ascontiguousarray(x64)).permute(0, 3, 1, 2), relu=True, stride=2, padding=3)
        if wrong == "pad0":
            y = F.max_pool2d(F.pad(y, (1, 1, 1, 1), value=0.0), 3, 2, 0)
        elif wrong == "shift":
            y = F.max_pool2d(F.pad(y, (0, 2, 0, 2), value=0.0), 3, 2, 0)
        else:
            y = F.max_pool2d(y, 3, 2, 1)
    return _nat(y)


def head_reference(sd, x64: np.ndarray) -> np.ndarray:
    """natural [n][128][128] -> conv5 + BN + ReLU -> mean over the 128 pixels -> FC + BatchNorm1d + ReLU -> L2 norm, [n][512]"""
    from oracle.osnet import BN_EPS, _conv_bn
    with torch.no_grad():
        y = _conv_bn(sd, "conv5", _nchw(x64, 16, 8), relu=True)
        v = F.linear(y.mean((2, 3)), sd["fc.0.weight"], sd["fc.0.bias"])
        v = F.relu(F.batch_norm(v, sd["fc.1.running_mean"], sd["fc.1.running_var"], sd["fc.1.weight"], sd["fc.1.bias"], False, 0.0, BN_EPS))
        return (v / v.norm(dim=1, keepdim=True)).numpy()


# ---------------------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------------------
def impulse_pixels(H: int, W: int, rows_per_wave: int, half_row_seam: bool):
    """(y, x) of the impulses: the corners, both sides of every wave-strip seam (at varying x, the image's left and right edge among
    them), both sides of the x = 15 / 16 half-row seam"""
    px = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)]
    xs = [0, W - 1, W // 2, 1, W - 2, W // 3, 2 * W // 3]
    for k, y in enumerate(range(rows_per_wave, H, rows_per_wave)):
        px += [(y - 1, xs[k % len(xs)]), (y, xs[(k + 3) % len(xs)])]
    if half_row_seam:
        px += [(1, 15), (1, 16), (H // 2, 15), (H // 2 + 1, 16), (H - 2, 16), (H - 2, 15)]
    return px


def block_inputs(u: BlockUnit, kind: str, regime: str, n: int, seed: int, nwaves: int) -> np.ndarray:
    """natural fp32 [n][P][cin]"""
    rms, top = weights(kind)[2][u.src]
    rng = np.random.default_rng(seed)
    v = np.zeros((n, u.P, u.cin), np.float32)
    if regime == "dense":
        v = (np.abs(rng.standard_normal(v.shape)) * rms * (rng.random(v.shape) >= 0.25)).astype(np.float32)
    elif regime == "impulses":
        tiles = u.cin // 16
        chans = [16 * t + 15 for t in range(tiles)] + [0, 5, 10]
        for i in range(n):
            for k, (y, x) in enumerate(impulse_pixels(u.H, u.W, u.H // nwaves, u.stage == 0)):
                v[i, y * u.W + x, chans[(k + i) % len(chans)] % u.cin] = 2 * top * (1 + 0.25 * i)
    elif regime != "blank":
        raise ValueError(regime)
    return v


# ---------------------------------------------------------------------------------------------------------------------------------
# checks
# ---------------------------------------------------------------------------------------------------------------------------------
def inside(label: str, got: np.ndarray, ref: np.ndarray, bnd_rel: float, width: int):
    """got, ref: natural float64 [n][P][C].  Every element within bnd_rel * max|ref of its crop|; a failure names crop, (y, x), channel,
    got, want and error.  Returns (the metric max over crops of max|got - ref| / max|ref|, the per-crop absolute bound broadcastable)."""
    scale = np.abs(ref).reshape(ref.shape[0], -1).max(1)
    assert (scale > 0).all(), f"{label}: a reference crop is identically zero: the metric is undefined"
    bnd = (bnd_rel * scale).reshape((-1,) + (1,) * (ref.ndim - 1))
    err = np.abs(got - ref)
    measured = float((err.reshape(ref.shape[0], -1).max(1) / scale).max())
    over = err > bnd
    if over.any():
        at = lambda i: (f"crop {i[0]}, (y, x) = {divmod(i[1], width)}, channel {i[2]}" if ref.ndim == 3 else f"crop {i[0]}, feature {i[1]}")
        i = tuple(int(k) for k in np.argwhere(over)[0])
        w = tuple(int(k) for k in np.unravel_index(np.argmax(err / bnd), err.shape))
        raise AssertionError(f"{label}: {int(over.sum())} of {over.size} outputs outside the band {bnd_rel:.2e}, first at {at(i)}: "
                             f"got {float(got[i])!r} want {float(ref[i])!r}, err {err[i]:.3e} > {float(np.broadcast_to(bnd, ref.shape)[i]):.3e}; "
                             f"worst ({measured:.2e} of the crop's largest value) at {at(w)}: got {float(got[w])!r} want {float(ref[w])!r}")
    return measured, np.broadcast_to(bnd, ref.shape)


def fp16_operand_distance(label: str, got, wrong, ref, bnd_rel: float):
    """(a) must miss by at least FP16_OPERANDS_MIN_BANDS bands on the metric itself"""
    scale = np.abs(ref).reshape(ref.shape[0], -1).max(1)
    d = float((np.abs(got - wrong).reshape(ref.shape[0], -1).max(1) / scale).max())
    assert d >= FP16_OPERANDS_MIN_BANDS * bnd_rel, (f"{label}: the fp16-operand reference is only {d:.2e} = {d / bnd_rel:.1f} bands away "
                                                    f"(needs {FP16_OPERANDS_MIN_BANDS}): the band does not tell fp32 grade from fp16 operands")
    return d


def relu_blind_spots(label: str, ref: np.ndarray, width: int):
    """ReLU zeros hide errors: at most 65 % of the reference may be exactly zero, and every 16-channel tile x image row and every tile x
    image column must hold a non-zero reference element (a property of the reference alone)"""
    n, P, C = ref.shape
    nz = (ref != 0).reshape(n, P // width, width, C // 16, 16)
    frac = 1 - nz.mean()
    assert frac <= MAX_ZERO_FRACTION, f"{label}: {frac:.1%} of the reference is exactly zero (limit {MAX_ZERO_FRACTION:.0%})"
    rows, cols = nz.any((2, 4)), nz.any((1, 4))
    assert rows.all(), f"{label}: channel tile x image row without a non-zero reference element at (crop, y, tile) {tuple(np.argwhere(~rows)[0])}"
    assert cols.all(), f"{label}: channel tile x image column without a non-zero reference element at (crop, x, tile) {tuple(np.argwhere(~cols)[0])}"
    return float(frac)


DEAD16 = np.uint16(0x7F11)      # the NaN of a dead input crop: NOT the outputs' poison pattern, which a NaN that keeps its payload through
                                # the arithmetic (x86 does, in the emulation) would otherwise reproduce in the output unnoticed


def _dead(arrays, k: int):
    """the crop-major input arrays with crops k .. poisoned (fp16 planes: a NaN in both parts; boxes: NaN)"""
    out = []
    for a in arrays:
        a = a.copy()
        a[k:] = DEAD16 if a.dtype == np.uint16 else np.nan
        out.append(a)
    return out


def _poison_crops(n: int, elems: int, f32: bool) -> np.ndarray:
    return np.full((n + 1, elems), F32_POISON if f32 else F16_POISON, np.uint32 if f32 else np.uint16)       # + one guard crop


def protocol(label: str, launch, inputs, n: int, full: bool, finite: bool = True) -> dict:
    """launch(inputs, n, count) -> (status, {name: raw bits [n + 1 guard][elems]}).  Runs the checks around a launch (module docstring) and
    returns the raw outputs of the count-less launch."""
    def flat(count, arrays=inputs, m=n):
        st, d = launch(arrays, m, count)
        names = sorted(d)
        return st, np.concatenate([d[k].view(np.uint8).reshape(d[k].shape[0], -1) for k in names], 1), d

    keep = {}

    def once():
        st, bits, d = flat(-1)
        keep.update(d)
        return st, bits
    base = _twice(label, once)
    for name, C in keep.items():
        if finite:
            _owned(f"{label} {name}", C, _first_rows(n + 1, n))
        else:           # the caller checks the owned crops itself (the crop kernel leaves the border alone)
            assert (C[n:] == (F32_POISON if C.dtype == np.uint32 else F16_POISON)).all(), f"{label} {name}: the guard crop was written"
    if not full:
        return keep

    def poison_from(k, d, what):
        for name, C in d.items():
            pz = F32_POISON if C.dtype == np.uint32 else F16_POISON
            assert (C[k:] == pz).all(), f"{label} {what}: {name} of a crop at or beyond count was written (first crop {k + int(np.argwhere(C[k:] != pz)[0][0])})"
    st, bits, _ = flat(n)
    assert st == 0 and np.array_equal(bits, base), f"{label}: count == n differs from a null count"
    if n > 1:
        st, bits, d = flat(n - 1, _dead(inputs, n - 1))
        assert st == 0 and np.array_equal(bits[:n - 1], base[:n - 1]), f"{label} count == n - 1: the live crops differ from the count-less launch (or read a dead crop)"
        poison_from(n - 1, d, "count == n - 1")
        for i in range(n):
            st, bits, _ = flat(-1, [a[i:i + 1] for a in inputs], 1)
            assert st == 0 and np.array_equal(bits[0], base[i]), f"{label}: crop {i} launched alone differs from crop {i} of the n = {n} launch"
    st, _, d = flat(0, _dead(inputs, 0))
    assert st == 0, f"{label} count == 0: status {st}"
    poison_from(0, d, "count == 0")
    return keep


# ---------------------------------------------------------------------------------------------------------------------------------
# block units
# ---------------------------------------------------------------------------------------------------------------------------------
# Which wrong reference applies where (every one listed must leave the band in EVERY case):
#   (a) fp16 operands      every tensor of every case -- also blank: the input is exactly zero there, the weights are not
#   (b) replicate padding  every tensor of every case (blank: conv1's bias response is a non-zero constant image whose zero-padded
#                          depthwise result differs from the replicated one along the whole border)
#   (c) gate one short     the sum loses the last pixel's value, divisor unchanged.  The gate's MLP has MID / 16 = 1 or 2 hidden units
#                          behind a ReLU: where they are dead the gate is a constant and NO test can see its mean.  Whether they are is
#                          a property of the float64 reference alone, so (c) applies to a tensor of a case when it moves the float64
#                          reference by more than GATE_APPLIES_BANDS bands, and run_block returns where it applied: the tests assert
#                          that it did in at least one case of every unit and weight kind
#   (d) shortcut dropped   "out" of every case, except blank on a block with an IDENTITY shortcut (conv4.1: the identity is the all-zero
#                          input, so dropping it changes nothing); the pair's x1s with conv2.0's downsample dropped; never x2s, the
#                          pre-shortcut sum
#   (f) pool before ReLU   "out" of the units with a fused transition
GATE_APPLIES_BANDS = 2.5


def block_wrong_references(u: BlockUnit, sd, x64, regime: str) -> dict:
    """tensor name -> {wrong reference name: tensor}"""
    w = {k: {} for k in u.tensors()}
    def add(name, ref, only=None):
        for k, t in ref.items():
            if only is None or k in only:
                w[k][name] = t
    add("(b) depthwise 3x3 with replicate padding", u.reference(sd, x64, "replicate"))
    add("(c) gate mean one pixel short", u.reference(sd, x64, "gate"))
    if not (regime == "blank" and u.identity):
        add("(d) shortcut dropped", u.reference(sd, x64, "shortcut"), ("out",))
    if u.blk is None:
        add("(d) conv2.0's downsample dropped", u.reference(sd, x64, "shortcut0"), ("x1s",))
    if u.trans:
        add("(f) transition pool before the ReLU", u.reference(sd, x64, "pool"), ("out",))
    return w


def block_launch(lib: ReidHpKatLib, u: BlockUnit, blob: np.ndarray):
    def launch(arrays, n, count):
        ih, il = (np.ascontiguousarray(a) for a in arrays)
        oh, ol = _poison_crops(n, u.out_px * u.cout, False), _poison_crops(n, u.out_px * u.cout, False)
        if u.blk is None:
            x1, x2 = _poison_crops(n, 2048 * 16, True), _poison_crops(n, 2048 * 16, True)
            st = lib.lib.kat_hp_stage0_pair(blob.ctypes.data, blob.size, ih.ctypes.data, il.ctypes.data, ih.size, x1.ctypes.data, x2.ctypes.data,
                                            x1.size, oh.ctypes.data, ol.ctypes.data, oh.size, n, count)
            return st, {"x1s": x1, "x2s": x2, "out_h": oh, "out_l": ol}
        st = lib.lib.kat_hp_block(u.blk, blob.ctypes.data, blob.size, ih.ctypes.data, il.ctypes.data, ih.size, oh.ctypes.data, ol.ctypes.data,
                                  oh.size, n, count)
        return st, {"out_h": oh, "out_l": ol}
    return launch


def run_block(lib: ReidHpKatLib, unit: str, kind: str, regime: str, n: int, seed: int = 0, full: bool = True) -> dict:
    """one case of a block unit; returns {tensor: measured metric}"""
    u = UNITS[unit]
    label = f"{unit} [{kind}, {regime}, n={n}]"
    sd, blob, _ = weights(kind)
    ih, il, x64 = pack_hl(block_inputs(u, kind, regime, n, seed, lib.nwaves(u.stage)))
    raw = protocol(label, block_launch(lib, u, blob), [ih, il], n, full)
    got = {"out": unpack_hl(raw["out_h"][:n], raw["out_l"][:n], u.cout)}
    if u.blk is None:
        got["x1s"], got["x2s"] = unpack_handover(raw["x1s"][:n]), unpack_handover(raw["x2s"][:n])
    ref = u.reference(sd, x64)
    if not any(r.any() for r in ref.values()):
        # reference_init_state_dict has no bias anywhere a zero input could reach (BatchNorm bias 0, running mean 0): the bias-only
        # response IS zero, the metric has no scale, and the known answer is exact -- every output a (hi, lo) or fp32 zero
        assert regime == "blank" and kind == "init", f"{label}: the reference is identically zero"
        for name, g in got.items():
            assert not g.any(), f"{label} {name}: {int((g != 0).sum())} outputs differ from the exact zero response, first at {tuple(np.argwhere(g != 0)[0])}"
        print(f"{label}: the reference is identically zero and so is every output")
        return {}
    zero = relu_blind_spots(f"{label} out", ref["out"], u.out_W)
    wrong = block_wrong_references(u, sd, x64, regime)
    half = u.reference(fp16_operands(sd), x64.astype(np.float16).astype(np.float64))
    measured = {}
    for name, (_, _, width) in u.tensors().items():
        key = unit if name == "out" else f"{unit}.{name}"
        b = band(lib.backend, key, kind)
        m = float((np.abs(got[name] - ref[name]).reshape(n, -1).max(1) / np.abs(ref[name]).reshape(n, -1).max(1)).max())
        print(f"{label} {name}: measured {m:.3e}, band {b:.3e}, ratio {m / b:.3f}" + (f", reference zeros {zero:.1%}" if name == "out" else ""))
        measured[key] = m
        note(lib.backend, key, kind, m)
    for name, (_, _, width) in u.tensors().items():
        key = unit if name == "out" else f"{unit}.{name}"
        b = band(lib.backend, key, kind)
        _, bnd = inside(f"{label} {name}", got[name], ref[name], b, width)
        fp16_operand_distance(f"{label} {name}", got[name], half[name], ref[name], b)
        ctl = {"(a) fp16 operands": half[name], **wrong[name]}
        gate = "(c) gate mean one pixel short"
        if not (np.abs(ctl[gate] - ref[name]) > GATE_APPLIES_BANDS * bnd).any():
            del ctl[gate]
        elif name == "out":
            measured["gate control applied"] = 1.0
        _caught(f"{label} {name}", got[name], bnd, ctl)
    return measured


# ---------------------------------------------------------------------------------------------------------------------------------
# crop kernel and stems
# ---------------------------------------------------------------------------------------------------------------------------------
def _frame_launch(lib: ReidHpKatLib, fn, blob, elems: int):
    fr = frame()

    def launch(arrays, n, count):
        boxes = np.ascontiguousarray(arrays[0], np.float32)
        oh, ol = _poison_crops(n, elems, False), _poison_crops(n, elems, False)
        head = (blob.ctypes.data, blob.size) if blob is not None else ()
        st = fn(*head, fr.ctypes.data, FRAME_W, FRAME_H, boxes.ctypes.data, oh.ctypes.data, ol.ctypes.data, oh.size, n, count)
        return st, {"out_h": oh, "out_l": ol}
    return launch


def run_crop(lib: ReidHpKatLib, boxes: np.ndarray, full: bool = True):
    """k_crop_resize_rgbx_hl against oracle.crops.get_crops.  The kernel stores hi = fp16(f), lo = fp16(f - hi) of the fp32 table value f:
    |f - hi| <= 2**-11 |f|, f - hi is exact in fp32, and its fp16 rounding errs by at most 2**-11 |f - hi| <= 2**-22 |f| while lo is a
    NORMAL fp16 number; when |f - hi| < 2**-14 lo is subnormal (spacing 2**-24) and the error is at most 2**-25 absolute.  So
    |hi + lo - f| <= max(2**-22 |f|, 2**-25).  The kernel writes the 256 x 128 interior only: the 3-pixel border must come back as it
    went in (poison here, the engine's one-time zero fill in the product) and the X channel must be written as zero in both planes.
    Returns (largest |err| / |f|, number of elements beyond the purely relative 2**-22 |f|)."""
    from oracle.crops import get_crops
    n = len(boxes)
    label = f"k_crop_resize_rgbx_hl n={n}"
    raw = protocol(label, _frame_launch(lib, lib.lib.kat_hp_crop, None, STEM_ROWS * STEM_COLS * 4), [boxes], n, full, finite=False)
    planes = [raw[k][:n].reshape(n, STEM_ROWS, STEM_COLS, 4) for k in ("out_h", "out_l")]
    border = np.ones((STEM_ROWS, STEM_COLS), bool)
    border[3:259, 3:131] = False
    for k, p in zip(("hi", "lo"), planes):
        assert (p[:, border] == F16_POISON).all(), f"{label}: the {k} plane's 3-pixel border was written"
        assert (p[:, 3:259, 3:131, 3] == 0).all(), f"{label}: the {k} plane's X channel is not zero"
    got = sum(p[:, 3:259, 3:131, :3].view(np.float16).astype(np.float64) for p in planes)
    assert np.isfinite(got).all(), f"{label}: {int((~np.isfinite(got)).sum())} interior elements not finite (unwritten)"
    want = get_crops(boxes, frame()).transpose(0, 2, 3, 1).astype(np.float64)
    err = np.abs(got - want)
    bnd = np.maximum(2.0 ** -22 * np.abs(want), 2.0 ** -25)
    over = err > bnd
    if over.any():
        i = tuple(int(k) for k in np.argwhere(over)[0])
        raise AssertionError(f"{label}: {int(over.sum())} elements off get_crops, first at crop {i[0]}, (y, x) = ({i[1]}, {i[2]}), channel {i[3]}: "
                             f"got {got[i]!r} want {want[i]!r}, err {err[i]:.3e} > {bnd[i]:.3e}")
    return float((err / np.abs(want)).max()), int((err > 2.0 ** -22 * np.abs(want)).sum()), planes


def stem_planes(regime: str, n: int, seed: int) -> np.ndarray:
    """normalised crops fp32 [n][256][128][3] built directly: dense = the table values of random pixels; impulses = zero except the table's
    largest value at the corners and at both sides of the seams between the eight waves' strips (pooled rows 8 w .. 8 w + 7 = input rows
    32 w ..), left and right edge included; blank = zero"""
    from oracle.crops import normalization_lut
    lut = normalization_lut()
    rng = np.random.default_rng(seed)
    v = np.zeros((n, 256, 128, 3), np.float32)
    if regime == "dense":
        px = rng.integers(0, 256, v.shape)
        for c in range(3):
            v[..., c] = lut[c][px[..., c]]
    elif regime == "impulses":
        for i in range(n):
            for k, (y, x) in enumerate(impulse_pixels(256, 128, 32, False)):
                v[i, y, x, (k + i) % 3] = lut[(k + i) % 3][255] * (1 - 0.125 * i)
    elif regime != "blank":
        raise ValueError(regime)
    return v


def planes_to_bits(v: np.ndarray):
    """[n][256][128][3] fp32 -> (hi, lo) RGBX planes with the zero border as raw bits [n][262 * 136 * 4], and float64 hi + lo"""
    hi, lo, v64 = split_hl(v)
    out = []
    for a in (hi, lo):
        p = np.zeros((v.shape[0], STEM_ROWS, STEM_COLS, 4), np.float16)
        p[:, 3:259, 3:131, :3] = a
        out.append(np.ascontiguousarray(p.view(np.uint16).reshape(v.shape[0], -1)))
    return out[0], out[1], v64


def _check_stem(lib, label, unit, kind, got, sd, x64, wrong_applies: bool):
    """Stem checks.  Wrong references: (a) fp16 operands and the shifted pool window in every dense / impulses / frame case; not in blank
    (a zero input makes the output relu(bias) everywhere: neither the weights nor the window matter).  (e) as first stated -- the
    pool's padding 0 instead of -inf -- is IDENTICAL to the reference on post-ReLU values (max(0, a) = a for a >= 0; k_stem_hp relies on
    exactly that, reid_hp.hpp:1477), so no band can catch it: asserted equal here, and the shifted window stands in for it."""
    b = band(lib.backend, unit, kind)
    ref = stem_reference(sd, x64)
    n = ref.shape[0]
    if not ref.any():           # blank crop on the reference's own initialisation: BatchNorm bias 0, the response is exactly zero
        assert not got.any(), f"{label}: {int((got != 0).sum())} outputs differ from the exact zero response"
        return 0.0
    m = float((np.abs(got - ref).reshape(n, -1).max(1) / np.abs(ref).reshape(n, -1).max(1)).max())
    print(f"{label}: measured {m:.3e}, band {b:.3e}, ratio {m / b:.3f}")
    note(lib.backend, unit, kind, m)
    _, bnd = inside(label, got, ref, b, 32)
    assert np.array_equal(stem_reference(sd, x64, "pad0"), ref), "(e) pool padding 0 must equal the reference on post-ReLU values"
    if wrong_applies:
        half = stem_reference(fp16_operands(sd), x64.astype(np.float16).astype(np.float64))
        fp16_operand_distance(label, got, half, ref, b)
        _caught(label, got, bnd, {"(a) fp16 operands": half, "(e') pool window without its padding row and column": stem_reference(sd, x64, "shift")})
    return m


def run_stem(lib: ReidHpKatLib, kind: str, regime: str, n: int, seed: int = 0, full: bool = True):
    """k_stem_hp on planes built directly"""
    label = f"k_stem_hp [{kind}, {regime}, n={n}]"
    sd, blob, _ = weights(kind)
    ih, il, x64 = planes_to_bits(stem_planes(regime, n, seed))

    def launch(arrays, m, count):
        a, c = (np.ascontiguousarray(t) for t in arrays)
        oh, ol = _poison_crops(m, 2048 * 16, False), _poison_crops(m, 2048 * 16, False)
        st = lib.lib.kat_hp_stem(blob.ctypes.data, blob.size, a.ctypes.data, c.ctypes.data, a.size, oh.ctypes.data, ol.ctypes.data, oh.size, m, count)
        return st, {"out_h": oh, "out_l": ol}
    raw = protocol(label, launch, [ih, il], n, full)
    got = unpack_hl(raw["out_h"][:n], raw["out_l"][:n], 16)
    return {"stem": _check_stem(lib, label, "stem", kind, got, sd, x64, regime != "blank")}


def run_stem_fused(lib: ReidHpKatLib, kind: str, boxes: np.ndarray, full: bool = True, against_planes=None):
    """k_stem_resize_fused_hp on frame + boxes; the reference normalises the resized uint8 crop in float64 ((v / 255 - mean) / std with the
    fp32 constants of base_backend.py) and runs the stem on that.  against_planes: the crop kernel's (hi, lo) planes of the same boxes --
    k_stem_hp runs on them and the two stems' outputs must agree within the sum of their bands."""
    from oracle.crops import MEAN_RGB, STD_RGB, get_crops_u8
    n = len(boxes)
    label = f"k_stem_resize_fused_hp [{kind}, n={n}]"
    sd, blob, _ = weights(kind)
    raw = protocol(label, _frame_launch(lib, lib.lib.kat_hp_stem_fused, blob, 2048 * 16), [boxes], n, full)
    got = unpack_hl(raw["out_h"][:n], raw["out_l"][:n], 16)
    x64 = (get_crops_u8(boxes, frame()).astype(np.float64) / 255.0 - MEAN_RGB.astype(np.float64)) / STD_RGB.astype(np.float64)
    res = {"stem_fused": _check_stem(lib, label, "stem_fused", kind, got, sd, x64, True)}
    if against_planes is not None:
        ph, pl = (np.ascontiguousarray(p.reshape(n, -1)) for p in against_planes)
        for p in (ph, pl):          # the product zero-fills the border once; the crop test left poison there
            p.reshape(n, STEM_ROWS, STEM_COLS, 4)[:, np.r_[0:3, 259:262]] = 0
            p.reshape(n, STEM_ROWS, STEM_COLS, 4)[:, :, np.r_[0:3, 131:136]] = 0
        oh, ol = _poison_crops(n, 2048 * 16, False), _poison_crops(n, 2048 * 16, False)
        assert lib.lib.kat_hp_stem(blob.ctypes.data, blob.size, ph.ctypes.data, pl.ctypes.data, ph.size, oh.ctypes.data, ol.ctypes.data, oh.size, n, -1) == 0
        sep = unpack_hl(oh[:n], ol[:n], 16)
        res["stem"] = _check_stem(lib, f"k_stem_hp after the crop kernel [{kind}, n={n}]", "stem", kind, sep, sd,
                                  sum(p.reshape(n, STEM_ROWS, STEM_COLS, 4)[:, 3:259, 3:131, :3].view(np.float16).astype(np.float64) for p in (ph, pl)), True)
        inside(f"{label} against k_stem_hp", got, sep, band(lib.backend, "stem", kind) + band(lib.backend, "stem_fused", kind), 32)
    return res


# ---------------------------------------------------------------------------------------------------------------------------------
# head
# ---------------------------------------------------------------------------------------------------------------------------------
def run_head(lib: ReidHpKatLib, kind: str, n: int, seed: int = 0, full: bool = True):
    """k_head_hp<128, 512>: dense stage-2 activations (crop 0 of n > 1 sparser: three quarters zero), an out_rows permutation scattered over
    2 n + 3 rows + guard, and a device-side count (null, n, n - 1, 0).  Wrong references: (a) fp16 operands; (g) out_rows ignored (crop i's
    embedding expected in row i)."""
    label = f"k_head_hp [{kind}, n={n}]"
    sd, blob, mags = weights(kind)
    rng = np.random.default_rng(seed)
    v = (np.abs(rng.standard_normal((n, 128, 128))) * mags["conv4.1"][0] * (rng.random((n, 128, 128)) >= 0.25)).astype(np.float32)
    if n > 1:
        v[0] *= rng.random((128, 128)) >= 0.66
    ih, il, x64 = pack_hl(v)
    total = 2 * n + 3 + 8
    rows = rng.permutation(2 * n + 3)[:n].astype(np.int32)
    if (rows == np.arange(n)).all():
        rows = np.ascontiguousarray(rows[::-1] + 1)
    b = band(lib.backend, "head", kind)

    def launch(count, live, a=ih, c=il, r=rows):
        C = np.full((total, 512), F32_POISON, np.uint32)
        a, c = _dead([a, c], live)
        st = lib.lib.kat_hp_head(blob.ctypes.data, blob.size, a.ctypes.data, c.ctypes.data, a.size, C.ctypes.data, total,
                                 r.ctypes.data if r is not None else None, len(a), count)
        return st, C

    def owned(k):
        m = np.zeros(total, bool)
        m[rows[:k]] = True
        return m
    C = _twice(label, lambda: launch(-1, n))
    _owned(label, C, owned(n))
    got = C[rows].view(np.float32).astype(np.float64)
    ref = head_reference(sd, x64)
    m = float((np.abs(got - ref).max(1) / np.abs(ref).max(1)).max())
    print(f"{label}: measured {m:.3e}, band {b:.3e}, ratio {m / b:.3f}")
    note(lib.backend, "head", kind, m)
    _, bnd = inside(label, got, ref, b, 1)
    half = head_reference(fp16_operands(sd), x64.astype(np.float16).astype(np.float64))
    fp16_operand_distance(label, got, half, ref, b)
    by_row = C.view(np.float32).astype(np.float64)            # (g): row i is expected to hold crop i
    assert (~(np.abs(by_row[:n] - ref) <= bnd)).any(), f"{label}: the wrong reference '(g) out_rows ignored' stays inside the band"
    _caught(label, got, bnd, {"(a) fp16 operands": half})
    if full:
        st, C2 = launch(n, n)
        assert st == 0 and np.array_equal(C2, C), f"{label}: count == n differs from a null count"
        for cnt in sorted({n - 1, 0}):
            st, C2 = launch(cnt, cnt)
            assert st == 0, f"{label} count == {cnt}: status {st}"
            _owned(f"{label} count == {cnt}", C2, owned(cnt))          # rows of crops at or beyond count still poison, the others finite
            assert np.array_equal(C2[rows[:cnt]], C[rows[:cnt]]), f"{label} count == {cnt}: live crops differ from the count-less launch"
        for i in sorted({0, n - 1, min(n - 1, 15), min(n - 1, 16)}):
            st, C1 = launch(-1, 1, ih[i:i + 1], il[i:i + 1], None)
            assert st == 0 and np.array_equal(C1[0], C[rows[i]]), f"{label}: crop {i} launched alone differs from crop {i} of the n = {n} launch"
    return {"head": m}


def report(backend: str):
    """the figures this process has seen, beside the table's"""
    for unit, d in sorted(SEEN.get(backend, {}).items()):
        for c, m in sorted(d.items()):
            have = MEASURED[backend].get(unit, {}).get(c)
            print(f"MEASURED {backend} {unit:12s} {c:5s} {m:.3e}" + (f"   table {have:.3e}, band {4 * have:.3e}, ratio {m / (4 * have):.3f}" if have else ""))
