"""Times of the detection post-processing kernels beside the host path they replace: A = 8400 anchors, 80 classes, fp16, "cn", for
1 / 16 / 64 streams at two pass rates (about 1 % of the anchors over the threshold -- a quiet scene -- and about 30 %, more than
max_candidates = 1024, so the exact top-K works).  The measuring program is tools/detpost_prof.hip: HIP events around each kernel of
the library's own sequence, 5 warm-up and 30 timed calls, and the device-to-host copy of the same tensor.  This script makes the
tensor (tests/detpost_ref.py random_pred, one stream, copied to every stream), runs the program, checks its checksum against the NumPy
reference's rows, and times that reference on this host: the host path is the copy plus S times the reference of one stream.

    python tools/detpost_prof.py [--streams 1 16 64] [--rates 0.01 0.3] [--repeats 30] [--out DIR]

``--obb`` times the ORIENTED layout instead (csrc/det_post_obb.hpp): A = 21 504 anchors (a 1024 x 1024 input), 15 classes, fp16, 64
streams, a sparse and a busy scene; per scene the axis-aligned path on the same boxes (the tensor without its angle row) and the
oriented path in both NMS modes, from the same run.  The checksums are compared with tests/detpost_obb_ref.py; where a scene has a
pair within the reference's margin of the threshold the NMS decisions may differ, which is reported and not an error.

``--extra`` times a POSE head instead (csrc/det_post_extra.hpp): A = 8400 anchors, 1 class, E = 51 values per anchor ("kpt3": 17
keypoints), fp16, "cn", 64 streams, a quiet and a busy scene; the three-kernel sequence -- score, the select kernel's source-storing
variant, k_detpost_extra -- with the third kernel's useful bytes per second (what it has to read and write: per emitted value one
element of the tensor and one float32, per row one source index), beside the host path it replaces, the copy of the tensor plus
tests/detpost_extra_ref.py on this host.  The checksum covers the rows, the extras and the source anchors.

``--mask`` times a SEGMENTATION head with the masks decoded on the device (csrc/det_post_mask.hpp): A = 8400 anchors, 80 classes, E =
32 coefficients, fp16, "cn", 64 streams, prototypes 32 x 160 x 160 fp16 of a 640 x 640 input, a quiet and a busy scene; the
four-kernel sequence with k_detpost_mask between its own events, beside a hipMemsetAsync of exactly the emitted mask bytes timed in
the same calls (the floor of a kernel that must write them), k_detpost_mask's useful bytes per second (the mask bytes stored plus
the prototype bytes inside the windows), and the host path it replaces: the copy of the prototypes plus tests/detpost_mask_ref.py
on this host.  The checksum covers the rows, the extras, the source anchors and stream 0's masks.

``--labels`` times the frame-space LABEL MAP (csrc/det_post_labels.hpp) through the public call, ``DetPost.labels``, between HIP events
(torch.cuda.Event), medians of ``--repeats`` calls in alternating blocks of five with the path it replaces, timed in the same run: the
torch-on-device sequence a caller writes today per stream -- ``coef @ proto``, the letterbox padding cut off, ``F.interpolate`` to
the frame, crop to the row's box, ``> 0``, first-wins.  16 and 64 streams of 1080p, prototypes 32 x 160 x 160 fp16 of a 640 x 640
input, a sparse scene (boxes covering about 0.3 x the frame area) and a busy one (about 2 x).  Then the measuring program runs the
kernel alone on the LDS patch and with the fallback forced, alternating, and its checksum is compared with the public call's labels
(and, on the sparse scene, with tests/detpost_labels_ref.py).  Reports; no threshold.

Needs a gfx950 device.  profiles/detpost_timing.txt, profiles/detpost_obb_timing.txt, profiles/detpost_extra_timing.txt,
profiles/detpost_mask_timing.txt and profiles/detpost_labels_timing.txt hold the outputs of such runs."""
import argparse
import os
import subprocess
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
SRC = ROOT / "tools" / "detpost_prof.hip"
EXE = ROOT / "tools" / "_build" / "detpost_prof"
CSRC = ROOT / "boxmot_amd" / "csrc"
DEPS = [SRC, CSRC / "det_post.hpp", CSRC / "det_post_obb.hpp", CSRC / "det_post_extra.hpp", CSRC / "det_post_select_body.hpp", CSRC / "kernel_macros.hpp",
        CSRC / "det_post_mask.hpp", CSRC / "det_post_labels.hpp", CSRC / "det_post_tiled.hpp", CSRC / "det_post_tiled_select_body.hpp"]
sys.path[:0] = [str(ROOT / "tests"), str(ROOT)]          # the reference lives with the tests


def build() -> Path:
    if not EXE.exists() or any(d.stat().st_mtime > EXE.stat().st_mtime for d in DEPS):
        EXE.parent.mkdir(parents=True, exist_ok=True)
        subprocess.check_call([os.environ.get("HIPCC", "hipcc"), "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-o", str(EXE), str(SRC)])
    return EXE


def obb_scene(A, nc, rate, seed, n_obj=150, size=1024):
    """One stream's (4 + nc + 1, A) fp16 tensor: clustered oriented boxes (sides 8..160 px, aspect <= 8) around n_obj objects, confs
    quantised to 1 / 128, an anchor 'active' with probability ``rate``"""
    rng = np.random.default_rng(seed)
    short = rng.integers(8, 41, n_obj)
    long_ = np.minimum(160, short * rng.integers(1, 9, n_obj))
    flip = rng.random(n_obj) < 0.5
    obj = np.stack([rng.integers(60, size - 60, n_obj), rng.integers(60, size - 60, n_obj), np.where(flip, short, long_), np.where(flip, long_, short)], 1)
    obj_ang = rng.integers(-50, 51, n_obj) / 32.0
    which = rng.integers(0, n_obj, A)
    box = (obj[which] + rng.integers(-24, 25, (A, 4)) / 4.0).astype(np.float32)
    ang = (obj_ang[which] + rng.integers(-8, 9, A) / 128.0).astype(np.float32)
    cf = rng.integers(128 // 3, 129, A).astype(np.float32) / np.float32(128)
    cf = np.where(rng.random(A) < rate, cf, cf * np.float32(0.125)).astype(np.float32)
    cls = (which + (rng.random(A) < 0.2)) % nc
    sc = cf[:, None] * (rng.integers(0, 5, (A, nc)).astype(np.float32) / np.float32(8))
    sc[np.arange(A), cls] = cf
    return np.concatenate([box.T, sc.T, ang[None]], 0).astype(np.float16)


def run_exe(exe, args, want, lenient=False):
    """the measuring program's output, printed; 0, or the exit status to stop with"""
    r = subprocess.run([str(exe), *[str(v) for v in args]], capture_output=True, text=True, timeout=300)
    print(r.stdout, end="", flush=True)
    if r.returncode != 0:
        print(r.stderr, file=sys.stderr)
        return r.returncode or 1
    got = [ln for ln in r.stdout.splitlines() if ln.startswith("checksum:")][0]
    if got == want:
        print("checksum equals the reference's", flush=True)
    elif lenient:
        print(f"checksum differs from the reference's (`{want}`): this scene has pairs within the margin of the threshold", flush=True)
    else:
        print(f"CHECKSUM MISMATCH: device `{got}`, reference `{want}`", file=sys.stderr)
        return 1
    return 0


def checksum(rows, counters):
    return f"checksum: rows {len(rows)} counters {counters[0]} {counters[1]} {counters[2]} sum {float(rows.astype(np.float64).sum()):.6f}"


def main_obb(exe, a, out) -> int:
    import detpost_obb_ref as oref
    import detpost_ref as ref
    A, nc, K, max_det, S = 21504, 15, 1024, 256, 64
    geo = ref.GEO_CENTER
    for name, rate in (("sparse", 0.01), ("busy", 0.3)):
        pred = obb_scene(A, nc, rate, 1)
        path, path_aa = out / f"detpost_obb_pred_{name}.bin", out / f"detpost_aa_pred_{name}.bin"
        pred.tofile(path)
        np.ascontiguousarray(pred[:4 + nc]).tofile(path_aa)
        rows, counters = ref.detpost(pred[:4 + nc], geo, "cn", 0.25, 0.45, max_det, K)
        print(f"== {name} scene (pass rate {rate}): {counters[0]} of {A} anchors pass, {counters[1]} candidates", flush=True)
        print(f"-- axis-aligned, the same boxes without the angle row: {counters[2]} kept by NMS", flush=True)
        status = run_exe(exe, [path_aa, S, A, nc, 0, 1, K, max_det, a.repeats], checksum(rows, counters))
        if status:
            return status
        found = oref.pairs(pred, 0.25, 0.45, K)
        print(f"-- oriented: the reference's margin to the threshold {found.margin:.2e}, float32 against float64 {found.err32:.2e}", flush=True)
        for mode, word in enumerate(oref.NMS_MODES):
            rows, counters = oref.detpost_obb(pred, geo, 0.25, 0.45, max_det, K, nms_mode=word, found=found)
            print(f"-- oriented, {word}: {counters[2]} kept by NMS", flush=True)
            status = run_exe(exe, [path, S, A, nc, 0, 1, K, max_det, a.repeats, 1, mode], checksum(rows, counters), lenient=found.margin < oref.MARGIN)
            if status:
                return status
    return 0


def main_extra(exe, a, out) -> int:
    import detpost_extra_ref as eref
    import detpost_ref as ref
    A, nc, E, kind, K, max_det, S = 8400, 1, 51, "kpt3", 1024, 256, 64
    geo = ref.GEO_CENTER
    for name, rate in (("quiet", 0.01), ("busy", 0.3)):
        pred = eref.with_extras(ref.random_pred(A, nc, "cn", np.float16, 1, rate, n_obj=60), "cn", eref.make_extras(A, E, kind, 2), np.float16)
        path = out / f"detpost_extra_pred_{name}.bin"
        pred.tofile(path)
        times = []
        for _ in range(5):
            t0 = time.perf_counter()
            rows, counters, extras, src = eref.detpost_extra(pred, geo, "cn", nc, E, kind, 0.25, 0.45, max_det, K)
            times.append(time.perf_counter() - t0)
        want = checksum(rows, counters) + f" extra {float(extras.astype(np.float64).sum()):.6f} src {int(src.astype(np.int64).sum())}"
        print(f"== {name} scene (pass rate {rate}): {counters[0]} of {A} anchors pass, {counters[1]} candidates, {counters[2]} kept by NMS, {len(rows)} rows", flush=True)
        print(f"NumPy reference of ONE stream on this host (tests/detpost_extra_ref.py): median {1e3 * sorted(times)[2]:.2f} ms of 5", flush=True)
        r = subprocess.run([str(exe), str(path), *[str(v) for v in (S, A, nc, 0, 1, K, max_det, a.repeats, 0, 0, E, eref.KINDS[kind])]], capture_output=True,
                           text=True, timeout=300)
        print(r.stdout, end="", flush=True)
        if r.returncode != 0:
            print(r.stderr, file=sys.stderr)
            return r.returncode or 1
        got = [ln for ln in r.stdout.splitlines() if ln.startswith("checksum:")][0]
        if got != want:
            print(f"CHECKSUM MISMATCH: device `{got}`, reference `{want}`", file=sys.stderr)
            return 1
        print("checksum equals the reference's", flush=True)
        med = [float(ln.split("median")[1].split("us")[0]) for ln in r.stdout.splitlines() if ln.startswith("k_detpost_extra")][0]
        useful = S * len(rows) * (E * (pred.itemsize + 4) + 4)
        print(f"k_detpost_extra: {useful} useful bytes ({S} x {len(rows)} rows x {E} values) in {med:.1f} us: {useful / med * 1e-3:.2f} GB/s", flush=True)
    return 0


def main_mask(exe, a, out) -> int:
    import detpost_extra_ref as eref
    import detpost_mask_ref as mref
    import detpost_ref as ref
    A, nc, E, K, max_det, S, mask, in_shape = 8400, 80, 32, 1024, 256, 64, (160, 160), (640, 640)
    geo = ref.GEO_CENTER
    rng = np.random.default_rng(3)
    proto = mref.vals(rng, (1, E) + mask).astype(np.float16)
    proto_path = out / "detpost_mask_proto.bin"
    proto.tofile(proto_path)
    for name, rate in (("quiet", 0.01), ("busy", 0.3)):
        pred = eref.with_extras(ref.random_pred(A, nc, "cn", np.float16, 1, rate, n_obj=60), "cn", mref.vals(rng, (A, E)), np.float16)
        path = out / f"detpost_mask_pred_{name}.bin"
        pred.tofile(path)
        times = []
        for _ in range(3):
            t0 = time.perf_counter()
            rows, counters, extras, src = eref.detpost_extra(pred, geo, "cn", nc, E, "raw", 0.25, 0.45, max_det, K)
            masks = mref.step9(pred[None], proto, "cn", A, rows, extras, src, mask, in_shape, False)
            times.append(time.perf_counter() - t0)
        flat = masks.reshape(-1).astype(np.int64)
        want = checksum(rows, counters) + f" extra {float(extras.astype(np.float64).sum()):.6f} src {int(src.astype(np.int64).sum())}" + \
            f" mask {int(flat.sum())} weighted {int((flat * (np.arange(flat.size) % 251 + 1)).sum())}"
        inside = sum(int(mref.window_of(mref.box_of(pred, "cn", int(an)), mask, in_shape).sum()) for an in src)
        print(f"== {name} scene (pass rate {rate}): {counters[0]} of {A} anchors pass, {counters[1]} candidates, {counters[2]} kept by NMS, {len(rows)} rows; "
              f"{inside} of {len(rows) * mask[0] * mask[1]} mask pixels inside their windows, {int(flat.sum())} set", flush=True)
        print(f"NumPy reference of ONE stream on this host (tests/detpost_extra_ref.py + detpost_mask_ref.py): median {1e3 * sorted(times)[1]:.2f} ms of 3", flush=True)
        r = subprocess.run([str(exe), str(path), *[str(v) for v in (S, A, nc, 0, 1, K, max_det, a.repeats, 0, 0, E, 0, mask[0], mask[1], in_shape[0], in_shape[1])],
                            str(proto_path)], capture_output=True, text=True, timeout=300)
        print(r.stdout, end="", flush=True)
        if r.returncode != 0:
            print(r.stderr, file=sys.stderr)
            return r.returncode or 1
        got = [ln for ln in r.stdout.splitlines() if ln.startswith("checksum:")][0]
        if got != want:
            print(f"CHECKSUM MISMATCH: device `{got}`, reference `{want}`", file=sys.stderr)
            return 1
        print("checksum equals the reference's", flush=True)
        med = {key: [float(ln.split("median")[1].split("us")[0]) for ln in r.stdout.splitlines() if ln.startswith(key)][0] for key in ("k_detpost_mask", "memset of those bytes")}
        stored, loaded = S * len(rows) * mask[0] * mask[1], S * inside * E * proto.itemsize
        print(f"k_detpost_mask: {stored} mask bytes stored + {loaded} prototype bytes inside the windows = {stored + loaded} useful bytes in "
              f"{med['k_detpost_mask']:.1f} us: {(stored + loaded) / med['k_detpost_mask'] * 1e-3:.1f} GB/s; the memset of the {stored} mask bytes alone "
              f"{med['memset of those bytes']:.1f} us ({stored / max(med['memset of those bytes'], 1e-9) * 1e-3:.1f} GB/s): ratio "
              f"{med['k_detpost_mask'] / max(med['memset of those bytes'], 1e-9):.2f}", flush=True)
    return 0


def label_scene(rng, n, cover, frame):
    """n rows [x1, y1, x2, y2, conf, cls] in frame coordinates, by descending confidence, whose boxes cover about ``cover`` times the frame area"""
    rows, cols = frame
    side = np.sqrt(cover * rows * cols / n)
    w, h = side * rng.uniform(0.6, 1.4, n), side * rng.uniform(0.6, 1.4, n)
    cx, cy = rng.uniform(0, cols, n), rng.uniform(0, rows, n)
    box = np.stack([np.clip(cx - w / 2, 0, cols), np.clip(cy - h / 2, 0, rows), np.clip(cx + w / 2, 0, cols), np.clip(cy + h / 2, 0, rows)], 1)
    box = np.round(box * 4) / 4
    conf = np.sort(rng.uniform(0.3, 0.95, n))[::-1]
    return np.concatenate([box, conf[:, None], rng.integers(0, 80, (n, 1))], 1).astype(np.float32)


def torch_labels(torch, F, geo, in_shape, d_proto, d_dets, n, d_coef, d_labels):
    """the path DetPost.labels replaces, as a caller writes it today with torch on the device, stream by stream"""
    S, rows, cols = d_labels.shape
    mh, mw = d_proto.shape[2:]
    ys = torch.arange(rows, device="cuda", dtype=torch.float32)[None, :, None]
    xs = torch.arange(cols, device="cuda", dtype=torch.float32)[None, None, :]
    for s in range(S):
        g = geo[s]
        logits = (d_coef[s, :n] @ d_proto[s].float().view(d_proto.shape[1], -1)).view(n, mh, mw)
        t, l = int(round(g.top * mh / in_shape[0])), int(round(g.left * mw / in_shape[1]))                      # scale_masks: the padding, in prototype pixels
        logits = logits[:, t:mh - t, l:mw - l]
        up = F.interpolate(logits[None], size=(rows, cols), mode="bilinear", align_corners=False)[0]
        b = d_dets[s, :n, :4, None, None]
        on = (up > 0) & (xs >= b[:, 0]) & (xs < b[:, 2]) & (ys >= b[:, 1]) & (ys < b[:, 3])
        first = on.to(torch.uint8).argmax(0)                                                            # the first True, 0 where there is none
        d_labels[s] = torch.where(on.any(0), first, torch.full_like(first, -1)).to(torch.int16)


def main_labels(exe, a, out) -> int:
    import torch
    import torch.nn.functional as F
    import detpost_labels_ref as lref
    from boxmot_amd.detpost import DetPost
    from boxmot_amd.ingest import letterbox_geometry
    E, max_det, mask, in_shape, frame = 32, 256, (160, 160), (640, 640), (1080, 1920)
    g = letterbox_geometry(frame[0], frame[1], in_shape)
    g5 = (g.gain, g.top, g.left, g.rows, g.cols)
    rng = np.random.default_rng(4)
    proto = lref.vals(rng, (E,) + mask).astype(np.float16)
    proto_path = out / "detpost_labels_proto.bin"
    proto.tofile(proto_path)
    reps = max(10, a.repeats // 5 * 5)
    for name, n, cover in (("sparse", 24, 0.3), ("busy", 180, 2.0)):
        dets, coef = label_scene(rng, n, cover, frame), lref.vals(rng, (n, E))
        dets_path, coef_path = out / f"detpost_labels_dets_{name}.bin", out / f"detpost_labels_coef_{name}.bin"
        dets.tofile(dets_path)
        coef.tofile(coef_path)
        area = float(((dets[:, 2] - dets[:, 0]) * (dets[:, 3] - dets[:, 1])).sum()) / (frame[0] * frame[1])
        print(f"== {name} scene: {n} rows per stream, boxes covering {area:.2f} x the frame area", flush=True)
        want = None
        if name == "sparse":
            t0 = time.perf_counter()
            want = lref.labels_of(g5, dets, n, coef, proto, mask, in_shape, max_det)
            print(f"NumPy reference of ONE stream on this host (tests/detpost_labels_ref.py): {time.perf_counter() - t0:.2f} s", flush=True)
        for S in (16, 64):
            post = DetPost(S, 8400, 80, extra=E, mask=mask, in_shape=in_shape, max_det=max_det)
            d_proto = torch.from_numpy(proto).cuda()[None].repeat(S, 1, 1, 1).contiguous()
            d_dets = torch.zeros((S, max_det, 6), device="cuda")
            d_coef = torch.zeros((S, max_det, E), device="cuda")
            d_dets[:, :n], d_coef[:, :n] = torch.from_numpy(dets).cuda(), torch.from_numpy(coef).cuda()
            d_rows = torch.full((S,), n, dtype=torch.int32, device="cuda")
            d_labels = torch.full((S,) + frame, -2, dtype=torch.int16, device="cuda")
            d_other = torch.full((S,) + frame, -2, dtype=torch.int16, device="cuda")
            st = torch.cuda.current_stream()
            paths = {"DetPost.labels": lambda: post.labels([g] * S, d_proto, d_dets, d_rows, d_coef, d_labels, hip_stream=st.cuda_stream),
                     "torch on the device": lambda: torch_labels(torch, F, [g] * S, in_shape, d_proto, d_dets, n, d_coef, d_other)}
            for fn in paths.values():
                fn(); fn()
            torch.cuda.synchronize()
            times = {k: [] for k in paths}
            for block in range(reps // 5):
                for key, fn in paths.items():
                    for _ in range(5):
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record(st); fn(); e1.record(st)
                        e1.synchronize()
                        times[key].append(e0.elapsed_time(e1))
            print(f"-- {S} streams of {frame[0]} x {frame[1]}, HIP events around the call, {reps} calls each in alternating blocks of 5", flush=True)
            for key, v in times.items():
                v = sorted(v)
                print(f"{key:22s} median {1e3 * v[len(v) // 2]:.1f} us  min {1e3 * v[0]:.1f}  max {1e3 * v[-1]:.1f}  ({len(v)} samples)", flush=True)
            med = {key: sorted(v)[len(v) // 2] for key, v in times.items()}
            print(f"ratio torch / DetPost.labels: {med['torch on the device'] / med['DetPost.labels']:.1f}", flush=True)
            lab, other = d_labels[0].cpu().numpy(), d_other[0].cpu().numpy()
            assert all(torch.equal(d_labels[0], d_labels[s]) for s in range(1, S))
            post.close()
            print(f"pixels where the torch path (scale_masks' integer-cropped interpolation) agrees with the label map: {100.0 * float((lab == other).mean()):.2f} %", flush=True)
            if want is not None and lab.tobytes() != want.tobytes():
                print("LABELS DIFFER FROM THE REFERENCE", file=sys.stderr)
                return 1
            if want is not None:
                print("the labels equal the reference's", flush=True)
            flat = lab.reshape(-1).astype(np.int64)
            checksum_want = f"checksum: labels sum {int(flat.sum())} weighted {int((flat * (np.arange(flat.size) % 251 + 1)).sum())} owned {int((flat >= 0).sum())}"
            del d_proto, d_dets, d_coef, d_labels, d_other
            torch.cuda.empty_cache()
            status = run_exe(exe, ["labels", dets_path, coef_path, proto_path, n, S, E, mask[0], mask[1], in_shape[0], in_shape[1], frame[0], frame[1], repr(float(g.gain)),
                                   repr(float(g.top)), repr(float(g.left)), reps], checksum_want)
            if status:
                return status
    return 0


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--streams", type=int, nargs="+", default=[1, 16, 64])
    ap.add_argument("--rates", type=float, nargs="+", default=[0.01, 0.3])
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--out", default=None, help="directory for the tensor files (default: a temporary one)")
    ap.add_argument("--build-only", action="store_true", help="compile the measuring program and stop (no device needed)")
    ap.add_argument("--obb", action="store_true", help="the oriented layout beside the axis-aligned one at 64 x 21504 x 15 (see above)")
    ap.add_argument("--extra", action="store_true", help="a pose head, 64 x 8400 x (4 + 1 + 51): the three-kernel sequence with extras (see above)")
    ap.add_argument("--mask", action="store_true", help="a segmentation head, 64 x 8400 x (4 + 80 + 32) with 32 x 160 x 160 prototypes: the four-kernel sequence (see above)")
    ap.add_argument("--labels", action="store_true", help="the frame-space label map at 16 / 64 x 1080p beside the torch-on-device path it replaces (see above)")
    a = ap.parse_args()
    exe = build()
    if a.build_only:
        return 0
    if a.labels:
        out = Path(a.out) if a.out else Path(tempfile.mkdtemp())
        out.mkdir(parents=True, exist_ok=True)
        return main_labels(exe, a, out)
    if a.mask:
        out = Path(a.out) if a.out else Path(tempfile.mkdtemp())
        out.mkdir(parents=True, exist_ok=True)
        return main_mask(exe, a, out)
    if a.extra:
        out = Path(a.out) if a.out else Path(tempfile.mkdtemp())
        out.mkdir(parents=True, exist_ok=True)
        return main_extra(exe, a, out)
    if a.obb:
        out = Path(a.out) if a.out else Path(tempfile.mkdtemp())
        out.mkdir(parents=True, exist_ok=True)
        return main_obb(exe, a, out)
    import detpost_ref as ref
    A, nc, K, max_det = 8400, 80, 1024, 256
    geo = ref.GEO_CENTER
    out = Path(a.out) if a.out else Path(tempfile.mkdtemp())
    out.mkdir(parents=True, exist_ok=True)
    for rate in a.rates:
        pred = ref.random_pred(A, nc, "cn", np.float16, 1, rate, n_obj=60)
        path = out / f"detpost_pred_{rate}.bin"
        pred.tofile(path)
        times = []
        for _ in range(5):
            t0 = time.perf_counter()
            rows, counters = ref.detpost(pred, geo, "cn", 0.25, 0.45, max_det, K)
            times.append(time.perf_counter() - t0)
        want = f"checksum: rows {len(rows)} counters {counters[0]} {counters[1]} {counters[2]} sum {float(rows.astype(np.float64).sum()):.6f}"
        print(f"== pass rate {rate}: {counters[0]} of {A} anchors pass, {counters[1]} candidates, {counters[2]} kept by NMS, {len(rows)} rows", flush=True)
        print(f"NumPy reference of ONE stream on this host (tests/detpost_ref.py): median {1e3 * sorted(times)[2]:.2f} ms of 5", flush=True)
        for S in a.streams:
            status = run_exe(exe, [path, S, A, nc, 0, 1, K, max_det, a.repeats], want)
            if status:
                return status
    return 0


if __name__ == "__main__":
    sys.exit(main())
