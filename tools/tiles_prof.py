"""Times of the two tiled-detection paths beside the untiled ones they sit next to, by HIP events through the library's public calls:

    letterbox_tiles            S streams x T rectangles in one launch            (csrc/ingest_letterbox_tiles.hpp)
    letterbox, T launches      the same number of output tensors, each the whole frame letterboxed (the existing kernel)
    letterbox_tiles, T x whole the new kernel on T copies of the whole-frame rectangle: the same pixels as the line above
    DetPost(tiles=T)           score over S * T tensors, one merged select / NMS workgroup per stream     (csrc/det_post_tiled.hpp)
    DetPost on S * T streams   the untiled handle on S * T pseudo-streams: the device part of what a caller could do before,
                               WITHOUT the host merge that had to follow it

16 streams of 2160 x 3840, T = 7 (the whole frame and a 2 x 3 grid, overlap 0.2), 640 x 640 fp16, 8400 anchors x 80 classes, K = 1024
by default; 5 warm-up and 30 timed calls of each, alternating, every call between its own event pair; median, min and max.  Every
step runs under a time limit (SIGALRM): a step that does not finish ends the program.

    python tools/tiles_prof.py [--streams 16] [--rows 2160] [--cols 3840] [--grid 2 3] [--repeats 30] [--pass-rate 0.05] [--out FILE]

Needs a gfx950 device.  profiles/tiles_timing.txt is the output of one such run."""
import argparse
import signal
import statistics
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))


class StepTimeout(Exception):
    pass


def _alarm(signum, frame):
    raise StepTimeout()


def timed(torch, stream, fn, warmup, repeats, limit_s):
    """per-call times in microseconds of fn() on `stream`, each between its own event pair, under one time limit"""
    signal.alarm(limit_s)
    try:
        for _ in range(warmup):
            fn()
        stream.synchronize()
        out = []
        for _ in range(repeats):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            fn()
            b.record(stream)
            b.synchronize()
            out.append(a.elapsed_time(b) * 1e3)
        return out
    finally:
        signal.alarm(0)


def line(name, us):
    return f"{name:<34s} median {statistics.median(us):8.1f} us  min {min(us):8.1f}  max {max(us):8.1f}  ({len(us)} samples)"


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--streams", type=int, default=16)
    ap.add_argument("--rows", type=int, default=2160)
    ap.add_argument("--cols", type=int, default=3840)
    ap.add_argument("--grid", type=int, nargs=2, default=(2, 3), metavar=("NY", "NX"))
    ap.add_argument("--size", type=int, nargs=2, default=(640, 640), metavar=("H", "W"))
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--pass-rate", type=float, default=0.05, help="share of a tile tensor's anchors over the threshold")
    ap.add_argument("--step-limit", type=int, default=120, help="seconds a step may take")
    ap.add_argument("--out", type=str, default=None, help="also write the report to this file")
    a = ap.parse_args()

    import torch

    import __graft_entry__ as g
    g.build()
    import detpost_ref
    from boxmot_amd.detpost import DetPost
    from boxmot_amd.ingest import FrameRing, tile_grid

    signal.signal(signal.SIGALRM, _alarm)
    S, (H, W) = a.streams, a.size
    tiles = tile_grid(a.rows, a.cols, grid=a.grid, overlap=0.2)
    T = len(tiles)
    st = torch.cuda.Stream()
    report = [f"{S} streams of {a.rows} x {a.cols}, T = {T} (the whole frame and a {a.grid[0]} x {a.grid[1]} grid of {tiles[1][3]} x {tiles[1][2]} tiles, overlap 0.2), "
              f"{H} x {W} fp16; {a.warmup} warm-up and {a.repeats} timed calls each, HIP events around every call"]

    # ---- the two letterbox kernels, alternating
    signal.alarm(a.step_limit)
    ring = FrameRing(2, S, a.rows, a.cols)
    frame = np.random.default_rng(0).integers(0, 256, (a.rows, a.cols, 3), dtype=np.uint8)
    for s in range(S):
        ring.host_view(0, s)[...] = np.roll(frame, 16 * s, axis=1)
    ring.submit(0)
    x = torch.empty((S * T, 3, H, W), dtype=torch.float16, device="cuda")
    y = torch.empty((S * T, 3, H, W), dtype=torch.float16, device="cuda")
    signal.alarm(0)

    def tiled_letterbox():
        ring.letterbox_tiles(0, x, tiles, hip_stream=st.cuda_stream)

    def whole_letterbox():                       # T launches of the existing kernel: S * T output tensors as well
        for t in range(T):
            ring.letterbox(0, y[t * S:(t + 1) * S], hip_stream=st.cuda_stream)

    def same_work_letterbox():                   # the new kernel on T copies of the whole-frame rectangle: the pixels of whole_letterbox
        ring.letterbox_tiles(0, z, [tiles[0]] * T, hip_stream=st.cuda_stream)

    z = torch.empty((S * T, 3, H, W), dtype=torch.float16, device="cuda")
    lt, lw, ls = [], [], []
    for _ in range(3):                           # alternating blocks: drift of the clocks hits all alike
        n = a.repeats // 3
        lt += timed(torch, st, tiled_letterbox, a.warmup, n, a.step_limit)
        lw += timed(torch, st, whole_letterbox, a.warmup, n, a.step_limit)
        ls += timed(torch, st, same_work_letterbox, a.warmup, n, a.step_limit)
    mt, mw, ms = statistics.median(lt), statistics.median(lw), statistics.median(ls)
    rows_of = lambda g_: sum(t_.new_h for t_ in g_) / len(g_)
    geo_t, geo_w = ring.letterbox_tiles(0, x, tiles, hip_stream=st.cuda_stream)[0], ring.letterbox(0, y[:S], hip_stream=st.cuda_stream)
    report += [line(f"letterbox_tiles, 1 launch", lt), line(f"letterbox, {T} launches", lw),
               line(f"letterbox_tiles, {T} x whole frame", ls),
               f"per output tensor: letterbox_tiles {mt / (S * T):.2f} us, letterbox {mw / (S * T):.2f} us, ratio {mt / mw:.3f}; "
               f"on the whole-frame rectangle {ms / (S * T):.2f} us, ratio {ms / mw:.3f}",
               f"picture rows per {H}-row output tensor (the rest is padding, written without a load): tiles {rows_of(geo_t):.0f}, whole frame {geo_w[0].new_h}"]
    # the tiled tensor of the whole-frame tile equals the untiled tensor of the same stream
    st.synchronize()
    same = all(torch.equal(x[s * T], y[s]) for s in range(S))
    report.append(f"tile 0 (the whole frame) of every stream equals letterbox's tensor: {same}")

    # ---- the two post-processing paths, alternating
    signal.alarm(a.step_limit)
    A, nc, K = 8400, 80, 1024
    per_tile = [detpost_ref.random_pred(A, nc, "cn", np.float16, 900 + t, a.pass_rate, n_obj=60) for t in range(T)]
    pred = torch.from_numpy(np.ascontiguousarray(np.stack(per_tile * S))).cuda()
    opts = dict(layout="cn", conf=0.25, iou=0.45, max_det=256, max_candidates=K)
    tiled = DetPost(S, A, nc, tiles=T, merge="ios", **opts)
    plain = DetPost(S * T, A, nc, **opts)
    tgeo = ring.letterbox_tiles(0, x, tiles, hip_stream=st.cuda_stream)
    pgeo = [(g_.gain, g_.top, g_.left, g_.rows, g_.cols) for gs in tgeo for g_ in gs]
    d_t, r_t = torch.zeros((S, 256, 6), device="cuda"), torch.zeros(S, dtype=torch.int32, device="cuda")
    d_p, r_p = torch.zeros((S * T, 256, 6), device="cuda"), torch.zeros(S * T, dtype=torch.int32, device="cuda")
    signal.alarm(0)
    pt, pp = [], []
    for _ in range(3):
        n = a.repeats // 3
        pt += timed(torch, st, lambda: tiled.run(pred, tgeo, d_t, r_t, hip_stream=st.cuda_stream), a.warmup, n, a.step_limit)
        pp += timed(torch, st, lambda: plain.run(pred, pgeo, d_p, r_p, hip_stream=st.cuda_stream), a.warmup, n, a.step_limit)
    ct, cp = tiled.counters(), plain.counters()
    report += [f"{A} anchors x {nc} classes per tile tensor, fp16, layout cn, K {K}, max_det 256, merge ios, pass rate {a.pass_rate}: stream 0 "
               f"tiled counters {ct[0].tolist()} rows {int(r_t[0])}; untiled pseudo-stream 0 counters {cp[0].tolist()} rows {int(r_p[0])}",
               line(f"DetPost(tiles={T}), {S} streams", pt), line(f"DetPost, {S * T} pseudo-streams", pp),
               f"ratio tiled / untiled pseudo-streams {statistics.median(pt) / statistics.median(pp):.3f} (the untiled path leaves {S * T} row "
               f"blocks in tile coordinates to be shifted, merged and NMS-ed on the host)"]
    text = "\n".join(report)
    print(text)
    if a.out:
        Path(a.out).write_text(text + "\n")
    tiled.close(); plain.close(); ring.close()
    return 0


if __name__ == "__main__":
    try:
        sys.exit(main())
    except StepTimeout:
        print("tiles_prof: a step ran past its time limit", file=sys.stderr)
        sys.exit(124)
