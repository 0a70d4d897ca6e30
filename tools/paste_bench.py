#!/usr/bin/env python3
"""Time the way out of the tiling driver: cgic_paste_tiles (one launch) against the loop it replaces.

    python tools/paste_bench.py [--hw 1356 2040] [--images 1 8] [--iters 50] [--tile 768]

For N images of one size: HIP-event time per call of highres.paste_tiles with fp32 and with uint8 output (out= given: no
allocation) -- `device_ms` from a captured graph of --iters launches (back to back on the device: the same buffers every launch, so
an image that fits the last-level cache is read from there), `eager_*` call by call from Python --, and on the same tensors the wall and device time of the blend part of highres.decompress_tiled(decode=...) -- the
reference's loop (inference_high_resolution.py:231-255) on torch ops, one image at a time, unchanged code restated here because
the original sits behind a decompress.  Bytes per second count 12 B read per tile pixel and 12 B (fp32) or 3 B (uint8) written
per image pixel.  Prints one JSON line per row."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from control_gic_amd import highres  # noqa: E402


def blend_loop(tile_px, tiles, pad, H, W, dev):
    """highres.decompress_tiled's blend part, line for line (one image)"""
    left, right, top, bottom = pad
    rec = torch.zeros((1, 3, H + top + bottom, W + left + right), device=dev)
    contrib = torch.zeros_like(rec)
    for (y, x, th, tw), p in zip(tiles, tile_px):
        wts = highres.gaussian_weights(tw, th, dev)
        rec[:, :, y:y + th, x:x + tw] += p * wts
        contrib[:, :, y:y + th, x:x + tw] += wts
    rec = (rec / contrib).clamp(0, 1)
    return rec[:, :, top:top + H, left:left + W]


def timed(fn, iters):
    """(device ms per call from HIP events over `iters` calls, wall ms per call with a synchronise at the end)"""
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters, (time.perf_counter() - t0) * 1e3 / iters


def timed_graph(fn, iters, reps=5):
    """device ms per call: `iters` calls captured into one graph (no host work between the launches), best of `reps` replays"""
    fn()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(iters):
            fn()
    best = float("inf")
    for _ in range(reps + 1):                      # (the first replay warms up)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        graph.replay()
        b.record()
        torch.cuda.synchronize()
        best = min(best, a.elapsed_time(b) / iters)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hw", type=int, nargs=2, default=(1356, 2040))
    ap.add_argument("--images", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--loop-iters", type=int, default=5)
    ap.add_argument("--tile", type=int, default=highres.TILE)
    opt = ap.parse_args()
    dev = torch.device("cuda", 0)
    H, W = opt.hw
    pad, _ = highres.compute_padding(H, W)
    left, right, top, bottom = pad
    tiles = highres.tile_grid(H + top + bottom, W + left + right, opt.tile)
    groups = highres._shape_groups(tiles)
    tile_pixels = sum(th * tw for _, _, th, tw in tiles)
    for N in opt.images:
        g = torch.Generator().manual_seed(N)
        batches = [(torch.rand(N * len(idxs), 3, th, tw, generator=g) * 1.4 - 0.2).to(dev) for (th, tw), idxs in groups]
        f32 = torch.empty(N, 3, H, W, device=dev)
        u8 = torch.empty(N, H, W, 3, dtype=torch.uint8, device=dev)
        for name, out, wbytes in (("paste fp32", f32, 12), ("paste uint8", u8, 3)):
            fn = lambda: highres.paste_tiles(batches, (H, W), N=N, out=out, frames=out is u8, tile=opt.tile)
            eager_ms, wall_ms = timed(fn, opt.iters)
            dev_ms = timed_graph(fn, opt.iters)
            moved = N * (12 * tile_pixels + wbytes * H * W)
            print(json.dumps({"what": name, "images": N, "hw": [H, W], "tiles": len(tiles), "device_ms": round(dev_ms, 5),
                              "eager_event_ms": round(eager_ms, 5), "eager_wall_ms": round(wall_ms, 5),
                              "bytes": moved, "TB_per_s": round(moved / dev_ms / 1e9, 3)}))
        # the loop: per image, tile by tile (row-major), on the same tile tensors
        per_image = [[None] * len(tiles) for _ in range(N)]
        for b, (_, idxs) in zip(batches, groups):
            for n in range(N):
                for k, i in enumerate(idxs):
                    per_image[n][i] = b[n * len(idxs) + k][None]
        loop = lambda: [blend_loop(per_image[n], tiles, pad, H, W, dev) for n in range(N)]
        dev_ms, wall_ms = timed(loop, opt.loop_iters)
        same = all(torch.equal(r[0], f) for r, f in zip(loop(), highres.paste_tiles(batches, (H, W), N=N, tile=opt.tile)))
        print(json.dumps({"what": "loop (decompress_tiled's blend)", "images": N, "hw": [H, W], "device_ms": round(dev_ms, 4), "wall_ms": round(wall_ms, 4),
                          "equal_to_paste_on_device": bool(same)}))


if __name__ == "__main__":
    main()
