#!/usr/bin/env python3
"""Time the partition map: cgic_partition_map (one launch) against the unweighted cgic_paste_tiles at the same geometry.

    python tools/partition_bench.py [--iters 50] [--reps 5]

Cases: 64 images of 256x256 (a plain batch: one tile per image) and one and eight 2040x1356 images (six tiles in four shapes each),
for fp32 -> fp32, fp32 -> uint8 and uint8 -> uint8.  Per case: HIP-event time per launch from a captured graph of --iters
back-to-back launches (the same buffers every launch, so a case that fits the last-level cache is read from there), best and worst
of --reps replays.  The yardstick is cgic_paste_tiles(weighted=False) on tile batches of the same geometry and output type, timed
in the same process: it moves 12 + 12 or 12 + 3 bytes per pixel; the partition launch adds 4/16 + 4/64 + 4/256 = 0.33 bytes of masks.
The bar for a case is the paste's best time x 1.014 plus the paste's own best-to-worst spread.  uint8 -> uint8 has no paste
counterpart: its time and bytes over time are recorded without a bar.  Prints one JSON line per row."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from control_gic_amd import draw, highres  # noqa: E402


def timed_graph(fn, iters, reps):
    """(best, worst) device ms per call: `iters` calls captured into one graph, `reps` timed replays after a warm-up replay"""
    fn()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(iters):
            fn()
    graph.replay()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        graph.replay()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b) / iters)
    return min(times), max(times)


def random_masks(rng, B, th, tw, dev):
    mc = (rng.random((B, 1, th // 16, tw // 16)) < 0.35).astype(np.int32)
    free = 1 - np.repeat(np.repeat(mc, 2, 2), 2, 3)
    mm = ((rng.random((B, 1, th // 8, tw // 8)) < 0.5) & (free == 1)).astype(np.int32)
    mf = ((1 - np.repeat(np.repeat(mc, 4, 2), 4, 3)) * (1 - np.repeat(np.repeat(mm, 2, 2), 2, 3))).astype(np.int32)
    return [torch.from_numpy(m).to(dev) for m in (mc, mm, mf)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    opt = ap.parse_args()
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    for N, H, W, tile in ((64, 256, 256, 256), (1, 1356, 2040, highres.TILE), (8, 1356, 2040, highres.TILE)):
        pad, _ = highres.compute_padding(H, W)
        left, right, top, bottom = pad
        tiles = highres.tile_grid(H + top + bottom, W + left + right, tile)
        groups = highres._shape_groups(tiles)
        tile_pixels = sum(th * tw for _, _, th, tw in tiles)
        g = torch.Generator().manual_seed(N)
        x = torch.rand(N, 3, H, W, generator=g).to(dev)
        x8 = (torch.rand(N, H, W, 3, generator=g) * 255).to(torch.uint8).to(dev)
        batches = [torch.rand(N * len(idxs), 3, th, tw, generator=g).to(dev) for (th, tw), idxs in groups]
        masks = [random_masks(rng, N * len(idxs), th, tw, dev) for (th, tw), idxs in groups]
        mask_bytes = N * tile_pixels * (4 / 16 + 4 / 64 + 4 / 256)
        f32 = torch.empty(N, 3, H, W, device=dev)
        u8 = torch.empty(N, H, W, 3, dtype=torch.uint8, device=dev)
        for name, src, out, rbytes, wbytes in (("fp32->fp32", x, f32, 12, 12), ("fp32->uint8", x, u8, 12, 3), ("uint8->uint8", x8, u8, 3, 3)):
            frames = out is u8
            row = {"images": N, "hw": [H, W], "tiles": len(tiles), "what": name}
            if src is x:
                paste = lambda: highres.paste_tiles(batches, (H, W), N=N, weighted=False, out=out, frames=frames, tile=tile)
                pb, pw = timed_graph(paste, opt.iters, opt.reps)
                moved = N * (12 * tile_pixels + wbytes * H * W)
                row.update({"paste_ms": round(pb, 5), "paste_worst_ms": round(pw, 5), "paste_TB_per_s": round(moved / pb / 1e9, 3),
                            "bar_ms": round(pb * 1.014 + (pw - pb), 5)})
            part = lambda: highres.partition_tiles(src, masks, frames=frames, out=out, tile=tile)
            b, w = timed_graph(part, opt.iters, opt.reps)
            moved = N * (rbytes + wbytes) * H * W + mask_bytes
            row.update({"partition_ms": round(b, 5), "partition_worst_ms": round(w, 5), "bytes": int(moved), "partition_TB_per_s": round(moved / b / 1e9, 3)})
            if "bar_ms" in row:
                row["within_bar"] = bool(b <= row["bar_ms"])
                row["partition_over_paste"] = round(b / row["paste_ms"], 4)
            print(json.dumps(row), flush=True)
        if N == 64:
            # the plain-batch entry on the same buffers: partition_map is the one-tile form of the same launch
            m = masks[0]
            b, w = timed_graph(lambda: draw.partition_map(x, m, out=f32), opt.iters, opt.reps)
            print(json.dumps({"images": N, "hw": [H, W], "what": "partition_map fp32->fp32 (one tile per launch column)", "partition_ms": round(b, 5),
                              "partition_worst_ms": round(w, 5)}), flush=True)


if __name__ == "__main__":
    main()
