#!/usr/bin/env python3
"""Time the device-side container (container.pack_device / container.load: csrc/cgic_container.hip) against the host paths it sits
next to (container.pack(entries_from_*) on to_host() results; CompressedBatch.from_host(unpack(blob))).

    python tools/container_bench.py [--rounds 5] [--iters 20] [--trace-loop N]

Shapes: 64 images of 256x256 at ratio (0.1, 0.8, 0.1), and eight 2040x1356 images through compress_tiled_batch (six tiles in four
shapes each).  Per shape, both paths in this one process, alternating, --rounds rounds of --iters calls each (a round's figure is the
mean of its calls); reported: the median round and the lowest and highest one.
  out   wall time from "the compress has been enqueued" (not finished: nothing has synchronised) to "a bytes object exists"
  pack  HIP-event time of the pack launches alone (the streams already on the device; --iters calls captured into one graph and
        replayed, so that the host's enqueue time is not in the figure)
  in    wall time from the file's bytes to decodable slot buffers on the device (ends in a device synchronise)
and the bytes each path moves between device and host.  The expectation is that the device path is no slower than the host path beyond
the host path's own round-to-round spread: `within` says whether median(device) <= median(host) + (max(host) - min(host)).
The two paths' bytes are compared before anything is timed.  Prints one JSON line per row.
--trace-loop N: no timing; N pack_device and N load calls per shape, for a kernel trace taken in a run of its own."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import control_gic_amd as cg  # noqa: E402
from control_gic_amd import container, highres  # noqa: E402
from control_gic_amd.quantize import vq_forward_route  # noqa: E402


def rounds_of(paths, rounds, iters):
    """{name: [mean seconds per call of each round]} for paths = {name: callable}, alternating the paths inside every round"""
    for fn in paths.values():
        fn()
    out = {k: [] for k in paths}
    for _ in range(rounds):
        for name, fn in paths.items():
            t = 0.0
            for _ in range(iters):
                t += fn()
            out[name].append(t / iters)
    return out


def stats(v):
    return {"median_us": round(statistics.median(v) * 1e6, 2), "min_us": round(min(v) * 1e6, 2), "max_us": round(max(v) * 1e6, 2)}


def report(what, shape, res, host, device, extra):
    h, d = res[host], res[device]
    row = {"shape": shape, "what": what, "host": stats(h), "device": stats(d),
           "device_over_host": round(statistics.median(d) / statistics.median(h), 4),
           "within": bool(statistics.median(d) <= statistics.median(h) + (max(h) - min(h)))}
    row.update(extra)
    print(json.dumps(row), flush=True)


def host_load(blob, codec, dev):
    """the way in that exists without the device side: unpack, then one from_host per (height, width, mode)"""
    groups = {}
    for e in container.unpack(blob):
        groups.setdefault((e["height"], e["width"], e["mode"]), []).append(e["streams"])
    return [cg.CompressedBatch.from_host(ims, mode, hh // 4, ww // 4, codec.slot_bytes(hh // 4, ww // 4), dev) for (hh, ww, mode), ims in groups.items()]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--trace-loop", type=int, default=0)
    opt = ap.parse_args()
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    freq = np.floor(1e6 / (1 + np.arange(1024)) ** 1.1).astype(np.int64)
    vq = cg.VectorQuantizer(1024, 4, beta=0.25).to(dev).eval()
    with torch.no_grad():
        vq.embedding.weight.copy_(torch.from_numpy(rng.standard_normal((1024, 4)).astype(np.float32)))
    vq.usage_counter.copy_(torch.from_numpy(freq.astype(np.float32)))
    codec = cg.GrainCodec(vq.embedding_counter, vq.embedding.weight.detach())
    sync = torch.cuda.synchronize

    def timed_out(compress, finish):
        def fn():
            sync()
            comp = compress()
            t0 = time.perf_counter()                  # the compress is enqueued; nothing has waited for it
            finish(comp)
            return time.perf_counter() - t0
        return fn

    def timed_in(load):
        def fn():
            sync()
            t0 = time.perf_counter()
            keep = load()
            sync()
            dt = time.perf_counter() - t0
            del keep
            return dt
        return fn

    def events(pack, iters):
        """device seconds per call: `iters` calls captured into one graph (the enqueue costs more host time than the launches take
        on the device), a warm-up replay, one timed replay"""
        pack()
        sync()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            keep = [pack() for _ in range(iters)]
        graph.replay()
        sync()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        graph.replay()
        b.record()
        sync()
        del keep
        return a.elapsed_time(b) * 1e-3 / iters

    # ---- 64 x 256x256 ---------------------------------------------------------------------------------------------------------
    B, H, W = 64, 256, 256
    ind = torch.from_numpy(rng.choice(1024, size=(B, H // 4, W // 4), p=freq / freq.sum()).astype(np.int64)).to(dev)
    e16 = torch.from_numpy((rng.random((B, H // 16, W // 16)) * 2.6).astype(np.float32)).to(dev)
    e8 = torch.from_numpy((rng.random((B, H // 8, W // 8)) * 2.6).astype(np.float32)).to(dev)
    mask, _, _, mode = cg.TripleGrainFixedEntropyRouter(0.1, 0.8, per_image=True)(e16, e8)
    compress = lambda: codec.compress(ind, mask, mode)
    host_out = lambda comp: container.pack(container.entries_from_batch(comp, H, W))
    dev_out = lambda comp: container.pack_device(comp, H, W).tobytes()
    comp = compress()
    blob = host_out(comp)
    assert dev_out(comp) == blob, "the device container differs from container.pack"
    nb = comp.nbytes.cpu()
    slot = comp.data.shape[2]
    shape = f"{B} x {H}x{W}"
    for _ in range(opt.trace_loop):
        container.pack_device(comp, H, W)
        container.load(blob, codec, dev)
    moved = {"file_bytes": len(blob), "slot_bytes": B * 5 * slot,
             "d2h_host_path": B * 5 * max(int(nb.max()), 0) + nb.numel() * 4, "d2h_device_path": len(blob) + 8}
    if not opt.trace_loop:
        res = rounds_of({"host": timed_out(compress, host_out), "device": timed_out(compress, dev_out)}, opt.rounds, opt.iters)
        report("out: compress enqueued -> bytes", shape, res, "host", "device", moved)
        ev = [events(lambda: container.pack_device(comp, H, W), opt.iters) for _ in range(opt.rounds)]
        print(json.dumps({"shape": shape, "what": "pack launches (HIP events)", "device": stats(ev), "launches": 3}), flush=True)
    back = container.load(blob, codec, dev)
    assert back.batch().to_host() == comp.to_host() and [c.to_host() for c in host_load(blob, codec, dev)] == [comp.to_host()]
    moved = {"file_bytes": len(blob), "h2d_host_path": B * 5 * slot + nb.numel() * 4, "h2d_device_path": (len(blob) + 15) // 16 * 16}
    if not opt.trace_loop:
        res = rounds_of({"host": timed_in(lambda: host_load(blob, codec, dev)), "device": timed_in(lambda: container.load(blob, codec, dev))},
                        opt.rounds, opt.iters)
        report("in: bytes -> decodable buffers", shape, res, "host", "device", moved)

    # ---- eight 2040x1356 images, tiled ----------------------------------------------------------------------------------------
    N, H, W = 8, 1356, 2040
    x = torch.from_numpy(rng.random((N, 3, H, W), dtype=np.float32)).to(dev)

    def encode(tiles):                      # a stand-in encoder that is a function of each tile's own pixels
        z = torch.nn.functional.avg_pool2d(tiles, 4)
        z = torch.cat([z, z[:, :1] * 2 - 1], dim=1) * 3 - 1.5
        e8, e16 = cg.entropy_maps(tiles)
        _, _, ind, mask, _, mode = vq_forward_route(z.contiguous(), vq.embedding.weight, 0.25, True, e16, e8, 0.1, 0.8, per_image=True)
        return ind, mask, mode

    compress = lambda: highres.compress_tiled_batch(x, encode, codec)
    host_out = lambda tiled: container.pack([e for n, t in enumerate(tiled) for e in container.entries_from_tiled(t, n)])
    dev_out = lambda tiled: container.pack_device(tiled).tobytes()
    tiled = compress()
    blob = host_out(tiled)
    assert dev_out(tiled) == blob, "the device container differs from container.pack"
    shared = tiled[0]._whole[0]
    slots = sum(c.data.numel() for _, c, _ in shared)
    d2h_host = sum(t_c.batch * 5 * max(int(t_c.nbytes.max()), 0) + t_c.nbytes.numel() * 4 for t in tiled for _, t_c, _ in t.groups)
    shape = f"{N} x {H}x{W} tiled ({N * len(tiled[0].tiles)} entries)"
    iters = max(opt.iters // 4, 1)
    for _ in range(opt.trace_loop):
        container.pack_device(tiled)
        container.load(blob, codec, dev)
    if opt.trace_loop:
        torch.cuda.synchronize()
        return
    moved = {"file_bytes": len(blob), "slot_bytes": slots, "d2h_host_path": d2h_host, "d2h_device_path": len(blob) + 8}
    res = rounds_of({"host": timed_out(compress, host_out), "device": timed_out(compress, dev_out)}, opt.rounds, iters)
    report("out: compress enqueued -> bytes", shape, res, "host", "device", moved)
    ev = [events(lambda: container.pack_device(tiled), opt.iters) for _ in range(opt.rounds)]
    print(json.dumps({"shape": shape, "what": "pack launches (HIP events)", "device": stats(ev), "launches": 3}), flush=True)
    back = container.load(blob, codec, dev).tiled((H, W))
    assert [t.streams() for t in back] == [t.streams() for t in tiled]
    moved = {"file_bytes": len(blob), "h2d_host_path": slots + sum(c.nbytes.numel() * 4 for _, c, _ in shared),
             "h2d_device_path": (len(blob) + 15) // 16 * 16}
    res = rounds_of({"host": timed_in(lambda: host_load(blob, codec, dev)),
                     "device": timed_in(lambda: container.load(blob, codec, dev).tiled((H, W)))}, opt.rounds, iters)
    report("in: bytes -> decodable buffers", shape, res, "host", "device", moved)


if __name__ == "__main__":
    main()
