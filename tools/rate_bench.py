#!/usr/bin/env python3
"""Rate table vs. one compress pass per candidate, same box, one JSON line.

At B images of HxW and C candidate ratios (default_candidates around coarse 0.1):
  rate:  grain_indices (VQ of the three encoder heads, quant_conv fused) + rate_table (pixels given: refined masks)
  plain: per candidate: grain_merge + VQ (quant_conv fused) + router (pixels given) + compress_streams  -- what finding the
         bpp of C ratios costs without the table
Latents are random (the conv encoder is not part of either path).

--curve: the rate curve next to the table, library entry points only (buffers allocated once, no VQ): cgic_rate_table at
C = 16 and C = 64 candidates and cgic_rate_curve (all n8 + 1 medium ranks), on the same maps as given (no pixels: the
curve's contract) -- plus the table at C = 16 with the pixels, as compress_to_bpp calls it.  HIP-event time per call over
--iters back-to-back calls after warm-up, the variants alternating over --rounds rounds; the median round is reported.

    python tools/rate_bench.py [--B 64] [--H 256] [--C 16] [--iters 20]
    python tools/rate_bench.py --curve [--B 64] [--H 256] [--iters 200] [--rounds 5]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import control_gic_amd as cg  # noqa: E402
from control_gic_amd import _lib  # noqa: E402
from control_gic_amd.quantize import _vq_forward  # noqa: E402


def curve_bench(a, dev, codec, inds, e16, e8, x):
    """cgic_rate_table (C = 16, 64) against cgic_rate_curve: device time per call"""
    import ctypes
    l = _lib.lib()
    B, h16, w16 = e16.shape
    n8 = 4 * h16 * w16
    tab = codec.huffman.table.handle
    stream = _lib.current_stream(dev)
    ptrs = [_lib.ptr(t) for t in (*inds, e16, e8)]
    variants = {}

    def table_variant(C, pixels):
        cands = cg.default_candidates(0.1, C)
        cr = (ctypes.c_double * C)(*[c for c, _ in cands])
        mr = (ctypes.c_double * C)(*[m for _, m in cands])
        nb = torch.empty((C, B, 5), dtype=torch.int32, device=dev)
        ws = torch.empty(l.cgic_rate_table_workspace_bytes(B, h16, w16, C, 1), dtype=torch.uint8, device=dev)
        px, keep = _lib.pixels_arg(pixels, B, h16, w16, 1, flat8=getattr(e8, "_cgic_flat8", None) if pixels is not None else None)
        return lambda: _lib.call("cgic_rate_table", tab, *ptrs, B, h16, w16, C, cr, mr, 1, px, _lib.ptr(nb), _lib.ptr(ws), stream), (nb, ws, keep)

    variants["table_C16_us"] = table_variant(16, None)
    variants["table_C64_us"] = table_variant(64, None)
    variants["table_C16_pixels_us"] = table_variant(16, x)
    nbc = torch.empty((B, n8 + 1, 5), dtype=torch.int32, device=dev)
    wsc = torch.empty(l.cgic_rate_curve_workspace_bytes(B, h16, w16), dtype=torch.uint8, device=dev)
    variants["curve_us"] = (lambda: _lib.call("cgic_rate_curve", tab, *ptrs, B, h16, w16, 0.1, _lib.ptr(nbc), _lib.ptr(wsc), stream), (nbc, wsc))

    # the curve holds the table's candidates (maps as given): same sizes
    variants["table_C64_us"][0]()
    variants["curve_us"][0]()
    cands = cg.default_candidates(0.1, 64)
    ks = [cg.router_ranks(c, m, h16 * w16)[1] for c, m in cands[1:-1]]
    exact = torch.equal(nbc[:, torch.tensor(ks, device=dev)], variants["table_C64_us"][1][0][1:-1].permute(1, 0, 2))
    times = {k: [] for k in variants}
    for fn, _ in variants.values():
        for _ in range(a.warmup):
            fn()
    torch.cuda.synchronize()
    for _ in range(a.rounds):
        for name, (fn, _) in variants.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(a.iters):
                fn()
            t1.record()
            torch.cuda.synchronize()
            times[name].append(t0.elapsed_time(t1) * 1000.0 / a.iters)
    out = {"metric": "rate_curve_vs_rate_table", "B": B, "H": 16 * h16, "W": 16 * w16, "ranks": n8 + 1, "exact": exact,
           "iters": a.iters, "rounds": a.rounds}
    for name, v in times.items():
        out[name] = round(sorted(v)[len(v) // 2], 1)
        out[name.replace("_us", "_spread_us")] = [round(min(v), 1), round(max(v), 1)]
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=64)
    ap.add_argument("--H", type=int, default=256)
    ap.add_argument("--C", type=int, default=16)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--curve", action="store_true", help="cgic_rate_curve next to cgic_rate_table (entry points only)")
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    B, H = a.B, a.H
    x = torch.from_numpy(rng.random((B, 3, H, H)).astype(np.float32)).to(dev)
    heads = [torch.from_numpy(rng.standard_normal((B, 4, H // s, H // s)).astype(np.float32)).to(dev) for s in (16, 8, 4)]
    vq = cg.VectorQuantizer(1024, 4, beta=0.25).to(dev).eval()
    vq.embedding.weight.data.copy_(torch.from_numpy(rng.standard_normal((1024, 4)).astype(np.float32)))
    vq.usage_counter.copy_(torch.from_numpy(np.floor(1e6 / (1 + np.arange(1024)) ** 1.1).astype(np.float32)))
    qc = torch.nn.Conv2d(4, 4, 1).to(dev)
    codec = cg.GrainCodec(cg.HuffmanCoding(vq.embedding_counter), vq.embedding.weight)
    cands = cg.default_candidates(0.1, a.C)
    with torch.no_grad():
        e8, e16 = cg.entropy_maps(x)
        if a.curve:
            inds = cg.grain_indices(vq, *heads, quant_conv=qc)
            return curve_bench(a, dev, codec, inds, e16, e8, x)

        def rate():
            inds = cg.grain_indices(vq, *heads, quant_conv=qc)
            return cg.rate_table(codec, *inds, e16, e8, cands, per_image=True, pixels=x)

        def plain():
            out = []
            for c, m in cands:
                masks, _, _, mode = cg.TripleGrainFixedEntropyRouter(c, m, per_image=True)(e16, e8, want_gate=False, pixels=x)
                h = cg.grain_merge(*heads, masks)
                ind = _vq_forward(h, vq.embedding.weight, 0.25, True, None, False, False, quant_conv=qc,
                                  prepared=vq._prepared_image())[2]
                out.append(codec.compress(ind, masks, mode).nbytes)
            return out

        tab = rate()
        ref = plain()
        exact = all(torch.equal(tab.nbytes[i], ref[i].clamp(min=0)) for i in range(len(cands)))

        def timed(fn):
            for _ in range(a.warmup):
                fn()
            torch.cuda.synchronize()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(a.iters):
                fn()
            t1.record()
            torch.cuda.synchronize()
            return t0.elapsed_time(t1) * 1000.0 / a.iters

        rate_us, plain_us = timed(rate), timed(plain)
    print(json.dumps({"metric": "rate_table_vs_compress_passes", "B": B, "H": H, "W": H, "C": len(cands), "exact": exact,
                      "rate_us": round(rate_us, 1), "plain_C_passes_us": round(plain_us, 1),
                      "plain_pass_us": round(plain_us / len(cands), 1), "rate_in_passes": round(rate_us / (plain_us / len(cands)), 2)}))


if __name__ == "__main__":
    main()
