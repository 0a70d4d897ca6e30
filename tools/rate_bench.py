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

--tiled: rate control of tiled 2040x1356 images (six tiles of four shapes each), N = 1 and N = 8 images:
  baseline: what can be written without cgic_rate_curve_tiles -- one cgic_rate_curve per shape group, the device -> host copy
            of the full per-tile curves, the fold over the settings on the host
  feature:  one cgic_rate_curve_tiles call (axis built, descriptors uploaded once) and the copy of image_nbytes [N, M, 5]
Device time by HIP events per call over --iters calls, and wall time to the folded result on the host; the variants alternate
over --rounds rounds; median round and [min, max].  Also the host time of tiled_settings, and compress_tiled_to_bpp of a
stand-in model against one compress_tiled_batch at a fixed ratio.

--device: the device-side rate pick against the host's, to the point where the masks and merged indices of the picked rank
exist on the device:
  host:    rate_curve (the [B, n8+1, 5] table to the host) -> choose -> router at the picked ratio -> gather_grain_indices
  device:  route_to_bpp (cgic_route_to_budget: curve at the reachable ranks, pick, masks + indices; nothing read back)
Wall time per call with a synchronisation after each (the host leg counts), and HIP-event device time of the entry points
called back to back on preallocated buffers: the host path's three launches (curve, router, gather) one by one, and the
chain.  The variants alternate over --rounds rounds; median round and [min, max].

    python tools/rate_bench.py [--B 64] [--H 256] [--C 16] [--iters 20]
    python tools/rate_bench.py --device [--B 64] [--H 256] [--iters 200] [--rounds 5]
    python tools/rate_bench.py --tiled [--iters 50] [--rounds 5]
    python tools/rate_bench.py --curve [--B 64] [--H 256] [--iters 200] [--rounds 5]
"""
import argparse
import ctypes
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


def device_bench(a, dev, codec, inds, e16, e8):
    """the host's rate pick (curve -> choose -> router -> gather) against route_to_bpp"""
    import time
    from control_gic_amd import rate
    l = _lib.lib()
    B, h16, w16 = e16.shape
    n16, n8, coarse = h16 * w16, 4 * h16 * w16, 0.1
    tab = codec.huffman.table.handle
    stream = _lib.current_stream(dev)
    ptrs = [_lib.ptr(t) for t in (*inds, e16, e8)]
    K, m = rate.reachable_ranks_vec(n16, coarse)
    ranks = tuple(zip(K.tolist(), m.tolist()))
    curve = cg.rate_curve(codec, *inds, e16, e8, coarse, ranks=ranks)
    bb = curve.batch_bpp[K]
    target = float(bb.median())

    def host_path():
        cv = cg.rate_curve(codec, *inds, e16, e8, coarse, ranks=ranks)
        k, _ = cg.choose(cv, target)
        c, md = cv.ratio(k)
        masks, _, _, _ = cg.TripleGrainFixedEntropyRouter(c, md, per_image=True)(e16, e8, want_gate=False)
        return k, masks, cg.gather_grain_indices(*inds, masks)

    def device_path():
        return cg.route_to_bpp(codec, *inds, e16, e8, coarse, target_bpp=target)

    k, masks, ind = host_path()
    route = device_path()
    exact = route.rank == k and all(torch.equal(x, y) for x, y in zip(route.masks + [route.ind], masks + [ind]))

    # the entry points on preallocated buffers
    R = int(K.numel())
    ranks_dev = K.to(torch.int32).to(dev)
    budget = torch.tensor([cg.budget_bytes(target, 256 * n16, B)], dtype=torch.int64, device=dev)
    mc, mm, mf = (torch.empty_like(t) for t in masks)
    out_ind, choice = torch.empty_like(ind), torch.empty(4, dtype=torch.int64, device=dev)
    nbc = torch.empty((B, n8 + 1, 5), dtype=torch.int32, device=dev)
    wsc = torch.empty(l.cgic_rate_curve_workspace_bytes(B, h16, w16), dtype=torch.uint8, device=dev)
    wsr = torch.empty(l.cgic_route_to_budget_workspace_bytes(B, h16, w16, R), dtype=torch.uint8, device=dev)
    mode = ctypes.c_int(0)
    md = curve.ratio(k)[1]
    launches = {
        "host_curve_launch_us": lambda: _lib.call("cgic_rate_curve", tab, *ptrs, B, h16, w16, coarse, _lib.ptr(nbc), _lib.ptr(wsc), stream),
        "host_router_launch_us": lambda: _lib.call("cgic_router_f32", ptrs[3], ptrs[4], B, h16, w16, coarse, md, 1, _lib.ptr(mc), _lib.ptr(mm),
                                                   _lib.ptr(mf), None, ctypes.byref(mode), None, stream),
        "host_gather_launch_us": lambda: _lib.call("cgic_gather_grain_indices", ptrs[0], ptrs[1], ptrs[2], _lib.ptr(mc), _lib.ptr(mm), _lib.ptr(mf),
                                                   B, 4 * h16, 4 * w16, _lib.ptr(out_ind), stream),
        "device_chain_us": lambda: _lib.call("cgic_route_to_budget", tab, *ptrs, B, h16, w16, coarse, _lib.ptr(ranks_dev), R, _lib.ptr(budget),
                                             _lib.ptr(mc), _lib.ptr(mm), _lib.ptr(mf), _lib.ptr(out_ind), _lib.ptr(choice), _lib.ptr(wsr), stream),
    }
    walls = {"host_path_wall_us": host_path, "device_path_wall_us": device_path}
    times = {n: [] for n in list(launches) + list(walls)}
    for fn in list(launches.values()) + list(walls.values()):
        for _ in range(a.warmup):
            fn()
    torch.cuda.synchronize()
    for _ in range(a.rounds):
        for name, fn in launches.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(a.iters):
                fn()
            t1.record()
            torch.cuda.synchronize()
            times[name].append(t0.elapsed_time(t1) * 1000.0 / a.iters)
        for name, fn in walls.items():
            iters = max(a.iters // 4, 3)
            torch.cuda.synchronize()
            w0 = time.perf_counter()
            for _ in range(iters):
                fn()
                torch.cuda.synchronize()
            times[name].append((time.perf_counter() - w0) * 1e6 / iters)
    out = {"metric": "route_to_bpp_vs_host_pick", "B": B, "H": 16 * h16, "W": 16 * w16, "ranks": R, "exact": bool(exact), "picked_rank": int(k),
           "iters": a.iters, "rounds": a.rounds}
    for name, v in times.items():
        out[name] = round(sorted(v)[len(v) // 2], 1)
        out[name.replace("_us", "_spread_us")] = [round(min(v), 1), round(max(v), 1)]
    out["host_launches_sum_us"] = round(out["host_curve_launch_us"] + out["host_router_launch_us"] + out["host_gather_launch_us"], 1)
    print(json.dumps(out))


class _StandIn(torch.nn.Module):
    """three strided convolutions as encoder heads, a router from the config, the library's VQ: enough of a model for
    compress_tiled_to_bpp (the real encoder is not part of what is measured)"""

    def __init__(self):
        super().__init__()
        nn = torch.nn
        self.encoder = nn.Module()
        self.encoder.conv_out_coarse, self.encoder.conv_out, self.encoder.conv_out_fine = \
            nn.Conv2d(3, 4, 16, stride=16), nn.Conv2d(3, 4, 8, stride=8), nn.Conv2d(3, 4, 4, stride=4)
        self.encoder.router_config = {"target": "", "params": {"coarse_grain_ratio": 0.1, "medium_grain_ratio": 0.4}}
        self.entropy_calculation_p8, self.entropy_calculation_p16 = cg.Entropy(8), cg.Entropy(16)
        self.quant_conv = nn.Conv2d(4, 4, 1)
        self.quantize = cg.VectorQuantizer(1024, 4, beta=0.25)

    def encode(self, x):
        e8, e16 = self.entropy_calculation_p8(x), self.entropy_calculation_p16(x)
        enc, p = self.encoder, self.encoder.router_config["params"]
        hc, hm, hf = enc.conv_out_coarse(x), enc.conv_out(x), enc.conv_out_fine(x)
        router = cg.TripleGrainFixedEntropyRouter(p["coarse_grain_ratio"], p["medium_grain_ratio"], per_image=p.get("per_image", False))
        mask, gate, fine_ratio, mode = router(e16, e8)
        quant, loss, ind = self.quantize(self.quant_conv(cg.grain_merge(hc, hm, hf, mask)))
        return quant, loss, None, mask, ind, fine_ratio, mode


def tiled_bench(a, dev):
    import time
    from control_gic_amd import highres, rate
    l = _lib.lib()
    rng = np.random.default_rng(0)
    H, W, coarse = 1356, 2040, 0.1
    vq = cg.VectorQuantizer(1024, 4, beta=0.25).to(dev).eval()
    vq.embedding.weight.data.copy_(torch.from_numpy(rng.standard_normal((1024, 4)).astype(np.float32)))
    vq.usage_counter.copy_(torch.from_numpy(np.floor(1e6 / (1 + np.arange(1024)) ** 1.1).astype(np.float32)))
    codec = cg.GrainCodec(cg.HuffmanCoding(vq.embedding_counter), vq.embedding.weight)
    tab = codec.huffman.table.handle
    stream = _lib.current_stream(dev)
    out = {"metric": "rate_curve_tiled_vs_per_group_curves", "H": H, "W": W, "coarse": coarse, "iters": a.iters, "rounds": a.rounds}

    rate.reachable_ranks_vec.cache_clear()
    rate._tiled_settings.cache_clear()
    shapes16 = [48 * 48, 37 * 48, 48 * 32, 37 * 32]
    t0 = time.perf_counter()
    mediums, ranks = cg.tiled_settings(shapes16, coarse)
    out["tiled_settings_cold_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
    t0 = time.perf_counter()
    cg.tiled_settings(shapes16, coarse)
    out["tiled_settings_cached_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
    out["settings"] = int(mediums.numel())

    for N in (1, 8):
        x = torch.from_numpy((rng.integers(0, 256, (N, 3, H, W)) / 255.0).astype(np.float32)).to(dev)
        pad, grid, order, batches = highres.cut_groups(x)
        groups = []
        for ((th, tw), idxs), batch in zip(order, batches):
            B = batch.shape[0]
            heads = [torch.from_numpy(rng.standard_normal((B, 4, th // s, tw // s)).astype(np.float32)).to(dev) for s in (16, 8, 4)]
            e8, e16 = cg.entropy_maps(batch, reference_order=True)
            groups.append((*cg.grain_indices(vq, *heads), e16.contiguous(), e8.contiguous(), [n for n in range(N) for _ in idxs]))
        shapes = [(th // 16, tw // 16) for (th, tw), _ in order]
        mediums, ranks = cg.tiled_settings([h * w for h, w in shapes], coarse)
        M, S = int(mediums.numel()), len(shapes)
        curve = cg.rate_curve_tiled(codec, groups, coarse, image_hw=(H, W), settings=(mediums, ranks), ends=False)

        # ---- baseline: a curve per group, all of it to the host, the fold there
        base = []
        for (ic, im, if_, e16, e8, images), (h16, w16) in zip(groups, shapes):
            B, n8 = len(images), 4 * h16 * w16
            nb = torch.empty((B, n8 + 1, 5), dtype=torch.int32, device=dev)
            ws = torch.empty(l.cgic_rate_curve_workspace_bytes(B, h16, w16), dtype=torch.uint8, device=dev)
            base.append(([_lib.ptr(t) for t in (ic, im, if_, e16, e8)], B, h16, w16, nb, ws, torch.tensor(images)))

        def base_launch():
            for ptrs, B, h16, w16, nb, ws, _ in base:
                _lib.call("cgic_rate_curve", tab, *ptrs, B, h16, w16, coarse, _lib.ptr(nb), _lib.ptr(ws), stream)

        def base_full():
            base_launch()
            folded = torch.zeros((N, M, 5), dtype=torch.int64)
            for s, (_, _, _, _, nb, _, images) in enumerate(base):
                folded.index_add_(0, images, nb.cpu()[:, ranks[s]].to(torch.int64))
            return folded

        # ---- feature: one call, descriptors and ranks uploaded once
        T = len(curve.tile_image)
        desc = (_lib.RateTile * T)()
        off, t = [0] * 5, 0
        for (ic, im, if_, e16, e8, images), (h16, w16) in zip(groups, shapes):
            n16 = h16 * w16
            for k, n in enumerate(images):
                desc[t] = _lib.RateTile(h16, w16, round(n16 * coarse), shapes.index((h16, w16)), n, 0, off[0] + k * n16, off[1] + 4 * k * n16,
                                        off[2] + 16 * k * n16, off[3] + k * n16, off[4] + 4 * k * n16)
                t += 1
            for i, per in enumerate((n16, 4 * n16, 16 * n16, n16, 4 * n16)):
                off[i] += len(images) * per
        bufs = [torch.cat([g[i].reshape(-1) for g in groups]) for i in range(5)]
        count = (ctypes.c_int64 * 5)(*[b.numel() for b in bufs])
        desc_dev = torch.frombuffer(bytearray(bytes(desc)), dtype=torch.uint8).to(dev)
        ranks_dev = ranks.to(torch.int32).to(dev)
        image_nb = torch.empty((N, M, 5), dtype=torch.int64, device=dev)
        tile_nb = torch.empty((T, M, 5), dtype=torch.int32, device=dev)
        ws = torch.empty(l.cgic_rate_curve_tiles_workspace_bytes(T, M, 1), dtype=torch.uint8, device=dev)
        fptrs = [_lib.ptr(b) for b in bufs]

        def feat_launch():
            _lib.call("cgic_rate_curve_tiles", tab, *fptrs, count, desc, _lib.ptr(desc_dev), T, N, coarse, _lib.ptr(ranks_dev), S, M,
                      _lib.ptr(image_nb), _lib.ptr(tile_nb), _lib.ptr(ws), stream)

        def feat_full():
            feat_launch()
            return image_nb.cpu()

        exact = torch.equal(base_full(), feat_full()) and torch.equal(feat_full(), curve.nbytes)
        res = {"exact": exact, "tiles": T}
        variants = {"baseline_device_us": (base_launch, True), "feature_device_us": (feat_launch, True),
                    "baseline_to_host_us": (base_full, False), "feature_to_host_us": (feat_full, False)}
        times = {k: [] for k in variants}
        for fn, _ in variants.values():
            for _ in range(a.warmup):
                fn()
        torch.cuda.synchronize()
        for _ in range(a.rounds):
            for name, (fn, events) in variants.items():
                iters = a.iters if events else max(a.iters // 5, 3)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                w0 = time.perf_counter()
                e0.record()
                for _ in range(iters):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                wall = (time.perf_counter() - w0) * 1e6 / iters
                times[name].append(e0.elapsed_time(e1) * 1000.0 / iters if events else wall)
        for name, v in times.items():
            res[name] = round(sorted(v)[len(v) // 2], 1)
            res[name.replace("_us", "_spread_us")] = [round(min(v), 1), round(max(v), 1)]
        res["feature_over_baseline_device"] = round(res["feature_device_us"] / res["baseline_device_us"], 3)
        res["feature_over_baseline_to_host"] = round(res["feature_to_host_us"] / res["baseline_to_host_us"], 3)
        out[f"N{N}"] = res

    # ---- the price of hitting the target in one pass: compress_tiled_to_bpp against one compress_tiled_batch at a fixed ratio
    torch.manual_seed(0)
    model = _StandIn().to(dev).eval()
    with torch.no_grad():
        model.quantize.embedding.weight.normal_()
        model.quantize.usage_counter.copy_(torch.from_numpy(np.floor(1e6 / (1 + np.arange(1024)) ** 1.1).astype(np.float32)))
    cg.install(model)
    x = torch.from_numpy((rng.integers(0, 256, (1, 3, H, W)) / 255.0).astype(np.float32)).to(dev)

    def encode(tiles):
        _, _, _, mask, ind, _, mode = model.encode(tiles)
        return ind, mask, mode

    def plain():
        p = model.encoder.router_config["params"]
        p["per_image"] = True
        try:
            return highres.compress_tiled_batch(x, encode, model._cgic_codec)
        finally:
            p["per_image"] = False

    with torch.no_grad():
        _, _, _, full = model.compress_tiled_to_bpp(x, 1e9)
        target = float(full.batch_bpp.median())
        for name, fn in (("compress_tiled_fixed_ratio_ms", plain), ("compress_tiled_to_bpp_ms", lambda: model.compress_tiled_to_bpp(x, target))):
            for _ in range(2):
                fn()
            v = []
            for _ in range(a.rounds):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                v.append((time.perf_counter() - t0) * 1e3)
            out[name] = round(sorted(v)[len(v) // 2], 2)
            out[name.replace("_ms", "_spread_ms")] = [round(min(v), 2), round(max(v), 2)]
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
    ap.add_argument("--tiled", action="store_true", help="cgic_rate_curve_tiles against one cgic_rate_curve per shape group + host fold")
    ap.add_argument("--device", action="store_true", help="route_to_bpp (the rate pick on the device) against rate_curve -> choose -> router -> gather")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    if a.tiled:
        return tiled_bench(a, dev)
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
        if a.device:
            e8r, e16r = cg.entropy_maps(x, reference_order=True)
            inds = cg.grain_indices(vq, *heads, quant_conv=qc)
            return device_bench(a, dev, codec, inds, e16r.detach().clone(), e8r.detach().clone())

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
