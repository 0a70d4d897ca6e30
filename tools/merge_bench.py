#!/usr/bin/env python3
"""Time the merge, the pools and the blends on half-precision features: the half kernels (ABI 16) against the route they replace.

    python tools/merge_bench.py [--B 16] [--C 512] [--hw 64 64] [--calls 50] [--rounds 5] [--limit 300] [--only SUBSTRING]

For each of the four operations (grain merge and fine blend on the fine grid --hw, medium blend and both pools on its half), in
bf16 and fp16, with the fp32 and with the half result:
  (a) the route before ABI 16, written out here: `.float()` of every feature, the _f32 entry point, `.to(half)` where a half
      result is wanted;
  (b) the half call (control_gic_amd.merge.*: one launch, no cast);
  (k) the _f32 call alone on features that are fp32 already (the same kernel family on fp32 elements, at the same shape).
The three run in ONE process and alternate round by round; a round is HIP events around --calls calls -- issued from Python (`ms`),
and again as one captured graph of the same calls per route (`graph_ms`: no host work between the launches; the same buffers every
call, so a tensor set that fits the last-level cache is read from there).  Per route: the median, the lowest and the highest
round (ms per call), the bytes counted from the shapes (every tensor read or written once per pass, masks included) and TB/s =
counted bytes / median.  One JSON line per step.

Without --step this is the driver: every step runs in a fresh child process under its own `timeout -k 10 <--limit>`, and the driver
stops at the first step that does not exit 0 (nothing more is started on a device that a step left in doubt)."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

OPS = ("grain_merge", "blend_fine", "blend_medium", "avg_pool2", "avg_pool4")
STEPS = [f"{op}:{dt}:{out}" for op in OPS for dt in ("bf16", "fp16") for out in ("fp32", "half")]


def counted_bytes(op, B, C, h, w, out_bytes, route):
    """bytes moved, every tensor once per pass.  (h, w): the grid of the call (the pools: of the input)"""
    n, m = B * C * h * w, B * h * w
    if op == "grain_merge":
        feats, masks, out = n + n // 4 + n // 16, 4 * (m + m // 4 + m // 16), n
    elif op == "blend_fine":
        feats, masks, out = 2 * n, 4 * (m + m // 4 + m // 16), n
    elif op == "blend_medium":
        feats, masks, out = 2 * n, 4 * (m + m // 4), n
    else:
        k = int(op[-1])
        feats, masks, out = n, 0, n // (k * k)
    if route == "b":                                    # halves in, the result out
        return 2 * feats + masks + out_bytes * out
    if route == "k":                                    # the fp32 kernel alone
        return 4 * feats + masks + 4 * out
    cast_in = (2 + 4) * feats                           # (a): .float() reads 2 and writes 4 per element, the kernel reads the 4 again
    cast_out = (4 + 2) * out if out_bytes == 2 else 0
    return cast_in + 4 * feats + masks + 4 * out + cast_out


def run_step(step, opt):
    import torch
    from control_gic_amd import _lib, merge
    op, dt_name, out_name = step.split(":")
    half = torch.bfloat16 if dt_name == "bf16" else torch.float16
    res = half if out_name == "half" else torch.float32
    dev = torch.device("cuda", 0)
    B, C = opt.B, opt.C
    h, w = opt.hw if op in ("grain_merge", "blend_fine") else (opt.hw[0] // 2, opt.hw[1] // 2)
    gen = torch.Generator().manual_seed(1)
    rnd = lambda *s: torch.randn(*s, generator=gen).to(half).to(dev)
    fh, fw = (h, w) if op in ("grain_merge", "blend_fine") else (2 * h, 2 * w)                 # the fine grid the masks belong to
    mk = [(torch.rand(B, 1, fh // s, fw // s, generator=gen) < 0.5).to(torch.int32).to(dev) for s in (4, 2, 1)]
    stream = lambda: _lib.current_stream(dev)
    p = _lib.ptr

    def f32_call(name, feats, *mid):
        out = torch.empty_like(feats[-1] if name != "cgic_avgpool_f32" else feats[0], dtype=torch.float32) if name != "cgic_avgpool_f32" else None
        return out

    if op == "grain_merge":
        feats = [rnd(B, C, h // 4, w // 4), rnd(B, C, h // 2, w // 2), rnd(B, C, h, w)]

        def kernel32(f):
            out = torch.empty_like(f[2])
            _lib.call("cgic_grain_merge_f32", p(f[0]), p(f[1]), p(f[2]), p(mk[0]), p(mk[1]), p(mk[2]), B, C, h, w, p(out), stream())
            return out
        new = lambda: merge.grain_merge(*feats, *mk, out_dtype=res)
    elif op == "blend_fine":
        feats = [rnd(B, C, h, w), rnd(B, C, h, w)]

        def kernel32(f):
            out = torch.empty_like(f[0])
            _lib.call("cgic_decoder_blend_fine_f32", p(f[0]), p(f[1]), p(mk[0]), p(mk[1]), p(mk[2]), B, C, h, w, p(out), stream())
            return out
        new = lambda: merge.decoder_blend_fine(*feats, *mk, out_dtype=res)
    elif op == "blend_medium":
        feats = [rnd(B, C, h, w), rnd(B, C, h, w)]

        def kernel32(f):
            out = torch.empty_like(f[0])
            _lib.call("cgic_decoder_blend_medium_f32", p(f[0]), p(f[1]), p(mk[0]), p(mk[1]), B, C, h, w, p(out), stream())
            return out
        new = lambda: merge.decoder_blend_medium(*feats, mk[0], mk[1], "shapes", out_dtype=res)
    else:
        k = int(op[-1])
        feats = [rnd(B, C, h, w)]

        def kernel32(f):
            out = torch.empty(B, C, h // k, w // k, device=dev)
            _lib.call("cgic_avgpool_f32", p(f[0]), B * C, h, w, k, p(out), stream())
            return out
        new = lambda: merge.avg_pool(feats[0], k, out_dtype=res)

    feats32 = [f.float() for f in feats]

    def old():
        out = kernel32([f.float() for f in feats])
        return out.to(half) if res == half else out

    routes = {"a": old, "b": new, "k": lambda: kernel32(feats32)}
    with torch.cuda.device(dev):
        same = torch.equal(old().view(torch.int16 if res == half else torch.int32), new().view(torch.int16 if res == half else torch.int32))
        for fn in routes.values():                      # warm up every route
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        ms = {r: [] for r in routes}
        for _ in range(opt.rounds):
            for r, fn in routes.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(opt.calls):
                    fn()
                b.record()
                torch.cuda.synchronize()
                ms[r].append(a.elapsed_time(b) / opt.calls)
        # the same calls captured into one graph per route: no host work between the launches (a call of a few microseconds is
        # otherwise timed by how fast Python issues it), replayed alternately
        graphs = {}
        for r, fn in routes.items():
            graphs[r] = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graphs[r]):
                for _ in range(opt.calls):
                    fn()
            graphs[r].replay()
        torch.cuda.synchronize()
        gms = {r: [] for r in routes}
        for _ in range(opt.rounds):
            for r, g in graphs.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                g.replay()
                b.record()
                torch.cuda.synchronize()
                gms[r].append(a.elapsed_time(b) / opt.calls)
    row = {"step": step, "shape": [B, C, h, w], "calls": opt.calls, "rounds": opt.rounds, "equal_bits_a_b": bool(same)}
    for r in routes:
        v, g = sorted(ms[r]), sorted(gms[r])
        med, gmed = v[len(v) // 2], g[len(g) // 2]
        nbytes = counted_bytes(op, B, C, h, w, 2 if res == half else 4, r)
        row[r] = {"ms": round(med, 5), "min_ms": round(v[0], 5), "max_ms": round(v[-1], 5), "graph_ms": round(gmed, 5), "graph_min_ms": round(g[0], 5),
                  "graph_max_ms": round(g[-1], 5), "bytes": nbytes, "TB_per_s": round(nbytes / med / 1e9, 3), "graph_TB_per_s": round(nbytes / gmed / 1e9, 3)}
    row["a_over_b"] = round(row["a"]["ms"] / row["b"]["ms"], 3)
    row["graph_a_over_b"] = round(row["a"]["graph_ms"] / row["b"]["graph_ms"], 3)
    # the bar: (b) takes no longer than (a) beyond the run-to-run spread of (a), the range over its rounds
    row["b_within_bar"] = bool(row["b"]["ms"] <= row["a"]["ms"] + (row["a"]["max_ms"] - row["a"]["min_ms"]))
    row["graph_b_within_bar"] = bool(row["b"]["graph_ms"] <= row["a"]["graph_ms"] + (row["a"]["graph_max_ms"] - row["a"]["graph_min_ms"]))
    print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=16)
    ap.add_argument("--C", type=int, default=512)
    ap.add_argument("--hw", type=int, nargs=2, default=(64, 64), help="the fine grid; the medium blend and the pools run on its half")
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--limit", type=int, default=300, help="seconds a step may take (timeout -k 10)")
    ap.add_argument("--only", default="", help="run the steps whose name contains this")
    ap.add_argument("--step", default=None, help="(internal) run this one step in this process")
    opt = ap.parse_args()
    if opt.step is not None:
        run_step(opt.step, opt)
        return 0
    for step in STEPS:
        if opt.only not in step:
            continue
        cmd = ["timeout", "-k", "10", str(opt.limit), sys.executable, os.path.abspath(__file__), "--step", step, "--B", str(opt.B), "--C", str(opt.C),
               "--hw", str(opt.hw[0]), str(opt.hw[1]), "--calls", str(opt.calls), "--rounds", str(opt.rounds)]
        rc = subprocess.run(cmd).returncode
        if rc != 0:
            print(json.dumps({"step": step, "exit": rc, "stopped": "no further step is started"}), flush=True)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
