#!/usr/bin/env python3
"""Time the fused SpatialNorm (csrc/cgic_norm.hip) against the torch expression it replaces, at the decoder's shapes.

    python tools/spatial_norm_bench.py [--B 64 1] [--calls 20] [--rounds 7] [--limit 300] [--only SUBSTRING]

A step is one (B, C, H) of the decoder of config_inference.yaml: 512x16^2, 512x32^2, 512x64^2, 256x128^2, 128x256^2, zq at 64x64.
Within a step, for fp32 features, and for fp16 features under torch.autocast with the fp32 and with the half result, each with and
without the swish that ResnetBlock puts behind the layer:
  (t) torch: interpolate, GroupNorm, the two 1x1 convs, the multiply, the add (decoder.py:46-53), `x * sigmoid(x)` for the swish
      and `.to(half)` where the half result is wanted;
  (k) control_gic_amd.norm.spatial_norm: one launch, or two where the plan says so (reported as `one_launch`).
The two run in ONE process and alternate round by round; a round is HIP events around --calls calls.  Per route: the median, the
lowest and the highest round (ms per call); for (k) also the bytes counted from the shapes (the features read once or twice, the
result written once) and TB/s = counted bytes / median.  `k_within_bar`: (k) takes no longer than (t) beyond the run-to-run spread
of (t), the range over its rounds.  One JSON line per step and variant.

Without --step this is the driver: every step runs in a fresh child process under its own `timeout -k 10 <--limit>`, and the driver
stops at the first step that does not exit 0 (nothing more is started on a device that a step left in doubt)."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = ((512, 16), (512, 32), (512, 64), (256, 128), (128, 256))
HQ = 64


def run_step(B, C, H, opt):
    import torch
    import torch.nn.functional as F
    from control_gic_amd import norm
    dev = torch.device("cuda", 0)
    gen = torch.Generator().manual_seed(1)
    rnd = lambda *s: torch.randn(*s, generator=gen).to(dev)
    f32 = rnd(B, C, H, H)
    zq = rnd(B, 4, HQ, HQ)
    gn_w, gn_b, wy, by, wb, bb = 1 + 0.1 * rnd(C), 0.1 * rnd(C), 0.5 * rnd(C, 4, 1, 1), 1 + 0.1 * rnd(C), 0.5 * rnd(C, 4, 1, 1), 0.1 * rnd(C)
    half = torch.float16

    def torch_route(f, swish, res):
        z = F.interpolate(zq, size=f.shape[-2:], mode="nearest")
        v = F.group_norm(f, 32, gn_w, gn_b, 1e-6) * F.conv2d(z, wy, by) + F.conv2d(z, wb, bb)
        if swish:
            v = v * torch.sigmoid(v)
        return v if res is None else v.to(res)

    def kernel_route(f, swish, res):
        return norm.spatial_norm(f, zq, gn_w, gn_b, wy, by, wb, bb, swish=swish, out_dtype=res)

    variants = [("fp32", f32, None, False), ("autocast-fp16-to-fp32", f32.to(half), None, True), ("autocast-fp16-to-fp16", f32.to(half), half, True)]
    with torch.cuda.device(dev), torch.no_grad():
        for name, f, res, autocast in variants:
            for swish in (False, True):
                ctx = lambda: torch.autocast("cuda", dtype=half, enabled=autocast)
                routes = {"t": lambda: torch_route(f, swish, res), "k": lambda: kernel_route(f, swish, res)}
                with ctx():
                    t, k = routes["t"]().float(), routes["k"]().float()
                    diff = float((t - k).abs().max())
                    for fn in routes.values():
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
                one = norm.one_launch(f.dtype, B, C, H, H)
                n = f.numel()
                nbytes = n * (f.element_size() * (1 if one else 2) + (4 if res is None else 2))
                row = {"step": f"B{B}-C{C}-{H}x{H}", "variant": name, "swish": swish, "one_launch": one, "calls": opt.calls, "rounds": opt.rounds,
                       "max_abs_diff_t_k": diff}
                for r in routes:
                    v = sorted(ms[r])
                    row[r] = {"ms": round(v[len(v) // 2], 5), "min_ms": round(v[0], 5), "max_ms": round(v[-1], 5)}
                row["k"]["bytes"] = nbytes
                row["k"]["TB_per_s"] = round(nbytes / row["k"]["ms"] / 1e9, 3)
                row["t_over_k"] = round(row["t"]["ms"] / row["k"]["ms"], 3)
                row["k_within_bar"] = bool(row["k"]["ms"] <= row["t"]["ms"] + (row["t"]["max_ms"] - row["t"]["min_ms"]))
                print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, nargs="+", default=(64, 1))
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--limit", type=int, default=300, help="seconds a step may take (timeout -k 10)")
    ap.add_argument("--only", default="", help="run the steps whose name contains this")
    ap.add_argument("--step", type=int, nargs=3, default=None, help="(internal) B C H: run this one step in this process")
    opt = ap.parse_args()
    if opt.step is not None:
        run_step(*opt.step, opt)
        return 0
    for B in opt.B:
        for C, H in SHAPES:
            if opt.only not in f"B{B}-C{C}-{H}x{H}":
                continue
            cmd = ["timeout", "-k", "10", str(opt.limit), sys.executable, os.path.abspath(__file__), "--step", str(B), str(C), str(H),
                   "--calls", str(opt.calls), "--rounds", str(opt.rounds)]
            rc = subprocess.run(cmd).returncode
            if rc != 0:
                print(json.dumps({"step": f"B{B}-C{C}-{H}x{H}", "exit": rc, "stopped": "no further step is started"}), flush=True)
                return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
