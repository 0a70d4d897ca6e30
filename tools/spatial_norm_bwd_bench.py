#!/usr/bin/env python3
"""Time forward + backward of SpatialNorm on the library's training kernels (SpatialNorm.backward_kernel = True: csrc/cgic_norm.hip, csrc/cgic_norm_bwd.hip,
forward with statistics, then reduce / finish / apply) against the module's torch path, at the decoder's shapes.

    python tools/spatial_norm_bwd_bench.py [--B 8 1] [--calls 10] [--rounds 7] [--limit 300] [--only SUBSTRING]

A step is one (B, C, H) of the decoder of config_inference.yaml (the shape list of tools/spatial_norm_bench.py), zq at 64x64.
Within a step, for fp32 features and for fp16 features under torch.autocast (the half result handed on, as a conv would hand on
half features), with the swish that ResnetBlock puts behind the layer, for ONE layer and for a STACK of eight layers (each on the
output of the one before, every layer with its own parameters, all of which and the features and zq want a gradient):
  (t) the module's torch path -- what it runs without the flag: the reference's expression, torch's autograd;
  (k) the same modules with backward_kernel = True.
The two run in ONE process and alternate round by round; a round is HIP events around --calls calls of forward + backward.  Per
route: the median, the lowest and the highest round (ms per call) and the peak of torch.cuda.max_memory_allocated over one call,
above what was allocated before it (MiB).  `t_over_k`: time ratio; `mem_t_over_k`: peak-memory ratio.  One JSON line per step,
variant and depth.

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
DEPTHS = (1, 8)


def run_step(B, C, H, opt):
    import torch
    from control_gic_amd import norm
    dev = torch.device("cuda", 0)
    gen = torch.Generator().manual_seed(1)
    rnd = lambda *s: torch.randn(*s, generator=gen).to(dev)
    half = torch.float16
    layers = {}
    for route in ("t", "k"):
        torch.manual_seed(2)
        layers[route] = [norm.SpatialNorm(C, 4, num_groups=32, eps=1e-6, affine=True).to(dev) for _ in range(max(DEPTHS))]
        for m in layers[route]:
            m.backward_kernel = route == "k"
    zq = rnd(B, 4, HQ, HQ).requires_grad_()
    f32 = rnd(B, C, H, H)
    go32 = rnd(B, C, H, H)

    def step(route, depth, f, go, res):
        h = f
        for m in layers[route][:depth]:
            h = m(h, zq, swish=True, out_dtype=res)
        h.backward(go)
        g = f.grad
        f.grad = None
        return g

    with torch.cuda.device(dev):
        for name, dtype, autocast in (("fp32", torch.float32, False), ("autocast-fp16", half, True)):
            f = f32.to(dtype).clone().requires_grad_()           # (a leaf of its own: .to() of an equal dtype returns f32 itself)
            res = half if autocast else None
            go = go32.to(dtype)
            for depth in DEPTHS:
                with torch.autocast("cuda", dtype=half, enabled=autocast):
                    assert layers["k"][0].uses_backward_kernel(f, zq) and not layers["t"][0].uses_backward_kernel(f, zq)
                    routes = {r: (lambda r=r: step(r, depth, f, go, res)) for r in ("t", "k")}
                    gt, gk = routes["t"]().float(), routes["k"]().float()
                    diff = float((gt - gk).abs().max() / gt.abs().max())
                    peak = {}
                    for r, fn in routes.items():
                        for _ in range(2):
                            fn()
                        torch.cuda.synchronize()
                        base = torch.cuda.memory_allocated()
                        torch.cuda.reset_peak_memory_stats()
                        fn()
                        torch.cuda.synchronize()
                        peak[r] = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
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
                row = {"step": f"B{B}-C{C}-{H}x{H}", "variant": name, "layers": depth, "calls": opt.calls, "rounds": opt.rounds,
                       "max_rel_diff_df_t_k": diff}
                for r in routes:
                    v = sorted(ms[r])
                    row[r] = {"ms": round(v[len(v) // 2], 5), "min_ms": round(v[0], 5), "max_ms": round(v[-1], 5), "peak_MiB": round(peak[r], 2)}
                row["t_over_k"] = round(row["t"]["ms"] / row["k"]["ms"], 3)
                row["mem_t_over_k"] = round(peak["t"] / peak["k"], 3) if peak["k"] else None
                print(json.dumps(row), flush=True)
            for ms_ in layers.values():
                for m in ms_:
                    m.zero_grad(set_to_none=True)
            zq.grad = None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, nargs="+", default=(8, 1))
    ap.add_argument("--calls", type=int, default=10)
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
