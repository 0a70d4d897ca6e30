#!/usr/bin/env python3
"""Time GroupNorm + swish on the library's kernels (control_gic_amd.norm.GroupNorm: csrc/cgic_norm.hip without zq) against the same
module's torch path, forward alone and forward + backward, at the encoder's shapes.

    python tools/group_norm_bench.py [--B 8 1] [--calls 10] [--rounds 7] [--limit 300] [--only SUBSTRING]

A step is one (B, C, H) of the encoder of config_inference.yaml (ch 128, ch_mult 1,2,2,4,4 at 256x256: the five levels below).
Within a step, for fp32 features and for fp16 features under torch.autocast, with the swish that ResnetBlock puts behind the
norm, for ONE layer and for a STACK of eight layers (each on the output of the one before, every layer with its own parameters):
  fwd      under no_grad;
  fwd+bwd  the features and every parameter want a gradient (k: GroupNorm.backward_kernel = True).
  (t) the module's torch path: F.group_norm, x * sigmoid(x) and, under autocast, the cast to the half type that autocast puts in
      front of the following conv (group_norm is on autocast's fp32 list, so the two results before it are fp32);
  (k) the kernels, which under autocast hand on the half type directly (what resblock.ResnetBlock asks for).
The two run in ONE process and alternate round by round; a round is HIP events around --calls calls.  Per route: the median, the
lowest and the highest round (ms per call) and the peak of torch.cuda.max_memory_allocated over one call, above what was allocated
before it (MiB).  `t_over_k`: time ratio; `mem_t_over_k`: peak-memory ratio.  `GBps_k`: the bytes the kernels must move -- fwd: the
features read twice (one launch: once) and written once -- over the median time: an end-to-end rate of the call, not a kernel's share
of peak.  One JSON line per step, variant, mode and depth.

Without --step this is the driver: every step runs in a fresh child process under its own `timeout -k 10 <--limit>`, and the driver
stops at the first step that does not exit 0 (nothing more is started on a device that a step left in doubt)."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = ((128, 256), (256, 128), (256, 64), (512, 32), (512, 16))
DEPTHS = (1, 8)


def run_step(B, C, H, opt):
    import torch
    import torch.nn.functional as F
    from control_gic_amd import norm
    dev = torch.device("cuda", 0)
    gen = torch.Generator().manual_seed(1)
    rnd = lambda *s: torch.randn(*s, generator=gen).to(dev)
    half = torch.float16
    torch.manual_seed(2)
    layers = [norm.GroupNorm(32, C, eps=1e-6).to(dev) for _ in range(max(DEPTHS))]
    with torch.no_grad():
        for m in layers:
            m.weight.add_(0.1 * torch.randn_like(m.weight))
            m.bias.add_(0.1 * torch.randn_like(m.bias))
            m.backward_kernel = True
    f32 = rnd(B, C, H, H)
    go32 = rnd(B, C, H, H)

    def torch_path(m, h, res):
        v = F.group_norm(h, m.num_groups, m.weight, m.bias, m.eps)
        v = v * torch.sigmoid(v)
        return v if res is None else v.to(res)

    def forward(route, depth, f, res):
        h = f
        for m in layers[:depth]:
            h = m(h, swish=True, out_dtype=res) if route == "k" else torch_path(m, h, res)
        return h

    def both(route, depth, f, go, res):
        forward(route, depth, f, res).backward(go)
        g = f.grad
        f.grad = None
        return g

    with torch.cuda.device(dev):
        for name, dtype, autocast in (("fp32", torch.float32, False), ("autocast-fp16", half, True)):
            res = half if autocast else None
            go = go32.to(dtype)
            for mode in ("fwd", "fwd+bwd"):
                f = f32.to(dtype).clone().requires_grad_(mode == "fwd+bwd")
                for depth in DEPTHS:
                    with torch.autocast("cuda", dtype=half, enabled=autocast), torch.set_grad_enabled(mode == "fwd+bwd"):
                        assert layers[0]._route(f) == ("train" if mode == "fwd+bwd" else "kernel")
                        if mode == "fwd":
                            routes = {r: (lambda r=r: forward(r, depth, f, res)) for r in ("t", "k")}
                        else:
                            routes = {r: (lambda r=r: both(r, depth, f, go, res)) for r in ("t", "k")}
                        vt, vk = routes["t"]().float(), routes["k"]().float()
                        diff = float((vt - vk).abs().max() / vt.abs().max())
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
                    row = {"step": f"B{B}-C{C}-{H}x{H}", "variant": name, "mode": mode, "layers": depth, "calls": opt.calls, "rounds": opt.rounds,
                           "one_launch": norm.one_launch(dtype, B, C, H, H), "max_rel_diff_t_k": diff}
                    for r in routes:
                        v = sorted(ms[r])
                        row[r] = {"ms": round(v[len(v) // 2], 5), "min_ms": round(v[0], 5), "max_ms": round(v[-1], 5), "peak_MiB": round(peak[r], 2)}
                    row["t_over_k"] = round(row["t"]["ms"] / row["k"]["ms"], 3)
                    row["mem_t_over_k"] = round(peak["t"] / peak["k"], 3) if peak["k"] else None
                    if mode == "fwd":
                        eb, ob = f.element_size(), (2 if autocast else 4)
                        moved = depth * f.numel() * ((1 if row["one_launch"] else 2) * eb + ob)
                        row["GBps_k"] = round(moved / (row["k"]["ms"] * 1e-3) / 1e9, 1)
                    print(json.dumps(row), flush=True)
                for m in layers:
                    m.zero_grad(set_to_none=True)


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
