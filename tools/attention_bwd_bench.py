#!/usr/bin/env python3
"""Time forward + backward of AttnBlock's attention on the library's kernels (torch.ops.cgic.attention_train: csrc/cgic_attn.hip with
its lse, then csrc/cgic_attn_bwd.hip) against the module's torch path, and record the peak memory of both.

    python tools/attention_bwd_bench.py [--calls 100] [--rounds 7] [--limit 600] [--only SUBSTRING]
    python tools/attention_bwd_bench.py --resources      # no GPU: registers / LDS / scratch / occupancy of every instantiation

A step is one [B, C, N]: the training shape [8,512,1024] (attn_resolutions: 32 of config_train.yaml), [2,512,4096], and the 36 864
tokens of a 768x768 tile, [1,512,36864].  Within a step, for fp32, fp16 and bf16 q, k, v (the half types as the 1x1 convs hand them
on under torch.autocast), all three wanting a gradient, with a given gradient of the result:
  (t) the module's torch path -- what it runs without the flag: bmm, scale, softmax in fp32, bmm, torch's autograd;
  (k) torch.ops.cgic.attention_train and its backward.
The two run in ONE process and alternate round by round; a round is HIP events around `calls` calls of forward + backward (100 by
default: a window of 0.1 to 1.7 s of the kernels, 0.03 to 0.2 s of torch's path; 4 calls and 5 rounds where B * N * N * C is beyond
2e11, where one call of the kernels is 0.13 to 0.8 s).  Per route: the median, the lowest and the highest
round (ms per call) and the peak of torch.cuda.max_memory_allocated over one call, above what was allocated before it (MiB).
`t_over_k`: time ratio; `mem_t_over_k`: peak-memory ratio.  Where torch's path does not fit the device, its entry says so and the
kernels are measured alone.  One JSON line per step and type.

Without --step this is the driver: every step runs in a fresh child process under its own `timeout -k 10 <--limit>`, and the driver
stops at the first step that does not exit 0 (nothing more is started on a device that a step left in doubt)."""
import argparse
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = ((8, 512, 1024), (2, 512, 4096), (1, 512, 36864))


def resources():
    """compile csrc/cgic_attn_bwd.hip with -Rpass-analysis=kernel-resource-usage and print one JSON line per kernel instantiation"""
    csrc = os.path.join(ROOT, "control-gic_amd", "csrc")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    out = subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-fast-math",
                          "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(csrc, "cgic_attn_bwd.hip"), "-o", os.devnull],
                         capture_output=True, text=True)
    if out.returncode:
        sys.stderr.write(out.stderr)
        return out.returncode
    row = None
    for line in out.stderr.splitlines():
        m = re.search(r"remark:\s+(.*?)\s+\[-Rpass", line)
        if not m:
            continue
        text = m.group(1)
        if text.startswith("Function Name:"):
            if row:
                print(json.dumps(row))
            name = text.split(":", 1)[1].strip()
            t = re.search(r"attn_bwd_(\w+?)_kernelINS0_\d(\w+?)E(?:Li(\d+)ELb(\d)E)?", name)
            row = {"kernel": (f"{t.group(1)} {t.group(2)}" + (f" C{t.group(3)} vec={t.group(4)}" if t.group(3) else "")) if t else name}
        elif row is not None and ":" in text:
            key, val = text.split(":", 1)
            if key.strip() in ("VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "SGPRs Spill", "VGPRs Spill"):
                row[key.strip()] = int(val)
    if row:
        print(json.dumps(row))
    # LDS bytes and workspace: asked of the plan itself (csrc/cgic_attn_bwd_plan.h through tests/host/attn_bwd_plan_main.cpp, built
    # with the host compiler), at B = 2, N = 4096 with made-up addresses 64 GiB apart
    import shutil
    import tempfile
    cxx = os.environ.get("CXX") or next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    if cxx is None:
        sys.stderr.write("no host C++ compiler: the plan's LDS bytes are not printed\n")
        return 1
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "attn_bwd_plan_main")
        subprocess.check_call([cxx, "-std=c++17", "-O1", os.path.join(ROOT, "tests", "host", "attn_bwd_plan_main.cpp"), "-o", exe])
        for dt, name in ((0, "fp32"), (1, "fp16"), (2, "bf16")):
            for C in (256, 512):
                n = C * 4096
                line = [dt, dt, 2, C, 4096, n, n, n, n, 1000000 // int(C ** 0.5)] + [(i + 1) << 36 for i in range(10)] + [-1]
                got = subprocess.run([exe] + [str(v) for v in line], capture_output=True, text=True, check=True).stdout
                f = dict(t.split("=", 1) for t in got.split())
                print(json.dumps({"plan": f"{name} C{C} B2 N4096", "dq_lds_bytes": int(f["dq_lds"]), "dkdv_lds_bytes": int(f["dkdv_lds"]),
                                  "workspace_bytes": int(f["workspace"]), "dq_grid": int(f["dq_grid"]), "dkdv_grid": int(f["dkdv_grid"])}))
    return 0


def run_step(B, C, N, opt):
    import torch
    import control_gic_amd  # noqa: F401  (registers torch.ops.cgic)
    dev = torch.device("cuda", 0)
    gen = torch.Generator().manual_seed(1)
    rnd = lambda: torch.randn(B, C, N, generator=gen)
    base32 = [rnd() for _ in range(4)]
    scale = C ** -0.5
    work = B * N * N * C
    calls = 4 if work > 2e11 else opt.calls            # (a timed window is `calls` calls: a second or so of the kernels at every shape)
    rounds = 5 if work > 2e11 else opt.rounds

    def torch_route(go, q, k, v):
        w = torch.bmm(q.permute(0, 2, 1), k)
        w = w * scale
        w = torch.nn.functional.softmax(w.float(), dim=2).to(q.dtype)
        return torch.autograd.grad(torch.bmm(v, w.permute(0, 2, 1)), (q, k, v), go)

    def kernel_route(go, q, k, v):
        return torch.autograd.grad(torch.ops.cgic.attention_train(q, k, v, scale)[0], (q, k, v), go)

    with torch.cuda.device(dev):
        for name, dtype in (("fp32", torch.float32), ("fp16", torch.float16), ("bf16", torch.bfloat16)):
            go, q, k, v = (t.to(dtype).to(dev) for t in base32)
            q, k, v = (t.requires_grad_() for t in (q, k, v))
            routes = {"t": lambda: torch_route(go, q, k, v), "k": lambda: kernel_route(go, q, k, v)}
            row = {"step": f"B{B}-C{C}-N{N}", "dtype": name, "calls": calls, "rounds": rounds}
            peak, first = {}, {}
            for r, fn in list(routes.items()):
                try:
                    for _ in range(2):
                        first[r] = fn()
                    torch.cuda.synchronize()
                    base = torch.cuda.memory_allocated()
                    torch.cuda.reset_peak_memory_stats()
                    fn()
                    torch.cuda.synchronize()
                    peak[r] = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
                except torch.OutOfMemoryError:
                    row[r] = {"does_not_fit": True, "device_MiB": round(torch.cuda.get_device_properties(dev).total_memory / 2 ** 20)}
                    del routes[r]
                    first.pop(r, None)
                    torch.cuda.empty_cache()
            if len(first) == 2:
                row["max_rel_diff_t_k"] = [round(float((a.float() - b.float()).abs().max() / a.float().abs().max()), 6) for a, b in zip(first["t"], first["k"])]
            first.clear()
            ms = {r: [] for r in routes}
            for _ in range(rounds):
                for r, fn in routes.items():
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    for _ in range(calls):
                        fn()
                    b.record()
                    torch.cuda.synchronize()
                    ms[r].append(a.elapsed_time(b) / calls)
            for r in routes:
                vals = sorted(ms[r])
                row[r] = {"ms": round(vals[len(vals) // 2], 4), "min_ms": round(vals[0], 4), "max_ms": round(vals[-1], 4), "peak_MiB": round(peak[r], 2)}
            if len(routes) == 2:
                row["t_over_k"] = round(row["t"]["ms"] / row["k"]["ms"], 3)
                row["mem_t_over_k"] = round(peak["t"] / peak["k"], 3) if peak["k"] else None
            print(json.dumps(row), flush=True)
            del go, q, k, v
            torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--limit", type=int, default=600, help="seconds a step may take (timeout -k 10)")
    ap.add_argument("--only", default="", help="run the steps whose name contains this")
    ap.add_argument("--resources", action="store_true")
    ap.add_argument("--step", type=int, nargs=3, default=None, help="(internal) B C N: run this one step in this process")
    opt = ap.parse_args()
    if opt.resources:
        return resources()
    if opt.step is not None:
        run_step(*opt.step, opt)
        return 0
    for B, C, N in SHAPES:
        if opt.only not in f"B{B}-C{C}-N{N}":
            continue
        cmd = ["timeout", "-k", "10", str(opt.limit), sys.executable, os.path.abspath(__file__), "--step", str(B), str(C), str(N),
               "--calls", str(opt.calls), "--rounds", str(opt.rounds)]
        rc = subprocess.run(cmd).returncode
        if rc != 0:
            print(json.dumps({"step": f"B{B}-C{C}-N{N}", "exit": rc, "stopped": "no further step is started"}), flush=True)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
