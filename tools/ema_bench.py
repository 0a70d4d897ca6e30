#!/usr/bin/env python3
"""Time the EMA update of the model's parameters after an optimiser step -- the five LitEma modules of CGIC.on_train_batch_end
(CGIC/models/model.py:147-153) -- on the 655 trainable tensors of the training config (tests/golden/ema.npz: 204 of the encoder, 446
of the decoder, the codebook and the two 1x1 convolutions; 130.36 M fp32 elements), three ways in ONE process:

  (a) loop     the reference's per-tensor torch loop restated (the expression of tests/ema_ref.py): per module the `num_updates >= 0` read on
               the host, then shadow.sub_(one_minus_decay * (shadow - param)) tensor by tensor;
  (b) foreach  the same arithmetic with torch._foreach_sub / _foreach_mul / _foreach_sub_ per module, one_minus_decay kept on the
               device (no host read);
  (c) kernel   control_gic_amd.LitEma: per module a one-thread launch and one launch over all tensors (csrc/cgic_ema.hip).

    python tools/ema_bench.py [--calls 10] [--rounds 9] [--warmup 3]
    python tools/ema_bench.py --route a|b|c --calls 3 --rounds 1          # one route alone, for rocprofv3 --kernel-trace --stats
    python tools/ema_bench.py --copies loop|kernel --calls 3              # store, restore and copy_to of one implementation alone, likewise

A STEP is the update of all five modules.  The routes alternate round by round; a round is HIP events around --calls steps (the time
the device needs from the first launch to the last, host gaps included) and a host clock around the same steps ending in a
synchronise.  Per route: median, lowest and highest round in ms per step, the peak of torch.cuda.max_memory_allocated over one step
above what was allocated before it (MiB; for store with nothing kept from an earlier store), and `GBps`: the 12 bytes per element an update must move (two reads, one write) over the
median -- an end-to-end rate of the step, not a kernel's share of peak.  The same for copy_to, store and restore (8 bytes per
element) of the reference's methods and of LitEma's.  All routes are checked to leave the same bits before anything is timed.
One JSON line per measurement."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--route", default=None, choices=["a", "b", "c"])
    ap.add_argument("--copies", default=None, choices=["loop", "kernel"])
    opt = ap.parse_args()

    import numpy as np
    import torch
    import control_gic_amd as cg

    if not torch.cuda.is_available():
        raise SystemExit("ema_bench: no HIP device (a timing needs one; there is no fallback)")
    dev = torch.device("cuda", 0)
    golden = np.load(os.path.join(ROOT, "tests", "golden", "ema.npz"))
    shapes = [tuple(int(v) for v in row if v >= 0) for row in golden["model/shape"]]
    owner = [int(o) for o in golden["model/owner"]]
    parts = [str(p) for p in golden["model/parts"]]
    elements = int(golden["model/numel"].sum())

    class Holder(torch.nn.Module):
        def __init__(self, shapes, seed):
            super().__init__()
            g = torch.Generator().manual_seed(seed)
            self.p = torch.nn.ParameterList([torch.nn.Parameter(torch.randn(s, generator=g) * 0.05) for s in shapes])

    with torch.cuda.device(dev):
        # everything is made on the host and moved once: the only kernels a trace of this program shows are the routes' own
        models = [Holder([s for s, o in zip(shapes, owner) if o == i], 100 + i) for i in range(len(parts))]
        emas = {r: [cg.LitEma(m, 0.9999) for m in models] for r in "abc"}                  # (one set of shadows per route)
        with torch.no_grad():
            for m in models:                                                                # the optimiser's step: params != shadows
                for p in m.parameters():
                    p.add_(torch.randn_like(p) * 0.01)
        models = [m.to(dev) for m in models]
        emas = {r: [e.to(dev) for e in es] for r, es in emas.items()}
        omd_host = 1.0 - float(emas["b"][0].decay.cpu().numpy().astype(np.float32))

        def pairs(e, m):
            named = dict(m.named_parameters())
            return [e._buffers[e.m_name2s_name[k]] for k in named if named[k].requires_grad], [p for p in named.values() if p.requires_grad]

        foreach_lists = [pairs(e, m) for e, m in zip(emas["b"], models)]
        foreach_tensor_scalar = [True]

        @torch.no_grad()
        def step_a():
            # what the reference's forward costs: a read of the counter on the host, two dicts built per call, three torch
            # operations per tensor
            for e, m in zip(emas["a"], models):
                decay = e.decay
                if bool(e.num_updates >= 0):                                                # (the host read; ema.py:28)
                    e.num_updates.add_(1)
                    warm = (e.num_updates + 1) / (e.num_updates + 10)
                    decay = warm if bool(warm < decay) else decay
                omd = 1.0 - decay
                params, shadows = dict(m.named_parameters()), dict(e.named_buffers())
                for key, p in params.items():
                    if p.requires_grad:
                        s = shadows[e.m_name2s_name[key]]
                        s.sub_(omd * (s - p))

        @torch.no_grad()
        def step_b():
            for e, (s, p) in zip(emas["b"], foreach_lists):
                d = torch._foreach_sub(s, p)
                if foreach_tensor_scalar[0]:
                    try:
                        torch._foreach_mul_(d, 1.0 - e.decay)
                    except (TypeError, RuntimeError):
                        foreach_tensor_scalar[0] = False                                    # (no Tensor overload: the host's float)
                if not foreach_tensor_scalar[0]:
                    torch._foreach_mul_(d, omd_host)
                torch._foreach_sub_(s, d)

        def step_c():
            for e, m in zip(emas["c"], models):
                e(m)

        steps = {"a": step_a, "b": step_b, "c": step_c}
        names = {"a": "loop", "b": "foreach", "c": "kernel"}
        routes = [] if opt.copies else [opt.route] if opt.route else ["a", "b", "c"]

        def shadows_of(r):
            return [b for e in emas[r] for k, b in e._buffers.items() if k not in ("decay", "num_updates")]

        # ---- the same bits, before anything is timed
        for r in routes:
            steps[r]()
        torch.cuda.synchronize()
        if not opt.route and not opt.copies:
            base = shadows_of("a")
            for r in "bc":
                same = all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(base, shadows_of(r)))
                print(json.dumps({"check": f"{names[r]} == loop, bit for bit, {len(base)} tensors", "ok": bool(same)}), flush=True)
                if not same:
                    raise SystemExit("ema_bench: the routes disagree")

        # ---- copy_to / store / restore: the reference's methods (ema.py:46-76) against LitEma's
        @torch.no_grad()
        def ref_copy_to():                                                              # one copy_ per tensor
            for e, m in zip(emas["a"], models):
                shadows = dict(e.named_buffers())
                for key, p in dict(m.named_parameters()).items():
                    if p.requires_grad:
                        p.data.copy_(shadows[e.m_name2s_name[key]])

        kept = {}

        @torch.no_grad()
        def ref_store():                                                                # one clone per tensor
            for i, m in enumerate(models):
                kept[i] = [p.clone() for p in m.parameters()]

        @torch.no_grad()
        def ref_restore():                                                              # one copy_ per tensor
            for i, m in enumerate(models):
                for p, c in zip(m.parameters(), kept[i]):
                    p.data.copy_(c)

        def k_store():
            for e, m in zip(emas["c"], models):
                e.store(m.parameters())

        def k_restore():
            for e, m in zip(emas["c"], models):
                e.restore(m.parameters())

        def k_copy_to():
            for e, m in zip(emas["c"], models):
                e.copy_to(m)

        def forget():
            """nothing kept from an earlier store: the peak of the next one counts its whole copy"""
            kept.clear()
            for e in emas["c"]:
                e._stash, e.collected_params = None, []

        if opt.copies:
            # one implementation of the three copies alone, for a kernel trace: --calls of each
            fns = {"loop": (ref_store, ref_restore, ref_copy_to), "kernel": (k_store, k_restore, k_copy_to)}[opt.copies]
            for fn in fns:
                for _ in range(opt.calls):
                    fn()
            torch.cuda.synchronize()
            print(json.dumps({"copies": opt.copies, "calls_of_each": opt.calls, "calls_in_all": 3 * opt.calls}), flush=True)
            return

        def measure(fns, bytes_per_element, what, before_peak=None):
            """fns: {route: callable}; alternating rounds"""
            ev, wall = {r: [] for r in fns}, {r: [] for r in fns}
            for r, fn in fns.items():
                for _ in range(opt.warmup):
                    fn()
            torch.cuda.synchronize()
            for _ in range(opt.rounds):
                for r, fn in fns.items():
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    a.record()
                    for _ in range(opt.calls):
                        fn()
                    b.record()
                    torch.cuda.synchronize()
                    wall[r].append((time.perf_counter() - t0) * 1e3 / opt.calls)
                    ev[r].append(a.elapsed_time(b) / opt.calls)
            out = {}
            for r, fn in fns.items():
                if before_peak is not None:
                    before_peak()
                torch.cuda.synchronize()
                before = torch.cuda.memory_allocated(dev)
                torch.cuda.reset_peak_memory_stats(dev)
                fn()
                torch.cuda.synchronize()
                peak = (torch.cuda.max_memory_allocated(dev) - before) / 2 ** 20
                med = float(np.median(ev[r]))
                out[r] = med
                print(json.dumps({"what": what, "route": names.get(r, r), "ms_per_step": round(med, 4), "lowest": round(min(ev[r]), 4),
                                  "highest": round(max(ev[r]), 4), "host_ms_per_step": round(float(np.median(wall[r])), 4),
                                  "peak_extra_MiB": round(peak, 2), "GBps": round(bytes_per_element * elements / med / 1e6, 1),
                                  "elements": elements, "tensors": len(shapes), "calls": opt.calls, "rounds": opt.rounds}), flush=True)
            return out

        t = measure({r: steps[r] for r in routes}, 12, "update")
        print(json.dumps({"steps_run_per_route": 1 + opt.warmup + opt.calls * opt.rounds + 1, "foreach_mul_by_device_scalar": foreach_tensor_scalar[0]}), flush=True)
        if not opt.route:
            print(json.dumps({"what": "update", "loop_over_kernel": round(t["a"] / t["c"], 2), "foreach_over_kernel": round(t["b"] / t["c"], 2)}), flush=True)

            ref_store(), k_store()
            for what, a, c in (("store", ref_store, k_store), ("restore", ref_restore, k_restore), ("copy_to", ref_copy_to, k_copy_to)):
                t = measure({"loop": a, "kernel": c}, 8, what, before_peak=forget if what == "store" else None)
                if what == "store":
                    ref_store(), k_store()                                                  # (restore needs both kept again)
                print(json.dumps({"what": what, "loop_over_kernel": round(t["loop"] / t["kernel"], 2)}), flush=True)


if __name__ == "__main__":
    main()
