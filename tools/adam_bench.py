#!/usr/bin/env python3
"""Time the optimiser tail of a training step -- clip the gradients by value, step Adam, update the five LitEma modules
(configs/config_train.yaml:7-8, CGIC/models/model.py:192-204 and :147-153) -- on the 655 trainable tensors of the training config
(tests/golden/ema.npz: 130.36 M fp32 elements) with lr 5e-5, betas (0.5, 0.9), clip 1.0 and the EMA on, four ways in ONE process:

  (a) reference   torch.nn.utils.clip_grad_value_, torch.optim.Adam (torch's default path), the reference's per-tensor EMA loop with its
                  `num_updates >= 0` read on the host;
  (b) stock       clip_grad_value_, torch.optim.Adam(fused=True), cg.LitEma: the strongest stock alternative;
  (c) fused       cg.Adam(clip_value=1.0) with the five cg.LitEma attached: clip, step and EMA in one pass (the `ema(model)` calls that
                  follow are made, and find nothing left to do);
  (d) split       cg.Adam(clip_value=1.0) without attachment, then the five cg.LitEma.

    python tools/adam_bench.py [--calls 5] [--rounds 7] [--warmup 2]
    python tools/adam_bench.py --route a|b|c|d --calls 3 --rounds 1          # one route alone, for a kernel trace

A TAIL is one clip + step + EMA of all five modules.  Every route has its own parameters, gradients, state and shadows; the gradients
are fixed tensors (the same addresses every step: cg.Adam then uploads its table of gradient addresses once).  The routes alternate
round by round; a round is HIP events around --calls tails (host gaps included) and a host clock around the same tails ending in a
synchronise.  Per route: median, lowest and highest round in ms per tail, the peak of torch.cuda.max_memory_allocated over one tail above
what was allocated before it, and the host synchronisations torch's sync debug mode reports in one tail.  Then the body kernel alone:
HIP events around 20 back-to-back steps of the plan of (c) (36 B per element) and of (d) (28 B), prologue and launch boundary included,
as TB/s.  One JSON line per measurement."""
import argparse
import json
import os
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--route", default=None, choices=["a", "b", "c", "d"])
    opt = ap.parse_args()

    import numpy as np
    import torch
    import control_gic_amd as cg

    if not torch.cuda.is_available():
        raise SystemExit("adam_bench: no HIP device (a timing needs one; there is no fallback)")
    dev = torch.device("cuda", 0)
    golden = np.load(os.path.join(ROOT, "tests", "golden", "ema.npz"))
    shapes = [tuple(int(v) for v in row if v >= 0) for row in golden["model/shape"]]
    owner = [int(o) for o in golden["model/owner"]]
    parts = [str(p) for p in golden["model/parts"]]
    elements = int(golden["model/numel"].sum())
    LR, BETAS, CLIP = 5e-5, (0.5, 0.9), 1.0

    class Holder(torch.nn.Module):
        def __init__(self, shapes, seed):
            super().__init__()
            g = torch.Generator().manual_seed(seed)
            self.p = torch.nn.ParameterList([torch.nn.Parameter(torch.randn(s, generator=g) * 0.05) for s in shapes])

    routes = [opt.route] if opt.route else ["a", "b", "c", "d"]
    names = {"a": "reference", "b": "stock", "c": "fused", "d": "split"}
    with torch.cuda.device(dev):
        models, emas, opts = {}, {}, {}
        for r in routes:
            ms = [Holder([s for s, o in zip(shapes, owner) if o == i], 100 + i) for i in range(len(parts))]
            es = [cg.LitEma(m, 0.9999, use_num_upates=True) for m in ms]
            models[r], emas[r] = [m.to(dev) for m in ms], [e.to(dev) for e in es]
            g = torch.Generator().manual_seed(7)
            for m in models[r]:
                for p in m.parameters():
                    p.grad = (torch.randn(p.shape, generator=g) * 0.5).to(dev)              # some beyond the clip
            params = [p for m in models[r] for p in m.parameters()]
            if r == "a":
                opts[r] = torch.optim.Adam(params, lr=LR, betas=BETAS)
            elif r == "b":
                opts[r] = torch.optim.Adam(params, lr=LR, betas=BETAS, fused=True)
            else:
                opts[r] = cg.Adam(params, lr=LR, betas=BETAS, clip_value=CLIP)
                if r == "c":
                    for e, m in zip(emas[r], models[r]):
                        opts[r].attach_ema(e, m)

        @torch.no_grad()
        def reference_ema(es, ms):
            for e, m in zip(es, ms):
                decay = e.decay
                if bool(e.num_updates >= 0):                                                # (the host read; ema.py:28)
                    e.num_updates.add_(1)
                    warm = (e.num_updates + 1) / (e.num_updates + 10)
                    decay = warm if bool(warm < decay) else decay
                omd = 1.0 - decay
                shadows = dict(e.named_buffers())
                for key, p in dict(m.named_parameters()).items():
                    if p.requires_grad:
                        s = shadows[e.m_name2s_name[key]]
                        s.sub_(omd * (s - p))

        def tail(r):
            ms, es, o = models[r], emas[r], opts[r]
            if r in "ab":
                torch.nn.utils.clip_grad_value_([p for m in ms for p in m.parameters()], CLIP)
            o.step()
            if r == "a":
                reference_ema(es, ms)
            else:
                for e, m in zip(es, ms):
                    e(m)

        # ---- one tail each, compared before anything is timed
        for r in routes:
            tail(r)
        torch.cuda.synchronize()
        if not opt.route:
            flat = {r: torch.cat([p.detach().reshape(-1) for m in models[r] for p in m.parameters()]) for r in routes}
            shadow = {r: torch.cat([b.reshape(-1) for e in emas[r] for k, b in e._buffers.items() if k not in ("decay", "num_updates")]) for r in routes}
            same = bool(torch.equal(flat["c"].view(torch.int32), flat["d"].view(torch.int32)) and torch.equal(shadow["c"].view(torch.int32), shadow["d"].view(torch.int32)))
            print(json.dumps({"check": "fused == split, bit for bit, parameters and shadows", "ok": same}), flush=True)
            for r in "ab":
                print(json.dumps({"check": f"fused against {names[r]}", "largest_parameter_difference": float((flat["c"] - flat[r]).abs().max()),
                                  "largest_shadow_difference": float((shadow["c"] - shadow[r]).abs().max()), "step_size": LR / (1 - BETAS[0])}), flush=True)
            if not same:
                raise SystemExit("adam_bench: the fused and the split route disagree")
            del flat, shadow

        for r in routes:
            for _ in range(opt.warmup):
                tail(r)
        torch.cuda.synchronize()
        ev, wall = {r: [] for r in routes}, {r: [] for r in routes}
        for _ in range(opt.rounds):
            for r in routes:
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                a.record()
                for _ in range(opt.calls):
                    tail(r)
                b.record()
                torch.cuda.synchronize()
                wall[r].append((time.perf_counter() - t0) * 1e3 / opt.calls)
                ev[r].append(a.elapsed_time(b) / opt.calls)
        med = {}
        for r in routes:
            torch.cuda.synchronize()
            before = torch.cuda.memory_allocated(dev)
            torch.cuda.reset_peak_memory_stats(dev)
            tail(r)
            torch.cuda.synchronize()
            peak = (torch.cuda.max_memory_allocated(dev) - before) / 2 ** 20
            mode = torch.cuda.get_sync_debug_mode()
            with warnings.catch_warnings(record=True) as seen:
                warnings.simplefilter("always")
                torch.cuda.set_sync_debug_mode("warn")
                try:
                    tail(r)
                finally:
                    torch.cuda.set_sync_debug_mode(mode)
            syncs = sum(1 for w in seen if "synchroniz" in str(w.message).lower() and "prototype" not in str(w.message).lower())
            torch.cuda.synchronize()
            med[r] = float(np.median(ev[r]))
            print(json.dumps({"what": "tail", "route": names[r], "ms_per_tail": round(med[r], 4), "lowest": round(min(ev[r]), 4), "highest": round(max(ev[r]), 4),
                              "host_ms_per_tail": round(float(np.median(wall[r])), 4), "peak_extra_MiB": round(peak, 2), "host_synchronisations": syncs,
                              "elements": elements, "tensors": len(shapes), "calls": opt.calls, "rounds": opt.rounds}), flush=True)
        if not opt.route:
            print(json.dumps({"what": "tail", "reference_over_fused": round(med["a"] / med["c"], 2), "stock_over_fused": round(med["b"] / med["c"], 2),
                              "split_over_fused": round(med["d"] / med["c"], 2)}), flush=True)

        # ---- the two launches alone: back-to-back steps of the plans of (c) and (d) on the addresses they already hold
        for r, nbytes in (("c", 36), ("d", 28)):
            if r not in routes:
                continue
            g = opts[r]._groups[0]
            ptrs = [p.grad.data_ptr() for p in g.taken]
            times = []
            for _ in range(5):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                a.record()
                for _ in range(20):
                    g.plan.step_pointers(ptrs, LR, None, BETAS, 1e-8, 0.0, CLIP)
                b.record()
                torch.cuda.synchronize()
                times.append(a.elapsed_time(b) / 20)
            ms = float(np.median(times))
            info = g.plan.info
            print(json.dumps({"what": "plan step alone", "route": names[r], "bytes_per_element": nbytes, "ms_per_step": round(ms, 4), "lowest": round(min(times), 4),
                              "highest": round(max(times), 4), "TBps": round(nbytes * info["elements"] / ms / 1e9, 3), "launches_per_step": 2,
                              "chunks": info["chunks"], "chunks_16": info["chunks_16"], "uploads": info["uploads"], "upload_waits": info["upload_waits"]}), flush=True)


if __name__ == "__main__":
    main()
