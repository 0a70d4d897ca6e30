#!/usr/bin/env python3
"""A/B of cgic_decompress_streams between builds of the library, alternating round by round.

    python tools/decode_ab.py ROUNDS NAME=path/to/libcgic_hip.so [NAME=path ...]

Every (round, library) is a fresh child process under its own `timeout -k 10 120` with CGIC_LIB set; the driver itself never opens the
GPU and stops at the first child that does not exit 0.  A child times GrainCodec.decompress with bench.graph_kernel_time (20 calls
captured in one hipGraph, 5 replays between HIP events) under the three decoder arguments, at B = 64 of 256x256 and at one 768x768
tile (Zipf table, ratios (0.1, 0.8)), and prints one JSON line of microseconds per call."""
import json, os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CASES = [(64, 64, 64), (1, 192, 192)]


def child():
    import numpy as np, torch
    import control_gic_amd as cg
    from bench import graph_kernel_time
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    freq = np.floor(1e6 / (1 + np.arange(1024)) ** 1.1).astype(np.int64)
    cb = torch.from_numpy(rng.standard_normal((1024, 4)).astype(np.float32)).to(dev)
    vq = cg.VectorQuantizer(1024, 4, beta=0.25).to(dev).eval()
    vq.usage_counter.copy_(torch.from_numpy(freq.astype(np.float32)))
    codec = cg.GrainCodec(vq.embedding_counter, cb)
    router = cg.TripleGrainFixedEntropyRouter(0.1, 0.8, per_image=True)
    out = {"lib": os.environ.get("CGIC_LIB", "tree")}
    for B, h, w in CASES:
        p = 1.0 / (1 + np.arange(1024)) ** 1.1
        ind = torch.from_numpy(rng.choice(1024, size=(B, h, w), p=p / p.sum())).to(dev)
        e16 = torch.from_numpy((rng.random((B, h // 4, w // 4)) * 2.6).astype(np.float32)).to(dev)
        e8 = torch.from_numpy((rng.random((B, h // 2, w // 2)) * 2.6).astype(np.float32)).to(dev)
        mask, _, _, mode = router(e16, e8, want_gate=False)
        comp = codec.compress(ind, mask, mode)
        for d in ("auto", "latency", "throughput"):
            st = codec.decompress(comp, decoder=d)[3]
            assert int(st.abs().max()) == 0
            out[f"{B}x{h}x{w}-{d}"] = round(graph_kernel_time(lambda: codec.decompress(comp, decoder=d)), 3)
    print(json.dumps(out), flush=True)


def main():
    rounds = int(sys.argv[1])
    libs = [(a.split("=", 1)[0], os.path.abspath(a.split("=", 1)[1])) for a in sys.argv[2:]]
    for r in range(rounds):
        for name, lib in libs:
            env = dict(os.environ, CGIC_LIB=lib)
            p = subprocess.run(["timeout", "-k", "10", "120", sys.executable, os.path.abspath(__file__), "child"], env=env, capture_output=True, text=True)
            line = [l for l in p.stdout.splitlines() if l.startswith("{")]
            print(r, name, p.returncode, line[-1] if line else p.stdout[-400:] + p.stderr[-800:], flush=True)
            if p.returncode != 0:
                print("stopped: a child did not exit 0", flush=True)
                return 1
    return 0


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "child":
        child()
    else:
        sys.exit(main())
