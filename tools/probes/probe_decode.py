"""GPU probe: phase clocks of the throughput decode side on the benchmark batch (CGIC_LIB=.../libcgic_hip_dbg.so): image 0's
workgroup of decode_image_kernel (CGIC_STAMP3 0-6) and of the one-band merge_kernel (CGIC_STAMP 10-14), the launch pair alone and
with NL lanes replaying it at once; sweeps per image (cgic_decode_stats); time per decode + merge launch pair from graph replays.
usage: probe_decode.py [lanes = 4] [rounds = 12]"""
import sys, os, ctypes, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import control_gic_amd as cg
from control_gic_amd import _lib
from control_gic_amd.pipeline import distinct_queue_streams
import bench
dev = torch.device("cuda", 0)
NL = int(sys.argv[1]) if len(sys.argv) > 1 else 4
ROUNDS = int(sys.argv[2]) if len(sys.argv) > 2 else 12
N = 20                                                                     # launches per graph
TICKS_PER_US = 2.29e3                                                      # the shader clock of clock64(), as the other probes take it
slots = [bench.make_inputs(64, 256, 256, seed=s) for s in range(NL)]
cb = slots[0][2]
vq = bench.make_quantizer(dev, cb)
codec = cg.GrainCodec(vq.embedding_counter, vq.embedding.weight)
hps = [bench.HotPath(dev, x, z, cb, (0.1, 0.8), vq=vq, codec=codec) for x, z, _ in slots]
for h in hps: h.step()
torch.cuda.synchronize()
comps = [h.out[6] for h in hps]
l = _lib.lib()
have_clocks = hasattr(l, "cgic_debug_phase_clocks")
if have_clocks: l.cgic_debug_phase_clocks.argtypes = [ctypes.c_void_p]

def clocks():
    c = (ctypes.c_longlong * 32)(); l.cgic_debug_phase_clocks(c); return list(c)

DEC = ["setup: loads issued, layout", "setup: wait, LUT + streams -> LDS", "first walk", "fix point", "scan", "final walk + stores"]
MRG = ["loads", "masks -> bitsets, prefixes", "rows above", "quads + stores"]

def phases(c):
    return [(c[k + 1] - c[k]) / TICKS_PER_US for k in range(6)], c[9], [(c[k + 1] - c[k]) / TICKS_PER_US for k in range(10, 14)]

def show(title, rows):
    # (with several lanes the stamps of concurrent launches can interleave: a sample with a negative or absurd phase is dropped)
    rows = [r for r in rows if all(0 <= v < 200 for v in r[0] + r[2])]
    if not rows:
        print(f"-- {title}: no consistent sample"); return
    d = np.array([r[0] for r in rows]); s = np.array([r[1] for r in rows]); m = np.array([r[2] for r in rows])
    print(f"-- {title}: image 0's workgroup, median of {len(rows)} samples (min .. max), us")
    for k, n in enumerate(DEC): print(f"   decode {k}->{k + 1} {n:36s} {np.median(d[:, k]):6.2f}  ({d[:, k].min():5.2f} .. {d[:, k].max():5.2f})")
    print(f"   decode total {np.median(d.sum(1)):6.2f}; sweeps of image 0: {s.mean():.1f}")
    for k, n in enumerate(MRG): print(f"   merge {10 + k}->{11 + k} {n:35s} {np.median(m[:, k]):6.2f}  ({m[:, k].min():5.2f} .. {m[:, k].max():5.2f})")
    print(f"   merge total {np.median(m.sum(1)):6.2f}")

# sweeps per image over the NL batches
cnt = torch.zeros(4, dtype=torch.int32, device=dev)
l.cgic_decode_stats(cnt.data_ptr())
for c in comps: codec.decompress(c, decoder="throughput")
torch.cuda.synchronize()
l.cgic_decode_stats(None)
tot, imgs, most = cnt.tolist()[:3]
print(f"sweeps per image over {imgs} images: mean {tot / max(imgs, 1):.2f}, max {most}")

if have_clocks:
    rows = []
    for _ in range(ROUNDS):
        codec.decompress(comps[0], decoder="throughput"); torch.cuda.synchronize(); rows.append(phases(clocks()))
    show("alone", rows)

streams = distinct_queue_streams(dev, NL)
def make_graph(fn, stream):
    for _ in range(2): fn()
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=stream):
            for _ in range(N): fn()
    torch.cuda.synchronize()
    return g
gs = [(make_graph((lambda c: (lambda: codec.decompress(c, decoder="throughput")))(comps[j]), streams[j]), streams[j]) for j in range(NL)]
def run(gs):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for g, s in gs:
        with torch.cuda.stream(s): g.replay()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6
rows, t1, tn = [], [], []
for _ in range(ROUNDS):
    t1.append(run(gs[:1]) / N)
    tn.append(run(gs) / (N * NL))
    if have_clocks: rows.append(phases(clocks()))            # whichever launch stamped last, with the other lanes' launches around it
if have_clocks: show(f"{NL} lanes", rows)
print(f"decode + merge pair per launch: alone best {min(t1):.2f} median {np.median(t1):.2f} us; {NL} lanes best {min(tn):.2f} median {np.median(tn):.2f} us")
