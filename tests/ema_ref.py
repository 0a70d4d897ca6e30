"""LitEma (CGIC/models/ema.py:25-76) restated in plain torch, for the tests: the decay rule, the per-element expression, and copy_to /
store / restore.  tests/test_ema_host.py pins it bit for bit to tests/golden/ema.npz, which the real class wrote
(tests/golden/make_golden_ema.py); the GPU tests compare the kernels with it, run on the CPU.

The arithmetic, all of it fp32:
    n >= 0:  n += 1 (an int32 tensor: wraps);  cand = float(1 + n) / float(10 + n);  decay = cand if cand < decay else decay
             (Python's min(self.decay, cand): a NaN decay stays)
    omd = 1.0 - decay
    shadow = shadow - (omd * (shadow - param))          three roundings, no fused multiply-add
"""
import numpy as np
import torch


def _wrap32(v):
    return (int(v) + 2 ** 31) % 2 ** 32 - 2 ** 31


def next_count(n):
    """num_updates after a call that found n there"""
    return _wrap32(n + 1) if n >= 0 else n


def one_minus_decay(decay, n=None):
    """np.float32 one_minus_decay of a call that found n in num_updates (None: no counter); decay: anything np.float32 takes"""
    decay = np.float32(decay)
    if n is not None and n >= 0:
        m = next_count(n)
        with np.errstate(all="ignore"):
            cand = np.float32(_wrap32(1 + m)) / np.float32(_wrap32(10 + m))
        decay = cand if cand < decay else decay
    with np.errstate(all="ignore"):
        return np.float32(1.0) - decay


def step(shadow, param, omd):
    """shadow - (omd * (shadow - param)) as three torch operations (each rounds once); shadow's dtype, like the reference's type_as"""
    omd = torch.tensor(float(omd), dtype=torch.float32)
    return shadow - (omd * (shadow - param))


def update(shadows, params, decay, n=None):
    """one LitEma.forward over lists of CPU tensors: (new shadows, num_updates afterwards)"""
    omd = one_minus_decay(decay, n)
    return [step(s, p, omd) for s, p in zip(shadows, params)], (None if n is None else next_count(n))


def copy_to(shadows, params):
    return [s.clone() for s in shadows]


def store(params):
    return [p.clone() for p in params]


def restore(stash):
    return [c.clone() for c in stash]


def bits(t):
    """the tensor's bit patterns as integers: comparisons are on these, so that -0.0 differs from 0.0 and a NaN equals itself"""
    t = t.detach().cpu().contiguous()
    return t.view({4: torch.int32, 2: torch.int16, 8: torch.int64}[t.element_size()])


def same_bits(a, b):
    """equal bit for bit, except that a NaN of any payload equals a NaN of any other (the sign and payload of a NaN that an
    operation makes are not part of IEEE 754's contract)"""
    a, b = a.detach().cpu(), b.detach().cpu()
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    nan_a, nan_b = torch.isnan(a), torch.isnan(b)
    if not torch.equal(nan_a, nan_b):
        return False
    return torch.equal(bits(a)[~nan_a], bits(b)[~nan_b])


class Small(torch.nn.Module):
    """the module of tests/golden/ema.npz (make_golden_ema.py builds the same one): a conv, a GroupNorm, a Linear with a one-element
    bias and a frozen parameter; `load` fills it from the file"""

    def __init__(self):
        super().__init__()
        self.conv = torch.nn.Conv2d(3, 5, 3)
        self.norm = torch.nn.GroupNorm(1, 5)
        self.head = torch.nn.Linear(5, 1)
        self.frozen = torch.nn.Parameter(torch.zeros(7), requires_grad=False)

    def load(self, golden, prefix):
        """the parameters recorded under `prefix` (e.g. "plain/init", "cross/param3")"""
        with torch.no_grad():
            for k, p in self.named_parameters():
                p.copy_(torch.from_numpy(golden[f"{prefix}/{k}"]))
        return self


class StandIn(torch.nn.Module):
    """a module of the reference LitEma's SHAPE (what install(patch_ema=True) looks for and LitEma.adopt takes over): the mapping
    m_name2s_name, the buffers decay and num_updates and one buffer per trainable parameter under its name without the dots"""

    def __init__(self, model, decay=0.9999, use_num_upates=False):
        super().__init__()
        self.m_name2s_name = {k: k.replace(".", "") for k, p in model.named_parameters() if p.requires_grad}
        self.register_buffer("decay", torch.tensor(decay, dtype=torch.float32))
        self.register_buffer("num_updates", torch.tensor(0 if use_num_upates else -1, dtype=torch.int))
        for k, p in model.named_parameters():
            if p.requires_grad:
                self.register_buffer(self.m_name2s_name[k], p.detach().clone())
        self.collected_params = []
