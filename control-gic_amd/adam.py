"""The tail of a training step on csrc/cgic_adam.hip: clip_grad_value_, torch.optim.Adam's step and LitEma's update over all tensors
of a parameter group in ONE pass over memory -- read g, p, m, v, s and write p, m, v, s, 36 bytes per element (28 without a shadow).

The reference clips every gradient by value (configs/config_train.yaml:7-8), steps two torch.optim.Adam (CGIC/models/model.py:192-204)
and updates five LitEma (model.py:147-153), each as per-tensor work over the same tensors.  Here a plan (cgic_adam_plan,
include/cgic_hip.h) holds the work list in device memory; a step is a one-workgroup launch that moves the step counts and the EMA
counters and computes the bias corrections, and one launch that applies torch's single-tensor chain to every element with one fp32
rounding per operation (tests/adam_ref.py restates it).  No device value is read on the host.

    opt = cg.Adam(model.parameters(), lr=5e-5, betas=(0.5, 0.9), clip_value=1.0)      # a torch.optim.Adam: state_dict()s interoperate
    opt.attach_ema(ema, model)                                                       # ema: a cg.LitEma of `model`; its shadows ride in the step
    loss.backward(); opt.step(); ema(model)                                          # ema(model) has nothing left to do for those pairs

    plan = cg.AdamPlan(params, exp_avgs, exp_avg_sqs, steps); plan.step(grads, lr=..., betas=...)     # the same on plain lists of tensors
    torch.ops.cgic.adam_step(params, grads, exp_avgs, exp_avg_sqs, steps, lr, b1, b2, eps, wd, clip, None, [], None, None)   # ... and as an op
"""
import ctypes as C
from collections import OrderedDict
from typing import List, Optional

import torch

from . import _lib
from . import ema as _ema

INFO = ("entries", "elements", "chunks", "chunk_elements", "chunks_16", "grid", "ema_groups", "shadowed", "uploads", "upload_waits", "table_bytes", "steps")
MAX_EMA_GROUPS = 16


def kernel_takes(t):
    """the kernel's tensors: fp32, dense, contiguous, on a HIP device"""
    return t.is_cuda and t.dtype == torch.float32 and t.layout == torch.strided and t.is_contiguous()


def _describe(t):
    return f"{t.dtype} {tuple(t.shape)} on {t.device}" if isinstance(t, torch.Tensor) else type(t).__name__


def check_lists(who, params, exp_avgs, exp_avg_sqs, steps, shadows=None, ema_group=None, emas=()):
    """every refusal of a plan's lists, before the first data_ptr(): -> (params, exp_avgs, exp_avg_sqs, shadows, ema_group, emas, device)"""
    params, exp_avgs, exp_avg_sqs, emas = list(params), list(exp_avgs), list(exp_avg_sqs), [tuple(e) for e in emas]
    n = len(params)
    if len(exp_avgs) != n or len(exp_avg_sqs) != n:
        raise ValueError(f"{who}: {n} params, {len(exp_avgs)} exp_avgs, {len(exp_avg_sqs)} exp_avg_sqs")
    shadows = [None] * n if shadows is None else list(shadows)
    if len(shadows) != n:
        raise ValueError(f"{who}: {len(shadows)} shadows for {n} params (None where a parameter has none)")
    ema_group = [-1 if s is None else 0 for s in shadows] if ema_group is None else [int(g) for g in ema_group]
    if len(ema_group) != n:
        raise ValueError(f"{who}: {len(ema_group)} EMA group indices for {n} params")
    if len(emas) > MAX_EMA_GROUPS:
        raise ValueError(f"{who}: {len(emas)} EMA groups; a plan takes up to {MAX_EMA_GROUPS}")
    _lib.require_device(*params, *exp_avgs, *exp_avg_sqs, *[s for s in shadows if s is not None], steps, *[t for e in emas for t in e if t is not None])
    device = steps.device
    for i, (p, m, v, s, g) in enumerate(zip(params, exp_avgs, exp_avg_sqs, shadows, ema_group)):
        for name, t in (("param", p), ("exp_avg", m), ("exp_avg_sq", v), ("shadow", s)):
            if t is None:
                continue
            if t.dtype != torch.float32:
                raise TypeError(f"{who}: the {name} of entry {i} is {t.dtype}; the kernel takes torch.float32 (cg.Adam updates other parameters with torch's implementation)")
            if tuple(t.shape) != tuple(p.shape):
                raise ValueError(f"{who}: entry {i}: param {tuple(p.shape)}, {name} {tuple(t.shape)}")
            if t.device != device:
                raise ValueError(f"{who}: the {name} of entry {i} is on {t.device}; the step counts are on {device} (one plan, one device)")
            if t.layout != torch.strided or not t.is_contiguous():
                raise ValueError(f"{who}: the {name} of entry {i} has strides {tuple(t.stride())} of shape {tuple(t.shape)}; the kernel takes contiguous tensors")
        if (s is None) != (g < 0) or g >= len(emas):
            raise ValueError(f"{who}: entry {i} has {'no' if s is None else 'a'} shadow and EMA group {g} of {len(emas)} (-1: none)")
    if steps.dtype != torch.float32 or steps.dim() != 1 or steps.numel() != n or not steps.is_contiguous():
        raise TypeError(f"{who}: steps {_describe(steps)}; expected contiguous torch.float32 [{n}], one step count per entry")
    for k, e in enumerate(emas):
        if len(e) != 2:
            raise ValueError(f"{who}: EMA group {k} is not a (decay, num_updates) pair")
        _ema._check_scalar(who, f"decay of EMA group {k}", e[0], torch.float32, device)
        if e[1] is not None:
            _ema._check_scalar(who, f"num_updates of EMA group {k}", e[1], torch.int32, device)
    return params, exp_avgs, exp_avg_sqs, shadows, ema_group, emas, device


def check_hyper(who, lr, betas, eps, weight_decay, clip_value, device=None):
    """torch.optim.Adam's ranges, and the clip bound: -> (lr as a float or None, lr tensor or None)"""
    lr_t = None
    if isinstance(lr, torch.Tensor):
        if lr.numel() != 1:
            raise ValueError("Tensor lr must be 1-element")
        if lr.is_cuda:
            if lr.dtype != torch.float32 or (device is not None and lr.device != device):
                raise TypeError(f"{who}: lr {_describe(lr)}; a device lr is one torch.float32 element on {device} (the value is read on the device)")
            lr, lr_t = None, lr
        else:
            lr = float(lr)
    if lr is not None and not 0.0 <= lr:
        raise ValueError(f"Invalid learning rate: {lr}")
    if not 0.0 <= eps:
        raise ValueError(f"Invalid epsilon value: {eps}")
    if not 0.0 <= betas[0] < 1.0:
        raise ValueError(f"Invalid beta parameter at index 0: {betas[0]}")
    if not 0.0 <= betas[1] < 1.0:
        raise ValueError(f"Invalid beta parameter at index 1: {betas[1]}")
    if not 0.0 <= weight_decay:
        raise ValueError(f"Invalid weight_decay value: {weight_decay}")
    if clip_value is not None and not 0.0 <= clip_value:
        raise ValueError(f"Invalid clip_value: {clip_value} (a bound is not negative and not NaN)")
    return lr, lr_t


def pointer_key(params, exp_avgs, exp_avg_sqs, steps, shadows, ema_group, emas):
    """what a plan was built from: the addresses and element counts of its entries, its step counts and its EMA groups"""
    return (tuple((p.data_ptr(), m.data_ptr(), v.data_ptr(), 0 if s is None else s.data_ptr(), p.numel(), g)
                  for p, m, v, s, g in zip(params, exp_avgs, exp_avg_sqs, shadows, ema_group)),
            steps.data_ptr(), tuple((d.data_ptr(), 0 if n is None else n.data_ptr()) for d, n in emas))


class AdamPlan:
    """cgic_adam_plan of lists of tensors: params, exp_avgs, exp_avg_sqs (fp32, contiguous, same shapes, one HIP device), steps (fp32
    [entries] there: the step counts, moved by the kernel), and optionally per entry a shadow (or None) with the index of its EMA group
    in `emas`, a list of up to 16 (decay fp32 [1], num_updates int32 [1] or None) pairs -- the buffers of one LitEma each.  Building
    it uploads the work list (synchronously: not while a stream is capturing); `step` only enqueues.  The plan holds addresses, not
    tensors: it is good for as long as the tensors keep their storage (`key` is what it was built from)."""

    def __init__(self, params, exp_avgs, exp_avg_sqs, steps, shadows=None, ema_group=None, emas=()):
        params, exp_avgs, exp_avg_sqs, shadows, ema_group, emas, device = check_lists("AdamPlan", params, exp_avgs, exp_avg_sqs, steps, shadows, ema_group, emas)
        self.device = device
        self.key = pointer_key(params, exp_avgs, exp_avg_sqs, steps, shadows, ema_group, emas)
        self.numels = [e[4] for e in self.key[0]]
        self.present = steps.data_ptr()              # what stands for the gradient of an EMPTY tensor (torch gives those no address): never read
        n = len(self.numels)
        arr = (_lib.AdamEntry * max(n, 1))()
        for e, (p, m, v, s, k, g) in zip(arr, self.key[0]):
            e.param, e.exp_avg, e.exp_avg_sq, e.shadow, e.n, e.ema_group = p or None, m or None, v or None, s or None, k, g
        groups = (_lib.AdamEmaGroup * max(len(emas), 1))()
        for e, (d, c) in zip(groups, self.key[2]):
            e.decay, e.num_updates = d or None, c or None
        self.handle = C.c_void_p()
        with _lib.on_device(device):
            _lib.call("cgic_adam_plan_create", arr, n, groups, len(emas), steps.data_ptr() or None, C.byref(self.handle))

    @property
    def info(self):
        """cgic_adam_plan_info as a dict; "uploads" counts the uploads of the gradient table so far"""
        out = (C.c_int64 * 12)()
        _lib.call("cgic_adam_plan_info", self.handle, out)
        return dict(zip(INFO, (int(v) for v in out)))

    def check_grads(self, who, grads):
        """every refusal of a step's gradients, before the first data_ptr()"""
        grads = list(grads)
        if len(grads) != len(self.numels):
            raise ValueError(f"{who}: {len(grads)} gradients for {len(self.numels)} entries (None where a parameter has none)")
        _lib.require_device(*[g for g in grads if g is not None])
        for i, (g, n) in enumerate(zip(grads, self.numels)):
            if g is None:
                continue
            if g.dtype != torch.float32 or g.layout != torch.strided or not g.is_contiguous() or g.numel() != n or g.device != self.device:
                raise ValueError(f"{who}: the gradient of entry {i} is {_describe(g)} with strides {tuple(g.stride()) if g.layout == torch.strided else g.layout}; "
                                 f"expected dense contiguous torch.float32 of {n} elements on {self.device}")
        return grads

    def step(self, grads, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, clip_value=None):
        """one fused step on the current stream: two launches, and an upload of the gradients' addresses when they differ from those
        of the previous call.  grads: per entry a dense fp32 contiguous tensor or None (no gradient: the entry's step count, m, v and
        p stay, its shadow is still updated); lr: a float or an fp32 [1] tensor on the plan's device, read there"""
        lr, lr_t = check_hyper("AdamPlan.step", lr, betas, eps, weight_decay, clip_value, self.device)
        grads = self.check_grads("AdamPlan.step", grads)
        self.step_pointers([0 if g is None else g.data_ptr() or self.present for g in grads], lr, lr_t, betas, eps, weight_decay, clip_value)

    def step_pointers(self, ptrs, lr, lr_t, betas, eps, weight_decay, clip_value):
        """`step` behind its checks: ptrs the gradients' addresses (0: none)"""
        hyper = _lib.AdamHyper(0.0 if lr is None else lr, betas[0], betas[1], eps, weight_decay, 0.0 if clip_value is None else clip_value,
                               int(clip_value is not None), 0, None if lr_t is None else lr_t.data_ptr())
        arr = (C.c_uint64 * max(len(ptrs), 1))(*ptrs)
        with _lib.on_device(self.device):
            _lib.call("cgic_adam_step", self.handle, arr, C.byref(hyper), _lib.current_stream(self.device))

    def close(self):
        h, self.handle = getattr(self, "handle", None), None
        if h:
            _lib.lib().cgic_adam_plan_destroy(h)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---- the op's plans by what they were built from, like ema.py's: the FIRST call on a new set of pointers builds a plan (a synchronous
# upload) and may push the oldest out (a hipFree): neither may happen while a stream is capturing
_PLAN_CACHE_SIZE = 16
_plans = OrderedDict()


def _adam_step(params, grads, exp_avgs, exp_avg_sqs, steps, lr, beta1, beta2, eps, weight_decay, clip_value=None, lr_tensor=None, shadows=None,
               decay=None, num_updates=None, fake=False):
    """one fused step over lists of tensors: every check, then the cached plan's launches"""
    who = "adam_step"
    shadows = list(shadows) if shadows is not None and len(shadows) else None
    if (shadows is None) != (decay is None):
        raise ValueError(f"{who}: shadows and decay come together (one EMA group over all entries; no shadows: an empty list and no decay)")
    emas = [] if decay is None else [(decay, num_updates)]
    lists = check_lists(who, params, exp_avgs, exp_avg_sqs, steps, shadows, None, emas)
    check_hyper(who, lr if lr_tensor is None else lr_tensor, (beta1, beta2), eps, weight_decay, clip_value, lists[-1])
    if fake:
        grads = list(grads)
        if len(grads) != len(lists[0]):
            raise ValueError(f"{who}: {len(grads)} gradients for {len(lists[0])} entries (None where a parameter has none)")
        return
    key = pointer_key(lists[0], lists[1], lists[2], steps, lists[3], lists[4], lists[5])
    plan = _plans.get(key)
    if plan is None:
        plan = _plans[key] = AdamPlan(lists[0], lists[1], lists[2], steps, lists[3], lists[4], lists[5])
        while len(_plans) > _PLAN_CACHE_SIZE:
            _plans.popitem(last=False)
    else:
        _plans.move_to_end(key)
    plan.step(grads, lr if lr_tensor is None else lr_tensor, (beta1, beta2), eps, weight_decay, clip_value)


@torch.library.custom_op("cgic::adam_step", mutates_args=("params", "exp_avgs", "exp_avg_sqs", "steps", "shadows", "num_updates"), device_types="cuda")
def adam_step(params: List[torch.Tensor], grads: List[Optional[torch.Tensor]], exp_avgs: List[torch.Tensor], exp_avg_sqs: List[torch.Tensor],
              steps: torch.Tensor, lr: float, beta1: float, beta2: float, eps: float, weight_decay: float, clip_value: Optional[float],
              lr_tensor: Optional[torch.Tensor], shadows: List[torch.Tensor], decay: Optional[torch.Tensor],
              num_updates: Optional[torch.Tensor]) -> None:
    """torch.ops.cgic.adam_step: clip by value (clip_value or None), torch.optim.Adam's step and -- with shadows, decay and optionally
    num_updates, the buffers of one LitEma -- the EMA of the new parameters, for all entries in one pass (cgic_adam_step), in place.
    grads[i] None: no gradient this step; shadows: one per entry, or an empty list with decay None.  steps: fp32 [entries], the step counts.  lr_tensor: fp32 [1] on the device, replaces lr.
    fp32 contiguous tensors on one device; the plan of a set of lists is cached, up to 16: the FIRST call on new pointers builds it
    and cannot be captured into a graph.  (Defined here, next to its class; ops.py lists it.)"""
    _adam_step(params, grads, exp_avgs, exp_avg_sqs, steps, lr, beta1, beta2, eps, weight_decay, clip_value, lr_tensor, shadows, decay, num_updates)


@adam_step.register_fake
def _(params, grads, exp_avgs, exp_avg_sqs, steps, lr, beta1, beta2, eps, weight_decay, clip_value, lr_tensor, shadows, decay, num_updates):
    _adam_step(params, grads, exp_avgs, exp_avg_sqs, steps, lr, beta1, beta2, eps, weight_decay, clip_value, lr_tensor, shadows, decay, num_updates, fake=True)


# ---------------------------------------------------------------------------------------------------------------- the optimiser
_OFF_FLAGS = ("amsgrad", "maximize", "differentiable", "capturable", "decoupled_weight_decay")


class _Group:
    """what cg.Adam keeps per param group: the parameters the kernel takes, the rest, the plan and what it was built from"""
    __slots__ = ("taken", "rest", "plan", "steps", "pkey", "skey", "shadows", "nparams", "flags", "emas", "owned", "device")


class Adam(torch.optim.Adam):
    """torch.optim.Adam whose step runs on csrc/cgic_adam.hip: per param group ONE pass over g, p, m, v (and s) for every parameter
    that is fp32, contiguous and on the group's HIP device, in a group without amsgrad, maximize, differentiable, capturable or
    decoupled_weight_decay; any other parameter is updated in the same step() by torch's own implementation.

    clip_value: clip every gradient to +-clip_value first, inside the same pass (Lightning's gradient_clip_algorithm 'value').  The
        clipped gradient is not written back: p.grad keeps the raw gradient, unlike after clip_grad_value_.  Parameters on torch's
        path are clipped by p.grad.clamp_ first, which does write.
    state[p] keeps torch's keys step, exp_avg, exp_avg_sq; `step` is a 0-dim view into one fp32 device buffer per param group, which
        the kernel moves.  state_dict() hands the step counts out as CPU tensors, as torch's default does, so a plain
        torch.optim.Adam loads it, and load_state_dict() takes a plain torch.optim.Adam's dict; the plan is rebuilt at the next step.
        Replace optimiser state through load_state_dict only.  A kernel-taken parameter's state exists from the first step on, also
        where it never had a gradient (step 0, zeros).
    step() reads no device value on the host.  The group's lr may be a float, a CPU tensor, or an fp32 [1] tensor on the device,
        which the kernel reads (a captured step then follows a schedule).
    attach_ema(ema, module): see there."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, *, clip_value=None, **kwargs):
        if clip_value is not None:
            clip_value = float(clip_value)
            if not 0.0 <= clip_value:
                raise ValueError(f"Invalid clip_value: {clip_value} (a bound is not negative and not NaN)")
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, **kwargs)
        self.clip_value = clip_value
        self._groups = {}
        self._attached = []

    @classmethod
    def from_torch(cls, opt, clip_value=None):
        """a cg.Adam on the SAME param groups (the dict objects), defaults and state as `opt`, a torch.optim.Adam"""
        if not isinstance(opt, torch.optim.Adam):
            raise TypeError(f"Adam.from_torch: {type(opt).__name__} is not a torch.optim.Adam")
        new = cls(opt.param_groups, clip_value=clip_value, **opt.defaults)
        new.param_groups = opt.param_groups
        if len(opt.state):
            new.load_state_dict(opt.state_dict())
        return new

    def __setstate__(self, state):
        super().__setstate__(state)
        self.__dict__.setdefault("clip_value", None)
        self._groups, self._attached = {}, self.__dict__.get("_attached", [])

    def __getstate__(self):
        d = dict(super().__getstate__())                     # (a plan is a handle of the library: a copy builds its own)
        d["clip_value"] = self.clip_value
        return d

    # ---- EMA
    def attach_ema(self, ema, module):
        """the shadows of `module`'s parameters that this optimiser owns ride in its step: `ema` (a cg.LitEma of `module`) is updated on
        the NEW parameters inside the fused pass, its num_updates moves once per step, and the `ema(module)` that follows such a step
        does nothing for those pairs -- it still updates, by torch's expression on the decay of the same step, the pairs that did not
        ride: parameters of another optimiser, on torch's path here, or beyond the 16 EMA groups of a plan.  An `ema(module)` with no
        fused step before it behaves as without attachment.  All of an ema's riding parameters must be in ONE param group (its
        counter moves once per plan); step() raises otherwise.  Measured on the training config's 655 tensors (profiles/adam.md): a tail with
        the five modules attached takes 1.170 ms against 1.277 ms for the same step followed by cg.LitEma -- not slower, but the
        difference is inside the run-to-run spread of that host-bound benchmark (kernel time: 0.95 ms against 0.74 + 0.33 ms)."""
        if not isinstance(ema, _ema.LitEma):
            raise TypeError(f"Adam.attach_ema: {type(ema).__name__} is not a control_gic_amd.LitEma (LitEma.adopt takes over a reference instance)")
        if not isinstance(module, torch.nn.Module):
            raise TypeError(f"Adam.attach_ema: module is a {type(module).__name__}")
        mine = {id(p) for g in self.param_groups for p in g["params"]}
        if not any(id(p) in mine for k, p in module.named_parameters() if k in ema.m_name2s_name):
            raise ValueError("Adam.attach_ema: this optimiser owns no parameter of the module that the ema has a shadow for")
        if not any(e is ema for e, _ in self._attached):
            self._attached.append((ema, module))
        self._groups = {}

    def _shadow_of(self):
        """id(param) -> (index in self._attached, shadow)"""
        out = {}
        for k, (ema, module) in enumerate(self._attached):
            for name, p in module.named_parameters():
                sname = ema.m_name2s_name.get(name)
                if sname is not None and p.requires_grad and id(p) not in out:
                    out[id(p)] = (k, ema._buffers[sname])
        return out

    # ---- state
    def state_dict(self):
        """torch's layout; the step counts of kernel-taken parameters as 0-dim fp32 CPU tensors (one device read per param group)"""
        sd = super().state_dict()
        index = {}
        at = 0
        for g in self.param_groups:
            for p in g["params"]:
                index[id(p)] = at
                at += 1
        for gi, g in self._groups.items():
            if g.steps is None:
                continue
            host = g.steps.detach().cpu()
            for i, p in enumerate(g.taken):
                st = sd["state"].get(index.get(id(p)))
                if st is not None and "step" in st:
                    st = sd["state"][index[id(p)]] = dict(st)
                    st["step"] = host[i].clone()
        return sd

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        self._groups = {}                                    # rebuilt from the new tensors and step values at the next step

    # ---- the plan of a param group
    @staticmethod
    def _flags(group):
        return tuple(bool(group.get(k, False)) for k in _OFF_FLAGS)

    def _build(self, gi, group):
        g = _Group()
        g.flags, g.nparams = self._flags(group), len(group["params"])
        lr = group["lr"]
        usable = not any(g.flags) and not (isinstance(lr, torch.Tensor) and lr.is_cuda and (lr.dtype != torch.float32 or lr.numel() != 1))
        g.device = next((p.device for p in group["params"] if kernel_takes(p)), None) if usable else None
        if isinstance(lr, torch.Tensor) and lr.is_cuda and g.device is not None and lr.device != g.device:
            g.device = None
        g.taken = [p for p in group["params"] if g.device is not None and kernel_takes(p) and p.device == g.device]
        ids = {id(p) for p in g.taken}
        g.rest = [p for p in group["params"] if id(p) not in ids]
        g.plan = g.steps = None
        g.pkey, g.skey, g.shadows, g.emas, g.owned = (), (), [], [], {}
        if not g.taken:
            return g
        n = len(g.taken)
        steps = torch.zeros(n, dtype=torch.float32, device=g.device)
        host, late = [0.0] * n, []
        exp_avgs, exp_avg_sqs = [], []
        for i, p in enumerate(g.taken):
            st = self.state[p]
            for key in ("exp_avg", "exp_avg_sq"):
                t = st.get(key)
                if t is None:
                    t = torch.zeros_like(p, memory_format=torch.preserve_format)
                elif not kernel_takes(t) or t.device != g.device or tuple(t.shape) != tuple(p.shape):
                    t = t.detach().to(device=g.device, dtype=torch.float32).reshape(p.shape).contiguous()
                st[key] = t
            old = st.get("step")
            if isinstance(old, torch.Tensor) and old.is_cuda:
                late.append((i, old))                        # a device value stays on the device
            elif old is not None:
                host[i] = float(old)
            exp_avgs.append(st["exp_avg"])
            exp_avg_sqs.append(st["exp_avg_sq"])
        if any(host):
            steps.copy_(torch.tensor(host, dtype=torch.float32))
        for i, old in late:
            steps[i].copy_(old.detach().reshape(()))
        for i, p in enumerate(g.taken):
            self.state[p]["step"] = steps[i]
        # the shadows that ride
        shadow_of = self._shadow_of() if self._attached else {}
        used, shadows, ema_group = [], [], []
        for p in g.taken:
            k, s = shadow_of.get(id(p), (None, None))
            if k is not None:
                ema = self._attached[k][0]
                ok = _ema.kernel_takes(s, p) and s.device == g.device and ema._scalars_on(g.device) and (k in used or len(used) < MAX_EMA_GROUPS)
                if ok and k not in used:
                    used.append(k)
                if not ok:
                    k = s = None
            shadows.append(s if k is not None else None)
            ema_group.append(used.index(k) if k is not None else -1)
        g.emas = [self._attached[k][0] for k in used]
        for other_gi, other in self._groups.items():
            if other_gi != gi and any(e is o for e in g.emas for o in other.emas):
                raise ValueError("cg.Adam: the parameters of one attached LitEma lie in more than one param group; its counter moves once per "
                                 "plan, so keep them in one group or leave that ema unattached")
        g.owned = {id(e): frozenset(id(p) for p, q in zip(g.taken, ema_group) if q >= 0 and g.emas[q] is e) for e in g.emas}
        g.shadows = [s for s in shadows if s is not None]
        g.steps = steps
        g.plan = AdamPlan([p.detach() for p in g.taken], exp_avgs, exp_avg_sqs, steps, shadows, ema_group, [(e.decay, e.num_updates) for e in g.emas])
        g.pkey = tuple(p.data_ptr() for p in g.taken)
        g.skey = tuple(s.data_ptr() for s in g.shadows)
        return g

    def _group(self, gi, group):
        g = self._groups.get(gi)
        if (g is None or g.nparams != len(group["params"]) or g.flags != self._flags(group) or g.pkey != tuple(p.data_ptr() for p in g.taken)
                or g.skey != tuple(s.data_ptr() for s in g.shadows)):
            self._groups.pop(gi, None)
            g = self._groups[gi] = self._build(gi, group)
        return g

    def _torch_step(self, group, params):
        """torch.optim.Adam.step for `params` of `group`, as the installed torch runs it"""
        from torch.optim.adam import adam as _adam
        with_grad, grads, exp_avgs, exp_avg_sqs, max_exp_avg_sqs, state_steps = [], [], [], [], [], []
        sub = dict(group)
        sub["params"] = params
        has_complex = self._init_group(sub, with_grad, grads, exp_avgs, exp_avg_sqs, max_exp_avg_sqs, state_steps)
        if not with_grad:
            return
        beta1, beta2 = group["betas"]
        extra = {"decoupled_weight_decay": group["decoupled_weight_decay"]} if "decoupled_weight_decay" in group else {}
        _adam(with_grad, grads, exp_avgs, exp_avg_sqs, max_exp_avg_sqs, state_steps, amsgrad=group["amsgrad"], has_complex=has_complex, beta1=beta1,
              beta2=beta2, lr=group["lr"], weight_decay=group["weight_decay"], eps=group["eps"], maximize=group["maximize"], foreach=group["foreach"],
              capturable=group["capturable"], differentiable=group["differentiable"], fused=group["fused"], grad_scale=getattr(self, "grad_scale", None),
              found_inf=getattr(self, "found_inf", None), **extra)

    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        with torch.no_grad():
            for gi, group in enumerate(self.param_groups):
                g = self._group(gi, group)
                clip = self.clip_value
                if g.rest:
                    if clip is not None:
                        for p in g.rest:
                            if p.grad is not None and not p.grad.is_sparse:
                                p.grad.clamp_(-clip, clip)
                    self._torch_step(group, g.rest)          # (first: a shadow of the pass below reads the parameter it finds)
                if g.plan is None:
                    continue
                lr, lr_t = check_hyper("cg.Adam", group["lr"], group["betas"], group["eps"], group["weight_decay"], clip, g.device)
                ptrs, keep = [], []
                for p in g.taken:
                    gr = p.grad
                    if gr is None:
                        ptrs.append(0)
                        continue
                    if gr.is_sparse:
                        raise RuntimeError("Adam does not support sparse gradients, please consider SparseAdam instead")
                    if not gr.is_contiguous():
                        gr = gr.contiguous()                 # (a temporary of this step: stream order keeps it until the pass has read it)
                        keep.append(gr)
                    ptrs.append(gr.data_ptr() or g.plan.present)
                g.plan.step_pointers(ptrs, lr, lr_t, group["betas"], group["eps"], group["weight_decay"], clip)
                for e in g.emas:
                    e._fused_pending = g.owned[id(e)]
        return loss


# ---------------------------------------------------------------------------------------------------------------- install()
def _swap(obj, model, clip_value, attach, made):
    if type(obj) is torch.optim.Adam:
        if id(obj) not in made:
            new = made[id(obj)] = Adam.from_torch(obj, clip_value=clip_value)
            if attach:
                attach_model_emas(new, model)
        return made[id(obj)]
    if isinstance(obj, (list, tuple)):
        return type(obj)(_swap(o, model, clip_value, attach, made) for o in obj)
    if isinstance(obj, dict):
        return {k: _swap(v, model, clip_value, attach, made) for k, v in obj.items()}
    if type(getattr(obj, "optimizer", None)) is torch.optim.Adam:          # a scheduler follows the optimiser that replaces its own
        obj.optimizer = _swap(obj.optimizer, model, clip_value, attach, made)
    return obj


def attach_model_emas(opt, model):
    """every cg.LitEma child `ema_<name>` of `model` whose module `model.<name>` has parameters in `opt` is attached to it
    (the reference: ema_encoder, ema_decoder, ema_quantize, ema_quant_conv, ema_post_quant_conv, model.py:61-66).  -> the names"""
    mine = {id(p) for g in opt.param_groups for p in g["params"]}
    names = []
    for name, child in model.named_children():
        target = getattr(model, name[4:], None) if name.startswith("ema_") else None
        if isinstance(child, _ema.LitEma) and isinstance(target, torch.nn.Module) and any(id(p) in mine for p in target.parameters()):
            opt.attach_ema(child, target)
            names.append(name)
    return names


def patch_optimizers(model, clip_value=None, attach_emas=False):
    """wrap model.configure_optimizers: every optimiser it returns of EXACTLY type torch.optim.Adam becomes a cg.Adam on the same param
    groups and defaults (other optimisers, and subclasses of Adam, are left alone); attach_emas: the model's cg.LitEma children are
    attached to the optimiser that owns their parameters"""
    original = model.configure_optimizers

    def configure_optimizers(*args, **kwargs):
        return _swap(original(*args, **kwargs), model, clip_value, attach_emas, {})

    configure_optimizers._cgic_original = original
    model.configure_optimizers = configure_optimizers
    return model
