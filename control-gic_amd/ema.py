"""LitEma (CGIC/models/ema.py) on csrc/cgic_ema.hip: the exponential moving average of a module's parameters as ONE launch over all
its tensors, with the decay rule evaluated on the device.

The reference's forward runs `shadow.sub_(one_minus_decay * (shadow - param))` tensor by tensor -- three launches and two temporaries
each -- and `if self.num_updates >= 0` reads a device buffer on the host.  Here a plan (cgic_ema_plan, include/cgic_hip.h) holds the
work list of all tensor pairs in device memory; an update is a one-thread launch that moves num_updates and computes one_minus_decay,
and one launch that applies  s - (omd * (s - p))  to every element with the same three fp32 roundings: bit-identical to the reference.

    ema = cg.LitEma(model, decay=0.9999, use_num_upates=True)        # the reference's constructor, its spelling included
    ema(model)                                                       # after every optimiser step: two launches, no synchronisation
    ema.store(model.parameters()); ema.copy_to(model); ...validate...; ema.restore(model.parameters())

    plan = cg.EmaPlan(shadows, params); plan.update(decay, num_updates)          # the same on plain lists of tensors
    torch.ops.cgic.ema_update(shadows, params, decay, num_updates)               # ... and as an op (ops.py)
"""
import ctypes as C
from collections import OrderedDict
from typing import List, Optional

import torch
from torch import nn

from . import _lib

COPY_TO, STORE, RESTORE = 0, 1, 2
_DIRECTIONS = {"copy_to": COPY_TO, "store": STORE, "restore": RESTORE, COPY_TO: COPY_TO, STORE: STORE, RESTORE: RESTORE}
INFO = ("entries", "elements", "chunks", "chunk_elements", "chunks_16", "grid", "stash_elements", "chunks_16_stash")


def kernel_takes(shadow, param):
    """the kernel's pairs: fp32, contiguous, same shape, both on one HIP device.  LitEma updates every other pair with the
    reference's torch expression"""
    return (shadow.is_cuda and param.is_cuda and shadow.device == param.device and shadow.dtype == torch.float32
            and param.dtype == torch.float32 and tuple(shadow.shape) == tuple(param.shape) and shadow.is_contiguous() and param.is_contiguous())


def _check_scalar(who, name, t, dtype, device):
    if not isinstance(t, torch.Tensor) or t.dtype != dtype or t.numel() != 1 or t.device != device:
        got = f"{t.dtype} {tuple(t.shape)} on {t.device}" if isinstance(t, torch.Tensor) else type(t).__name__
        raise TypeError(f"{who}: {name} {got}; expected one {dtype} element on {device} (LitEma's buffer: the value is read on the device)")


def check_pairs(who, shadows, params):
    """every refusal of a list of pairs, before the first data_ptr(): -> (shadows, params, device) as lists"""
    shadows, params = list(shadows), list(params)
    if len(shadows) != len(params):
        raise ValueError(f"{who}: {len(shadows)} shadows for {len(params)} params")
    _lib.require_device(*shadows, *params)
    device = shadows[0].device if shadows else None
    for i, (s, p) in enumerate(zip(shadows, params)):
        if s.dtype != torch.float32 or p.dtype != torch.float32:
            raise TypeError(f"{who}: pair {i} is {s.dtype} / {p.dtype}; the kernel takes torch.float32 (LitEma updates other pairs with torch's expression)")
        if tuple(s.shape) != tuple(p.shape):
            raise ValueError(f"{who}: pair {i}: shadow {tuple(s.shape)}, param {tuple(p.shape)}")
        if s.device != device or p.device != device:
            raise ValueError(f"{who}: pair {i} is on {s.device} / {p.device}; pair 0 is on {device} (one plan, one device)")
        if not s.is_contiguous() or not p.is_contiguous():
            raise ValueError(f"{who}: pair {i}: shadow strides {tuple(s.stride())}, param strides {tuple(p.stride())} of shape {tuple(s.shape)}; "
                             "the kernel takes contiguous tensors")
    return shadows, params, device


def pointer_key(shadows, params):
    """what a plan was built from: the addresses and element counts of its pairs"""
    return tuple((s.data_ptr(), p.data_ptr(), s.numel()) for s, p in zip(shadows, params))


class EmaPlan:
    """cgic_ema_plan of a list of (shadow, param) pairs: fp32, contiguous, same shape, all on one HIP device.  Building it uploads the
    work list (synchronously: not while a stream is capturing); `update` and `copy` only enqueue.  The plan holds addresses, not
    tensors: it is good for as long as the tensors keep their storage (`key` is what it was built from)."""

    def __init__(self, shadows, params):
        shadows, params, device = check_pairs("EmaPlan", shadows, params)
        self.device = device
        self.key = pointer_key(shadows, params)
        arr = (_lib.EmaEntry * max(len(self.key), 1))()
        for e, (s, p, n) in zip(arr, self.key):
            e.shadow, e.param, e.n = s or None, p or None, n
        self.handle = C.c_void_p()
        with _lib.on_device(device):
            _lib.call("cgic_ema_plan_create", arr, len(self.key), C.byref(self.handle))
        out = (C.c_int64 * 8)()
        _lib.call("cgic_ema_plan_info", self.handle, out)
        self.info = dict(zip(INFO, (int(v) for v in out)))

    def update(self, decay, num_updates=None):
        """shadow = shadow - (omd * (shadow - param)) for every element; decay: fp32 [1] on the plan's device; num_updates: int32
        [1] there or None (LitEma's buffers).  Two launches on the current stream, nothing else."""
        if self.device is None:
            return
        _check_scalar("EmaPlan.update", "decay", decay, torch.float32, self.device)
        if num_updates is not None:
            _check_scalar("EmaPlan.update", "num_updates", num_updates, torch.int32, self.device)
        with _lib.on_device(self.device):
            _lib.call("cgic_ema_update", self.handle, decay.data_ptr(), None if num_updates is None else num_updates.data_ptr(),
                      _lib.current_stream(self.device))

    def copy(self, direction, stash=None):
        """"copy_to": param = shadow; "store": stash = param; "restore": param = stash -- bit for bit, one launch.  stash: fp32
        [info["stash_elements"]] on the plan's device (`new_stash()`); tensor i lives at the sum of the element counts before it, each
        rounded up to a multiple of 4 (`stash_views`)."""
        if direction not in _DIRECTIONS:
            raise ValueError(f"EmaPlan.copy: direction {direction!r}; expected 'copy_to', 'store' or 'restore'")
        d = _DIRECTIONS[direction]
        if self.device is None:
            return
        if d != COPY_TO:
            if (not isinstance(stash, torch.Tensor) or stash.dtype != torch.float32 or stash.device != self.device or not stash.is_contiguous()
                    or stash.numel() < self.info["stash_elements"]):
                got = f"{stash.dtype} of {stash.numel()} elements on {stash.device}" if isinstance(stash, torch.Tensor) else type(stash).__name__
                raise ValueError(f"EmaPlan.copy: stash {got}; expected contiguous torch.float32 of at least {self.info['stash_elements']} on {self.device}")
        with _lib.on_device(self.device):
            _lib.call("cgic_ema_copy", self.handle, d, None if d == COPY_TO else stash.data_ptr(), _lib.current_stream(self.device))

    def new_stash(self):
        """ONE allocation for all tensors of the plan (the caching allocator's blocks are 512-byte aligned)"""
        return torch.empty(max(self.info["stash_elements"], 1), dtype=torch.float32, device=self.device)

    def stash_views(self, stash, shapes):
        """the tensors inside a stash, as views of the given shapes"""
        views, at = [], 0
        for (_, _, n), shape in zip(self.key, shapes):
            views.append(stash[at:at + n].view(shape))
            at += (n + 3) // 4 * 4
        return views

    def close(self):
        h, self.handle = getattr(self, "handle", None), None
        if h:
            _lib.lib().cgic_ema_plan_destroy(h)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---- the op's plans by what they were built from.  The modules keep their own plans; only torch.ops.cgic.ema_update comes here.  A
# new set of pointers builds a plan (a synchronous upload) and may push the oldest out (a hipFree): neither may happen while a
# stream is capturing, so call the op once eagerly on the tensors a capture will use, and on no more than _PLAN_CACHE_SIZE sets of
# tensors in turn
_PLAN_CACHE_SIZE = 16
_plans = OrderedDict()


def cached_plan(shadows, params):
    """the plan of these pairs, from a small LRU cache keyed by their addresses and sizes (pairs already checked)"""
    key = pointer_key(shadows, params)
    plan = _plans.get(key)
    if plan is None:
        plan = _plans[key] = EmaPlan(shadows, params)
        while len(_plans) > _PLAN_CACHE_SIZE:
            _plans.popitem(last=False)
    else:
        _plans.move_to_end(key)
    return plan


def check_update(who, shadows, params, decay, num_updates):
    """every refusal of an update over lists of tensors, before the first data_ptr(): -> (shadows, params) as lists"""
    shadows, params, device = check_pairs(who, shadows, params)
    if device is None:
        _lib.require_device(decay, num_updates)
        device = decay.device
    _check_scalar(who, "decay", decay, torch.float32, device)
    if num_updates is not None:
        _check_scalar(who, "num_updates", num_updates, torch.int32, device)
    return shadows, params


def _ema_update(shadows, params, decay, num_updates=None):
    """one EMA step over lists of tensors: every check, then the cached plan's two launches"""
    shadows, params = check_update("ema_update", shadows, params, decay, num_updates)
    if not shadows:
        # (no pair, no plan: the counter still moves, as in the reference)
        if num_updates is not None:
            num_updates.copy_(torch.where(num_updates >= 0, num_updates + 1, num_updates))
        return
    cached_plan(shadows, params).update(decay, num_updates)


@torch.library.custom_op("cgic::ema_update", mutates_args=("shadows", "num_updates"), device_types="cuda")
def ema_update(shadows: List[torch.Tensor], params: List[torch.Tensor], decay: torch.Tensor, num_updates: Optional[torch.Tensor]) -> None:
    """torch.ops.cgic.ema_update: shadows[i] -= (1 - decay') * (shadows[i] - params[i]) for all i in one launch, bit-identical to the
    reference's three torch operations; decay fp32 [1]; num_updates int32 [1] or None: when >= 0 it is incremented and decay' =
    min(decay, (1 + n) / (10 + n)), on the device (cgic_ema_update).  fp32 contiguous pairs of equal shape on one device; the plan of a
    list of pairs is cached, up to 16 lists: the FIRST call on a new set of pointers builds the plan -- a synchronous upload, and
    beyond 16 sets a hipFree of the oldest -- and so cannot be captured into a graph; call it once eagerly on those tensors first.
    Every later call only enqueues two launches.  (Defined here, next to its module, like the norms' and the attention's ops; ops.py
    lists it.)"""
    _ema_update(shadows, params, decay, num_updates)


@ema_update.register_fake
def _(shadows, params, decay, num_updates):
    check_update("ema_update", shadows, params, decay, num_updates)


def _torch_one_minus_decay(decay, num_updates):
    """ema.py:26-32 on the device without reading a value on the host: (one_minus_decay, num_updates afterwards)"""
    counted = num_updates >= 0
    n = torch.where(counted, num_updates + 1, num_updates)
    cand = (1 + n) / (10 + n)
    return 1.0 - torch.where(counted & (cand < decay), cand, decay), n


class LitEma(nn.Module):
    """The reference's LitEma with its constructor, buffers, state_dict keys and methods; forward / copy_to / store / restore run on
    the library's kernels.  forward reads no device value on the host and builds its plan on first use (and again when a tensor has
    moved, e.g. after .to()); pairs the kernel does not take (a half-precision, non-contiguous or CPU parameter) are updated by the
    reference's torch expression in the same call."""

    def __init__(self, model, decay=0.9999, use_num_upates=False):
        super().__init__()
        if not 0.0 <= decay <= 1.0:
            raise ValueError("Decay must be between 0 and 1")
        trainable = [(key, p) for key, p in model.named_parameters() if p.requires_grad]
        # a buffer's name may hold no dot: the shadow of "conv.weight" is the buffer "convweight", and the mapping remembers it
        self.m_name2s_name = {key: key.replace(".", "") for key, _ in trainable}
        self.register_buffer("decay", torch.tensor(decay, dtype=torch.float32))
        self.register_buffer("num_updates", torch.tensor(0 if use_num_upates else -1, dtype=torch.int32))     # -1: never counted
        for key, p in trainable:
            self.register_buffer(self.m_name2s_name[key], p.detach().clone())
        self.collected_params = []
        self._init_plans()

    def _init_plans(self):
        self._plan = None                   # the EmaPlan of forward / copy_to
        self._store_plan = None             # the EmaPlan of store / restore: this module's own, kept while the parameters stay put
        self._stash = None                  # (plan, flat buffer, indices in the parameter list) of the last store
        self._fused_pending = None          # set by a cg.Adam this module is attached to: the ids of the parameters whose shadows its step updated

    @classmethod
    def adopt(cls, ema):
        """a LitEma on the SAME buffers as `ema` (an instance of the reference's class): the tensor objects, their names and the
        state_dict keys stay what they are"""
        if not has_reference_shape(ema):
            raise TypeError(f"LitEma.adopt: {type(ema).__name__} has not the reference's m_name2s_name / decay / num_updates")
        self = cls.__new__(cls)
        nn.Module.__init__(self)
        self.m_name2s_name = ema.m_name2s_name
        for name, buf in ema._buffers.items():
            self.register_buffer(name, buf, persistent=name not in getattr(ema, "_non_persistent_buffers_set", ()))
        self.collected_params = list(getattr(ema, "collected_params", []))
        self.train(ema.training)
        self._init_plans()
        return self

    def __getstate__(self):
        d = self.__dict__.copy()            # (a plan is a handle of the library: a copy of the module builds its own)
        d["_plan"] = d["_store_plan"] = d["_stash"] = d["_fused_pending"] = None
        return d

    # ---- the pairs of a model
    def _scalars_on(self, device):
        """decay (fp32) and num_updates (int32) are where the update kernel reads them"""
        return (self.decay.device == device and self.num_updates.device == device and self.decay.dtype == torch.float32
                and self.num_updates.dtype == torch.int32)

    def _pairs(self, model, need_scalars=False):
        """(kernel shadows, kernel params, [(shadow, param)] for torch's expression) of the trainable parameters, matched by name
        against `model` as the reference does (ema.py:35-44).  The kernel's pairs are the ones kernel_takes() accepts on the device of
        the first such pair; need_scalars: and none at all unless decay and num_updates are on that device too"""
        ks, kp, rest = [], [], []
        device, use_kernel = None, True
        for key, p in model.named_parameters():
            if not p.requires_grad:
                if key in self.m_name2s_name:
                    raise AssertionError(f"LitEma: {key} has a shadow but no longer requires a gradient")
                continue
            s = self._buffers[self.m_name2s_name[key]]
            takes = use_kernel and kernel_takes(s, p)
            if takes and device is None:
                device = s.device
                use_kernel = takes = not need_scalars or self._scalars_on(device)
            if takes and s.device == device:
                ks.append(s)
                kp.append(p)
            else:
                rest.append((s, p))
        return ks, kp, rest

    def _plan_for(self, ks, kp):
        key = pointer_key(ks, kp)
        if self._plan is None or self._plan.key != key:
            self._plan = EmaPlan([t.detach() for t in ks], [t.detach() for t in kp])
        return self._plan

    def _forward_behind_a_fused_step(self, model, rode):
        """the forward that follows a step of a cg.Adam this module is attached to (adam.py: attach_ema): the pairs of the parameters
        in `rode` were updated inside that step, which also moved num_updates.  What is left -- parameters of another optimiser, or on
        torch's path there -- gets torch's expression on the decay of the SAME step, computed from the counter as the step left it"""
        left = []
        for key, p in model.named_parameters():
            if not p.requires_grad:
                if key in self.m_name2s_name:
                    raise AssertionError(f"LitEma: {key} has a shadow but no longer requires a gradient")
                continue
            if id(p) not in rode:
                left.append((self._buffers[self.m_name2s_name[key]], p))
        if not left:
            return
        n = self.num_updates
        counted = n >= 0
        cand = (1 + n) / (10 + n)
        omd = 1.0 - torch.where(counted & (cand < self.decay), cand, self.decay)
        for s, p in left:
            s = s if s.dtype == p.dtype and s.device == p.device else s.type_as(p)
            s.sub_((s - p) * omd)

    def forward(self, model):
        with torch.no_grad():
            rode = getattr(self, "_fused_pending", None)
            if rode is not None:
                self._fused_pending = None
                return self._forward_behind_a_fused_step(model, rode)
            ks, kp, rest = self._pairs(model, need_scalars=True)
            if rest or not ks:
                # torch's expression for these, on the decay of THIS call: taken before the kernel moves the counter
                omd, after = _torch_one_minus_decay(self.decay, self.num_updates)
            if ks:
                self._plan_for(ks, kp).update(self.decay, self.num_updates)
            else:
                self.num_updates.copy_(after)
            for s, p in rest:
                # (as the reference: a shadow of another type than its parameter is converted, and the copy is what gets updated)
                s = s if s.dtype == p.dtype and s.device == p.device else s.type_as(p)
                s.sub_((s - p) * omd)

    def copy_to(self, model):
        with torch.no_grad():
            ks, kp, rest = self._pairs(model)
            if ks:
                self._plan_for(ks, kp).copy(COPY_TO)
            for s, p in rest:
                p.data.copy_(s.data)

    def _plan_of_parameters(self, take):
        if self._store_plan is None or self._store_plan.key != pointer_key(take, take):
            self._store_plan = EmaPlan(take, take)          # (directions 1 and 2 never touch the shadow side)
        return self._store_plan

    def store(self, parameters):
        """keep a copy of `parameters` (any iterable of tensors) until restore(): the fp32 contiguous HIP ones go into ONE new buffer
        by one launch, the others are cloned one by one.  collected_params lists the copies in order, the former as views of that
        buffer.  The plan of a parameter list is this module's own, built at its first store (a synchronous upload: not inside a
        capture) and kept for as long as the parameters keep their storage"""
        with torch.no_grad():
            parameters = list(parameters)
            device = _first_device(parameters)
            mine = [i for i, p in enumerate(parameters) if p.device == device and kernel_takes(p, p)]
            copies = [None] * len(parameters)
            self._stash = None
            if mine:
                take = [parameters[i].detach() for i in mine]
                plan = self._plan_of_parameters(take)
                stash = plan.new_stash()
                plan.copy(STORE, stash)
                for i, view in zip(mine, plan.stash_views(stash, [t.shape for t in take])):
                    copies[i] = view
                self._stash = (plan, stash, mine)
            self.collected_params = [p.clone() if c is None else c for c, p in zip(copies, parameters)]

    def restore(self, parameters):
        """write the copies store() kept back into `parameters` (the same list, in the same order): one launch for the tensors that
        went into the buffer if they are still where they were, a copy_ each for the rest"""
        with torch.no_grad():
            parameters = list(parameters)
            by_kernel = ()
            if self._stash is not None:
                plan, stash, mine = self._stash
                take = [parameters[i].detach() for i in mine if i < len(parameters)]
                if len(take) == len(mine) and all(kernel_takes(t, t) for t in take) and pointer_key(take, take) == plan.key:
                    plan.copy(RESTORE, stash)
                    by_kernel = frozenset(mine)
            for i, (kept, p) in enumerate(zip(self.collected_params, parameters)):
                if i not in by_kernel:
                    p.data.copy_(kept)


def _first_device(tensors):
    for t in tensors:
        if t.is_cuda:
            return t.device
    return None


def has_reference_shape(m):
    """the reference's LitEma by its shape (ema.py:11-14): m_name2s_name and the buffers decay and num_updates"""
    return (isinstance(m, nn.Module) and isinstance(getattr(m, "m_name2s_name", None), dict)
            and "decay" in m._buffers and "num_updates" in m._buffers)


def patch_ema(model):
    """every direct attribute of `model` with the shape of the reference's LitEma becomes LitEma.adopt(it): in the reference
    ema_encoder, ema_decoder, ema_quantize, ema_quant_conv and ema_post_quant_conv (model.py:61-66).  -> the names swapped"""
    names = [name for name, m in model.named_children() if has_reference_shape(m) and not isinstance(m, LitEma)]
    for name in names:
        setattr(model, name, LitEma.adopt(getattr(model, name)))
    return names
