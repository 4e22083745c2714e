"""FusedAdamW: the reference's parameter update (main.py:243-247
``clip_grad_norm_``, main.py:420-425 AdamW) on libdctae's HIP kernels
(dctae_optim.hip): one gradient-norm pass and one pass that
scales the gradients by the clip coefficient, applies ``torch.optim.AdamW``'s
single-tensor arithmetic in fp32 and, with ``model=`` given, writes the bf16
operand packs of that ``DCTAutoencoder`` (``model._Packed``), so the next
forward does not rebuild them with torch ops.

Differences from ``clip_grad_norm_`` + ``torch.optim.AdamW``:
``p.grad`` is read, never rewritten (the clipped gradient exists only inside
the kernel); the total norm is accumulated in fp64 and left on the device in
``opt.grad_norm`` without a host synchronisation.  State (``step``,
``exp_avg``, ``exp_avg_sq``) has torch's keys and tensor types, so a
``state_dict()`` moves between the two optimizers in both directions.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional

import numpy as np
import torch

from . import _lib

_SEG_DTYPE = np.dtype([(name, {C.c_void_p: np.uint64, C.c_int64: np.int64, C.c_int32: np.int32}[ct])
                       for name, ct in _lib.OptimSeg._fields_])
assert _SEG_DTYPE.itemsize == C.sizeof(_lib.OptimSeg)


def _pad64(k: int) -> int:
    return (k + 63) // 64 * 64


def step_scalars(lr: float, beta1: float, beta2: float, weight_decay: float, step: float):
    """(1 - lr * wd, step_size, bias_correction2_sqrt) in double, as
    torch.optim.adam._single_tensor_adam computes them for its ``step``-th update."""
    bias_correction1 = 1 - beta1 ** step
    bias_correction2 = 1 - beta2 ** step
    return 1 - lr * weight_decay, lr / bias_correction1, bias_correction2 ** 0.5


def segment_plan(model) -> List[dict]:
    """One entry per ``requires_grad`` parameter of a ``DCTAutoencoder``, in
    ``named_parameters()`` order: ``name``, ``param``, ``rows``, ``cols`` and,
    for the linear weights ``_Packed`` holds, ``pack`` (its key in ``_Packed.w``
    / ``.wt``), ``row_off`` (the weight's first row inside that pack: q, k, v at
    0, d, 2d of ``qkv``) and the pack's ``pack_rows``; for the q / k / v biases
    ``bias_pack`` and ``bias_off`` inside the concatenated ``_Packed.b``; for the
    other Linear biases ``bias_alias``.  Needs no device."""
    from .model import _packed_linears
    where: Dict[int, dict] = {}
    for name, linears in _packed_linears(model):
        rows = sum(lin.weight.shape[0] for lin in linears)
        off = 0
        for lin in linears:
            where[id(lin.weight)] = dict(pack=name, row_off=off, pack_rows=rows)
            if lin.bias is not None and len(linears) > 1:
                where[id(lin.bias)] = dict(bias_pack=name, bias_off=off)
            elif lin.bias is not None:
                where[id(lin.bias)] = dict(bias_alias=name)   # _Packed.b[name] is the parameter's own storage
            off += lin.weight.shape[0]
    plan = []
    for name, p in model.named_parameters():
        if not p.requires_grad:
            continue
        rows, cols = (p.shape[0], p[0].numel()) if p.dim() >= 2 else (1, p.numel())
        plan.append(dict(name=name, param=p, rows=rows, cols=cols, **where.get(id(p), {})))
    return plan


class FusedAdamW(torch.optim.Optimizer):
    """``torch.optim.AdamW`` with ``clip_grad_norm_(params, max_grad_norm)`` in
    front, on HIP kernels.  ``max_grad_norm=None``: no norm pass, ``grad_norm``
    is None.  ``model``: the ``DCTAutoencoder`` whose packed bf16 weights the
    step maintains."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, *, max_grad_norm=None,
                 model=None, amsgrad=False, maximize=False, capturable=False, differentiable=False):
        for flag, on in (("amsgrad", amsgrad), ("maximize", maximize), ("capturable", capturable),
                         ("differentiable", differentiable)):
            if on:
                raise NotImplementedError(f"FusedAdamW: {flag}=True has no kernel")
        if isinstance(lr, torch.Tensor):
            raise NotImplementedError("FusedAdamW: a tensor lr needs capturable=True, which has no kernel")
        if lr < 0 or eps < 0 or weight_decay < 0 or not 0 <= betas[0] < 1 or not 0 <= betas[1] < 1:
            raise ValueError(f"invalid hyper-parameters: lr={lr} betas={betas} eps={eps} weight_decay={weight_decay}")
        if max_grad_norm is not None and not max_grad_norm >= 0:
            raise ValueError(f"invalid max_grad_norm: {max_grad_norm}")
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.grad_norm: Optional[torch.Tensor] = None
        self._model = model
        self._static = None       # per-parameter table rows (everything but p / g / group / norm0 / work0)
        self._pinned = None
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=False,
                                      maximize=False, foreach=None, capturable=False, differentiable=False,
                                      fused=None, decoupled_weight_decay=True))
        self._pk = None
        self._where: Dict[int, dict] = {}
        if model is not None:
            from .model import _Packed, _param_stamp
            self._stamp = _param_stamp
            self._where = {id(e["param"]): e for e in segment_plan(model)}
            self._pk = _Packed(model, training=True)
            self._seen = {k: _param_stamp(e["param"]) for k, e in self._where.items()}

    # ---- refusals ----
    @staticmethod
    def _check_param(p):
        if p.device.type != "cuda":
            raise NotImplementedError(f"FusedAdamW runs on HIP kernels: a parameter is on {p.device}")
        if p.dtype != torch.float32:
            raise NotImplementedError(f"FusedAdamW keeps fp32 master weights: a parameter is {p.dtype}")
        if p.is_sparse or not p.is_contiguous():
            raise NotImplementedError("FusedAdamW: sparse or non-contiguous parameter")

    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        g = self.param_groups[-1]
        for flag in ("amsgrad", "maximize", "capturable", "differentiable"):
            if g.get(flag):
                raise NotImplementedError(f"FusedAdamW: {flag}=True has no kernel")
        for p in g["params"]:
            self._check_param(p)
        self._static = None

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        self._static = None

    # ---- table ----
    def _init_state(self, p):
        st = self.state[p]
        if len(st) == 0:
            st["step"] = torch.tensor(0.0, dtype=torch.float32)
            st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            return True
        return False

    def _build_static(self):
        params = [p for g in self.param_groups for p in g["params"]]
        tab = np.zeros(len(params), dtype=_SEG_DTYPE)
        dev = params[0].device
        for i, p in enumerate(params):
            self._check_param(p)
            if p.device != dev:
                raise NotImplementedError(f"FusedAdamW: parameters on {dev} and {p.device}")
            st = self.state.get(p, {})
            if len(st):
                if st["step"].device.type != "cpu":   # a fused / capturable torch optimizer's state
                    st["step"] = st["step"].detach().to("cpu", torch.float32)
                for k in ("exp_avg", "exp_avg_sq"):
                    t = st[k]
                    if t.device != p.device or t.dtype != torch.float32 or t.shape != p.shape or not t.is_contiguous():
                        st[k] = t.to(p.device, torch.float32).reshape(p.shape).contiguous()
                tab["exp_avg"][i] = st["exp_avg"].data_ptr()
                tab["exp_avg_sq"][i] = st["exp_avg_sq"].data_ptr()
            rows, cols = (p.shape[0], p[0].numel()) if p.dim() >= 2 else (1, p.numel())
            tab["rows"][i], tab["cols"][i] = rows, cols
            e = self._where.get(id(p), {})
            if "pack" in e:
                w, wt = self._pk.w[e["pack"]], self._pk.wt[e["pack"]]
                assert w.shape == (e["pack_rows"], _pad64(cols)) and wt.shape == (cols, _pad64(e["pack_rows"]))
                tab["w_dst"][i], tab["ldw"][i], tab["w_row_off"][i] = w.data_ptr(), w.shape[1], e["row_off"]
                tab["wt_dst"][i], tab["ldwt"][i], tab["wt_col_off"][i] = wt.data_ptr(), wt.shape[1], e["row_off"]
            elif "bias_pack" in e:
                b = self._pk.b[e["bias_pack"]]
                tab["copy_dst"][i] = b.data_ptr() + 4 * e["bias_off"]
        self._params, self._static, self._device = params, tab, dev
        self._index = {id(p): i for i, p in enumerate(params)}
        nbytes = max(1, tab.nbytes)
        if self._pinned is None or self._pinned[0].numel() < nbytes or self._table_dev.device != dev:
            # the host writes a staging buffer only after the copy that last read it has finished
            self._pinned = [torch.empty(nbytes, dtype=torch.uint8).pin_memory() for _ in range(2)]
            self._events = [None, None]
            self._turn = 0
            self._table_dev = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            self._norm_ws = None

    def _refresh_pack(self, written):
        """Entries of the optimizer's pack whose parameter this step does not rewrite and
        that changed by other means since the pack last saw them: redo them with torch ops."""
        pk = self._pk
        for k, e in self._where.items():
            p = e["param"]
            now = self._stamp(p)
            if "bias_alias" in e:   # _Packed.b holds the parameter itself: only a reallocation matters
                if pk.b[e["bias_alias"]].data_ptr() != p.data_ptr():
                    pk.b[e["bias_alias"]] = p.detach().float().contiguous()
                continue
            if k in written or self._seen.get(k) == now:
                continue
            if "pack" in e:
                r0, r1, c = e["row_off"], e["row_off"] + e["rows"], e["cols"]
                pk.w[e["pack"]][r0:r1, :c] = p.detach().to(torch.bfloat16).view(torch.int16)
                pk.wt[e["pack"]][:c, r0:r1] = p.detach().t().to(torch.bfloat16).view(torch.int16)
            elif "bias_pack" in e:
                pk.b[e["bias_pack"]][e["bias_off"]:e["bias_off"] + e["cols"]] = p.detach()
            self._seen[k] = now

    # ---- step ----
    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if self._static is None:
            self._build_static()
        active, grads, slots, hyper = [], [], [], {}
        for gi, group in enumerate(self.param_groups):
            b1, b2 = group["betas"]
            for flag in ("amsgrad", "maximize", "capturable", "differentiable"):
                if group.get(flag):
                    raise NotImplementedError(f"FusedAdamW: {flag}=True has no kernel")
            if isinstance(group["lr"], torch.Tensor):
                raise NotImplementedError("FusedAdamW: a tensor lr needs capturable=True, which has no kernel")
            for p in group["params"]:
                g = p.grad
                if g is None:
                    continue
                if g.is_sparse:
                    raise NotImplementedError("FusedAdamW does not support sparse gradients")
                self._check_param(p)
                if g.device != p.device or g.dtype != torch.float32:
                    raise NotImplementedError(f"FusedAdamW: a {g.dtype} gradient on {g.device} for an fp32 parameter "
                                              f"on {p.device}")
                if not g.is_contiguous():
                    g = g.contiguous()
                i = self._index[id(p)]
                if self._init_state(p):
                    st = self.state[p]
                    self._static["exp_avg"][i] = st["exp_avg"].data_ptr()
                    self._static["exp_avg_sq"][i] = st["exp_avg_sq"].data_ptr()
                st = self.state[p]
                st["step"] += 1
                key = (gi, float(st["step"]))
                slot = hyper.get(key)
                if slot is None:
                    decay, step_size, bc2_sqrt = step_scalars(group["lr"], b1, b2, group["weight_decay"], key[1])
                    slot = hyper[key] = (len(hyper), (decay, 1 - b1, b2, 1 - b2, step_size, bc2_sqrt, group["eps"], 0.0))
                active.append(i)
                grads.append(g)
                slots.append(slot[0])
        if len(hyper) > _lib.OPTIM_MAX_GROUPS:
            raise NotImplementedError(f"FusedAdamW: {len(hyper)} distinct (param group, step) hyper-parameter sets in "
                                      f"one step, the kernel takes {_lib.OPTIM_MAX_GROUPS}")
        self.grad_norm = None
        if not active:
            if self.max_grad_norm is not None:
                self.grad_norm = torch.zeros((), device=self._device)
            return loss
        dev = self._device
        ctx = _lib.context(dev)
        tab = self._static[active]
        tab["p"] = [self._params[i].data_ptr() for i in active]
        tab["g"] = [g.data_ptr() for g in grads]
        tab["group"] = slots
        n_norm, n_work = C.c_int64(), C.c_int64()
        ctx.check(ctx.lib.dctae_optim_plan(ctx.h, C.c_void_p(tab.ctypes.data), len(active), C.byref(n_norm),
                                           C.byref(n_work)), "optim_plan")
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev)
            turn = self._turn
            self._turn ^= 1
            if self._events[turn] is not None:
                self._events[turn].synchronize()
            stage = self._pinned[turn][:tab.nbytes]
            stage.numpy()[:] = tab.view(np.uint8).reshape(-1)
            table = self._table_dev[:tab.nbytes]
            table.copy_(stage, non_blocking=True)
            if self._events[turn] is None:
                self._events[turn] = torch.cuda.Event()
            self._events[turn].record(stream)
            st_ptr = C.c_void_p(stream.cuda_stream)
            stats = None
            if self.max_grad_norm is not None:
                if self._norm_ws is None or self._norm_ws.numel() < n_norm.value:
                    self._norm_ws = torch.empty(max(1, n_norm.value), dtype=torch.float64, device=dev)
                stats = torch.empty(2, device=dev)
                ctx.check(ctx.lib.dctae_optim_gradnorm(ctx.h, _lib.ptr(table), len(active), n_norm.value,
                                                       C.c_float(self.max_grad_norm), _lib.ptr(self._norm_ws),
                                                       _lib.ptr(stats), st_ptr), "optim_gradnorm")
                self.grad_norm = stats[0]
            groups = (_lib.OptimGroup * len(hyper))(*[_lib.OptimGroup(*v) for _, v in hyper.values()])
            ctx.check(ctx.lib.dctae_optim_adamw_pack(ctx.h, _lib.ptr(table), len(active), n_work.value, groups,
                                                     len(hyper), _lib.ptr(stats), st_ptr), "optim_adamw_pack")
        # the kernel wrote the parameters behind autograd's back: move their version counters, so
        # saved-tensor checks and DCTAutoencoder._weights()'s key stay truthful
        updated = [self._params[i] for i in active]
        torch._C._increment_version(updated)
        if self._pk is not None:
            done = set()
            for p in updated:
                if id(p) in self._where:
                    self._seen[id(p)] = self._stamp(p)
                    done.add(id(p))
            self._refresh_pack(done)
            self._model._install_packed(self._pk)
        return loss
