"""Fused optimizers over :class:`FlatParams` (``csrc/kernels/optim.hip``).

``FusedAdamW`` / ``FusedAGD`` keep fp32 master weights (when the model is
bf16), exp_avg and exp_avg_sq as three flat fp32 buffers.  ``step()`` is one
kernel launch (plus two tiny ones for global-norm clipping, which never sync
the host: the clip coefficient stays on the device).

``state_dict()`` is torch-optimizer shaped ({"state": {idx: {...}},
"param_groups": [...]}) but every tensor in it is a view into a flat buffer,
so a flash checkpoint of the optimizer is three contiguous extents.

``FusedQAdamW`` is ``FusedAdamW`` with the two moments held as 8- or 4-bit
block-quantized codes (``csrc/kernels/optim_qflat.hip``,
``docs/quantized_flat_adam.md``): fewer bytes per update and per checkpoint.

Parity: ATorch optimizers (atorch/atorch/optimizers/agd.py, bf16_optimizer.py,
adam_offload.py) and the fused Adam they use.
"""

from typing import Optional

import torch

from ..ops import _hip
from ..parallel.flat import FlatParams
from ._ref_math import adam_update_, agd_update_, clip_scale


import weakref

_DEFERRING = weakref.WeakSet()  # optimizers holding a deferred state write-back


def flush_deferred_state():
    """Complete every pending deferred state write-back (device-side waits
    for the ring snapshots involved, then the replay kernels)."""
    for opt in list(_DEFERRING):
        opt.flush_deferred()


class _FlatOptimizer(torch.optim.Optimizer):
    def __init__(self, flat: FlatParams, defaults: dict, master_weights: Optional[bool] = None,
                 max_grad_norm: float = 0.0):
        self.flat = flat
        super().__init__(flat.params, defaults)
        # a lazily zeroed gradient generation (parallel/flat.py) is fully
        # defined before the update reads the whole buffer
        if hasattr(flat, "finalize_grads"):
            self.register_step_pre_hook(lambda opt, args, kwargs: opt.flat.finalize_grads())
        dev = flat.device
        self.master_weights = (flat.dtype != torch.float32) if master_weights is None else master_weights
        n = flat.numel
        self._alloc_moments(n, dev)
        self.master = flat.data.float().clone() if self.master_weights else None
        # the step counter lives in a CPU tensor that the state dict exposes
        # directly: an in-place (flash checkpoint) restore restores it too
        self._step_t = torch.zeros((), dtype=torch.float32)
        self.max_grad_norm = max_grad_norm
        # e.g. 1/world for summed DDP gradients; a FlatFSDP shard brings its own
        self.grad_scale = float(getattr(flat, "grad_scale", 1.0))
        self._scalars = torch.zeros(4, dtype=torch.float32, device=dev)  # sumsq, coef, norm, pad
        self.last_grad_norm = None

    def _alloc_moments(self, n: int, dev):
        """The moment buffers (a subclass with another state layout overrides this)."""
        self.exp_avg = torch.zeros(n, dtype=torch.float32, device=dev)
        self.exp_avg_sq = torch.zeros(n, dtype=torch.float32, device=dev)

    @property
    def step_count(self) -> int:
        return int(self._step_t.item())

    @step_count.setter
    def step_count(self, v: int):
        self._step_t.fill_(float(v))

    # ------------------------------------------------------------ helpers
    def _gscale_ptr(self):
        """Device scalar = grad_scale * clip coefficient (None if trivial)."""
        f = self.flat
        if not f.data.is_cuda or (self.max_grad_norm <= 0 and self.grad_scale == 1.0):
            return None

        def add_sumsq(out):
            _hip.check(_hip.lib().dw_sumsq_flat(_hip.ptr(f.grad), _hip.dtype_code(f.grad), f.numel, _hip.ptr(out),
                                                _hip.ptr(_hip.grid_sum_ws(out.device)), _hip.stream()), "sumsq")

        # a sharded gradient (FlatFSDP) reduces the sum: the global norm
        gs, nrm = _hip.grad_scale_scalar(self._scalars, add_sumsq, self.max_grad_norm, self.grad_scale,
                                         getattr(f, "norm_reduce", False), getattr(f, "norm_group", None))
        if nrm is not None:
            self.last_grad_norm = nrm
        return gs

    def _cpu_inputs(self):
        """CPU path (reference math): the scaled fp32 gradient, the weights
        the update writes (master or parameters) and the decay selection."""
        f = self.flat
        g = f.grad.float()
        scale = self.grad_scale
        if self.max_grad_norm > 0:
            sq = (g * g).sum().reshape(1)
            if getattr(f, "norm_reduce", False):
                import torch.distributed as dist

                dist.all_reduce(sq, group=f.norm_group)
            scale, nrm = clip_scale(sq, self.grad_scale, self.max_grad_norm)
            self.last_grad_norm = torch.tensor(nrm)
        decay = f.decay_mask.cpu().repeat_interleave(64)[: f.numel].to(f.device).bool()
        return g * scale, (self.master if self.master is not None else f.data), decay

    def _cpu_write_params(self):
        if self.master is not None:
            self.flat.data.copy_(self.master.to(self.flat.data.dtype))

    def zero_grad(self, set_to_none: bool = False):
        self.flat.zero_grad()

    # ------------------------------------------------- overlapped update
    _overlap = None

    def overlap_with_forward(self, model, chunks: int = 24):
        """Run each ``step()``'s update on a side stream, in forward order,
        under the next forward pass (``optimizers/overlap.py``).  Parameters
        and optimizer state are complete once that forward has returned, or
        after :meth:`join`."""
        from .overlap import StepOverlap

        if self._overlap is not None:
            self._overlap.remove()
        self._overlap = StepOverlap(self, model, chunks) if chunks > 0 else None
        return self._overlap

    def join(self):
        """Order the current stream after a pending overlapped update (and a
        deferred state write-back: the state is complete afterwards)."""
        if self._overlap is not None:
            self._overlap.join()
        self.flush_deferred()

    def _run_update(self, launch_range):
        """The update over the whole buffer: one launch, or piecewise on the
        overlap side stream."""
        if self._overlap is not None:
            self._overlap.launch(launch_range)
        else:
            launch_range(0, self.flat.numel)

    # ---------------------------- deferred state write-back (ring snapshots)
    # A flash-checkpoint snapshot through the bounded HBM ring (copier.py
    # _save_slice_ring) reads parameters and optimizer state while the next
    # forward / backward run; the next update normally has to wait until the
    # ring has taken ALL of them -- with a state larger than the ring that is
    # the PCIe drain of the excess (70B TP=8 shard: 123.5 GB, 64 GB ring,
    # ~0.7 s stall per save, profiles/r3/tp8_shard_70b_staging_ring64.json).
    # Instead the update runs at once: the elements whose state the ring has
    # copied are updated normally; for the others only the NEW PARAMETERS are
    # written (the next forward needs them) while their master / exp_avg /
    # exp_avg_sq keep the snapshot's values, and the step's gradient (+ clip
    # coefficient, lr, bias corrections) is kept.  Once the ring has drained,
    # one replay kernel applies the K kept steps and writes the state -- the
    # same per-element math (csrc/kernels/optim_elem.h adam_elem), so the result
    # is bit-identical to having waited.  Up to DWAMD_DEFER_STATE_STEPS
    # (default 4) steps are deferred; the memory cost is one gradient copy of
    # the deferred elements per step.  ``DWAMD_DEFER_STATE=0`` turns it off.
    _dsw = None
    _dsw_offer = None

    def offer_ring_fence(self, copier) -> bool:
        import os

        if (not self._dsw_supported() or os.environ.get("DWAMD_DEFER_STATE", "1") == "0"
                or self._overlap is not None or not self.flat.data.is_cuda):
            return False
        if self.master is None:
            # no fp32 master: the parameters ARE the weights the replay starts
            # from, and a deferred step overwrites them -- replaying the kept
            # steps would apply them twice.  Wait for the ring instead.
            return False
        if self._dsw is not None and self._dsw["copier"] is not copier:
            return False
        if self._dsw is None and not self._ring_touches(copier):
            return False  # the ring reads none of this optimizer's tensors (someone else's snapshot)
        self._dsw_offer = copier
        return True

    def _dsw_supported(self) -> bool:
        return False

    def _ring_touches(self, copier) -> bool:
        f = self.flat
        mine = [(f.data.data_ptr(), f.data.data_ptr() + f.data.element_size() * f.numel)] + self._dsw_ranges(
            0, f.numel)
        return any(a < mb and ma < b for a, b in copier.ring_sources() for ma, mb in mine)

    def _dsw_ranges(self, lo: int, hi: int):
        out = []
        for t, es in ((self.exp_avg, 4), (self.exp_avg_sq, 4), (self.master, 4)):
            if t is not None:
                out.append((t.data_ptr() + es * lo, t.data_ptr() + es * hi))
        return out

    def _dsw_first_unstaged(self, copier) -> int:
        """First flat element whose state the ring reads but has not copied
        yet (flat.numel: none)."""
        src, staged = copier.ring_sources(), copier.ring_staged()
        n = self.flat.numel
        first = n
        for t in (self.exp_avg, self.exp_avg_sq, self.master):
            if t is None:
                continue
            base, end = t.data_ptr(), t.data_ptr() + 4 * n
            # the part of the buffer the snapshot covers, minus what it has copied
            for a, b in src:
                a, b = max(a, base), min(b, end)
                if a >= b:
                    continue
                cur = a
                for sa, sb in staged:
                    if sa <= cur < sb:
                        cur = sb
                if cur < b:
                    first = min(first, (cur - base) // 4)
                    break
        return first

    def _dsw_replay(self, write_state: bool, extra=None):
        """Launch the replay over the deferred elements: the kept steps (+
        ``extra`` = this step's (grad view, gscale, lr, bc1, bc2))."""
        import ctypes

        d = self._dsw
        lo, f = d["lo"], self.flat
        n = f.numel - lo
        steps = list(d["steps"]) + ([extra] if extra is not None else [])
        K = len(steps)
        g = self.param_groups[0]
        b1, b2 = g["betas"]
        arr = ctypes.c_void_p * K
        farr = ctypes.c_float * K
        grads = arr(*[ctypes.c_void_p(x[0].data_ptr()) for x in steps])
        gss = arr(*[ctypes.c_void_p(x[1].data_ptr() if x[1] is not None else 0) for x in steps])
        ms = self.master
        _hip.check(_hip.lib().dw_adam_replay(
            _hip.ptr(f.data[lo:]), _hip.dtype_code(f.data), _hip.ptr(None if ms is None else ms[lo:]),
            _hip.ptr(self.exp_avg[lo:]), _hip.ptr(self.exp_avg_sq[lo:]), n, K, grads, _hip.dtype_code(f.grad), gss,
            farr(*[x[2] for x in steps]), farr(*[x[3] for x in steps]), farr(*[x[4] for x in steps]), float(b1),
            float(b2), float(g["eps"]), float(g["weight_decay"]), int(getattr(self, "adamw", True)),
            _hip.ptr(f.decay_mask[lo // 64:]), int(write_state), _hip.stream()), "adam_replay")

    def flush_deferred(self):
        """Write the deferred state back: the current stream waits for the
        ring snapshot (device side), then the replay runs on it."""
        d = self._dsw
        if d is None:
            return
        c = d["copier"]
        c.fence()  # every chunk copied: the old state may be overwritten now
        from ..flash_checkpoint import copier as _cp

        if _cp._FENCED is not None:
            _cp._FENCED.discard(c)
        self._dsw_replay(True)
        self._dsw = None
        _DEFERRING.discard(self)

    def _dsw_step(self, launch, gs, lr, bc1, bc2) -> bool:
        """The update under a pending ring snapshot (see above).  Returns
        False when no deferral applies (the caller runs the plain update)."""
        import os

        c = self._dsw_offer
        self._dsw_offer = None
        if c is None:
            return False
        f = self.flat
        n = f.numel
        from ..flash_checkpoint import copier as _cp

        def discard():
            if _cp._FENCED is not None:
                _cp._FENCED.discard(c)

        if c.ring_done():
            # drained: complete any deferral, then the plain update
            if self._dsw is not None:
                self.flush_deferred()
            c.fence()
            discard()
            return False
        if self._dsw is None:
            lo = self._dsw_first_unstaged(c) // 256 * 256
            if lo >= n:  # the state is fully copied; only parameters may still be in flight
                c.ring_wait_ranges([(f.data.data_ptr(), f.data.data_ptr() + f.data.element_size() * n)])
                return False
            kmax = self._defer_budget((n - lo) * f.grad.element_size())
            if kmax < 1:
                # not even one kept gradient fits next to the next step's
                # activations: wait for the ring (the stall deferral avoids)
                c.fence()
                discard()
                return False
            self._dsw = {"copier": c, "lo": lo, "steps": [], "kmax": kmax}
            _DEFERRING.add(self)
        d = self._dsw
        kmax = d["kmax"]
        if len(d["steps"]) >= kmax:
            self.flush_deferred()  # waits for the ring (the stall this bounds)
            c.fence()
            discard()
            return False
        lo = d["lo"]
        # parameters are written below: their snapshot copies must have run
        c.ring_wait_ranges([(f.data.data_ptr(), f.data.data_ptr() + f.data.element_size() * n)])
        if lo > 0:
            launch(0, lo)  # staged state: the plain update
        gk = f.grad[lo:].clone()  # this step's gradient of the deferred elements
        gsk = gs.clone() if gs is not None else None
        step = (gk, gsk, float(lr), float(bc1), float(bc2))
        self._dsw_replay(False, extra=step)  # new parameters from the snapshot's state + the kept steps
        d["steps"].append(step)
        return True

    last_defer_plan = None

    def _defer_budget(self, per_step: int) -> int:
        """Deferred steps (K) whose kept gradients fit in HBM: each deferred
        step keeps a copy of the deferred elements' gradient until the ring
        drains.  Budget = the driver's free HBM minus ``DWAMD_DEFER_RESERVE_GB``
        (2).  The caching allocator's unused cache is NOT counted: at an
        optimizer step it holds the blocks the freed activations came from,
        which the next forward takes again (a process-lifetime peak statistic
        is no measure of that: it keeps earlier, larger workloads).  K =
        min(DWAMD_DEFER_STATE_STEPS, 4 by default, budget // per-step
        bytes); 0 = wait for the ring.  The plan is kept in
        ``last_defer_plan`` (and counted by ``hbm_budget.plan``'s
        ``defer_bytes``)."""
        import os

        kcap = max(1, min(7, int(os.environ.get("DWAMD_DEFER_STATE_STEPS", "4"))))
        dev = self.flat.device
        try:
            free = int(torch.cuda.mem_get_info(dev)[0])
            cached = max(0, int(torch.cuda.memory_reserved(dev)) - int(torch.cuda.memory_allocated(dev)))
        except Exception:
            free, cached = 0, 0
        margin = int(float(os.environ.get("DWAMD_DEFER_RESERVE_GB", "2")) * (1 << 30))
        budget = free - margin
        k = max(0, min(kcap, budget // max(1, per_step + 64)))
        self.last_defer_plan = {"steps": int(k), "per_step_bytes": int(per_step), "budget_bytes": int(budget),
                                "driver_free_bytes": int(free), "allocator_cache_bytes": int(cached),
                                "decision": "defer" if k >= 1 else "wait"}
        from ..common.log import logger

        logger.info(f"deferred optimizer-state write-back plan: {self.last_defer_plan}")
        return int(k)

    def checkpoint_safe_tensors(self):
        """Tensors only ``step()`` writes (an overlapped flash-checkpoint
        snapshot may still be reading them after the save call returns)."""
        return [t for t in (self.flat.data, self.exp_avg, self.exp_avg_sq, self.master) if t is not None]

    # -------------------------------------------------------- state dict
    def _moment_views(self, o: int, c: int) -> dict:
        """The per-parameter moment entries of the state dict: flat views of
        elements [o, o + c) (none for a subclass whose moments are not per
        parameter)."""
        return {"exp_avg": self.exp_avg[o:o + c], "exp_avg_sq": self.exp_avg_sq[o:o + c]}

    def state_dict(self):
        self.flush_deferred()
        # The per-parameter views never change: build them once.  All params
        # share one "step" tensor (same value), updated in place.
        if getattr(self, "_sd_views", None) is None:
            views = {}
            for i, (o, c) in enumerate(self.flat.offsets):
                v = self._moment_views(o, c)
                if self.master is not None:
                    v["master_param"] = self.master[o:o + c]
                views[i] = {k: t.view(self.flat.params[i].shape) for k, t in v.items()}
            self._sd_views = views
        state = {i: {"step": self._step_t, **v} for i, v in self._sd_views.items()}
        groups = []
        for g in self.param_groups:
            d = {k: v for k, v in g.items() if k != "params"}
            d["params"] = list(range(len(self.flat.params)))
            groups.append(d)
        return {"state": state, "param_groups": groups}

    def load_state_dict(self, sd):
        self.flush_deferred()
        st = sd["state"]
        if self.flat.data.is_cuda:
            # a flash-checkpoint restore may still be landing this state on a
            # side stream (deferred_restore.py): order these copies after it
            from ..flash_checkpoint import deferred_restore

            deferred_restore.wait_all()
        with torch.no_grad():
            for i, (o, c) in enumerate(self.flat.offsets):
                if i not in st:
                    continue
                s = st[i]
                for k, dst in self._moment_views(o, c).items():
                    self._put(dst, s[k])
                if self.master is not None and "master_param" in s:
                    self._put(self.master[o:o + c], s["master_param"])
                self.step_count = int(float(s["step"]))
        for g, sg in zip(self.param_groups, sd.get("param_groups", [])):
            for k, v in sg.items():
                if k != "params":
                    g[k] = v

    @staticmethod
    def _put(dst, src):
        src = src.reshape(-1)
        if src.data_ptr() == dst.data_ptr() and src.numel() == dst.numel() and src.dtype == dst.dtype:
            return  # the restore wrote these views in place already
        dst.copy_(src)


class FusedAdamW(_FlatOptimizer):
    def __init__(self, flat: FlatParams, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01,
                 adamw=True, master_weights=None, max_grad_norm=0.0):
        super().__init__(flat, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay), master_weights,
                         max_grad_norm)
        self.adamw = adamw

    def _dsw_supported(self) -> bool:
        return True

    @torch.no_grad()
    def step(self, closure=None):
        loss = closure() if closure is not None else None
        self.step_count += 1
        g = self.param_groups[0]
        b1, b2 = g["betas"]
        bc1 = 1.0 - b1 ** self.step_count
        bc2 = 1.0 - b2 ** self.step_count
        f = self.flat
        if f.data.is_cuda:
            if self._overlap is not None:
                self._overlap.join()  # the previous update, if no forward ran since
            gs = self._gscale_ptr()
            ms = self.master

            def launch(lo, hi):
                _hip.check(_hip.lib().dw_adam_flat(
                    _hip.ptr(f.data[lo:hi]), _hip.dtype_code(f.data), _hip.ptr(None if ms is None else ms[lo:hi]),
                    _hip.ptr(f.grad[lo:hi]), _hip.dtype_code(f.grad), _hip.ptr(self.exp_avg[lo:hi]),
                    _hip.ptr(self.exp_avg_sq[lo:hi]), _hip.ptr(gs), hi - lo, 0, float(g["lr"]), float(b1),
                    float(b2), float(g["eps"]), float(g["weight_decay"]), float(bc1), float(bc2), int(self.adamw),
                    _hip.ptr(f.decay_mask[lo // 64:]), _hip.stream()), "adam")

            if self._dsw_offer is not None and self._dsw_step(launch, gs, g["lr"], bc1, bc2):
                return loss
            if self._dsw is not None:
                self.flush_deferred()  # (a fence taken over earlier, no longer offered)
            self._run_update(launch)
            return loss
        grad, w, decay = self._cpu_inputs()
        adam_update_(w, grad, self.exp_avg, self.exp_avg_sq, lr=g["lr"], b1=b1, b2=b2, eps=g["eps"],
                     wd=g["weight_decay"], bc1=bc1, bc2=bc2, adamw=self.adamw, decay=decay)
        self._cpu_write_params()
        return loss


class FusedAGD(_FlatOptimizer):
    """AGD (reference atorch/atorch/optimizers/agd.py) on flat buffers."""

    def __init__(self, flat: FlatParams, lr=1e-3, betas=(0.9, 0.999), delta=1e-5, weight_decay=0.0,
                 clip=None, master_weights=None, max_grad_norm=0.0):
        super().__init__(flat, dict(lr=lr, betas=betas, delta=delta, weight_decay=weight_decay, clip=clip),
                         master_weights, max_grad_norm)

    @torch.no_grad()
    def step(self, closure=None):
        loss = closure() if closure is not None else None
        self.step_count += 1
        t = self.step_count
        g = self.param_groups[0]
        b1, b2 = g["betas"]
        bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
        bc1_prev = 1.0 - b1 ** (t - 1) if t > 1 else 0.0
        clip = float(g["clip"]) if g["clip"] is not None else 0.0
        f = self.flat
        if f.data.is_cuda:
            if self._overlap is not None:
                self._overlap.join()
            gs = self._gscale_ptr()
            ms = self.master

            def launch(lo, hi):
                _hip.check(_hip.lib().dw_agd_flat(
                    _hip.ptr(f.data[lo:hi]), _hip.dtype_code(f.data), _hip.ptr(None if ms is None else ms[lo:hi]),
                    _hip.ptr(f.grad[lo:hi]), _hip.dtype_code(f.grad), _hip.ptr(self.exp_avg[lo:hi]),
                    _hip.ptr(self.exp_avg_sq[lo:hi]), _hip.ptr(gs), hi - lo, 0, float(g["lr"]), float(b1),
                    float(b2), float(g["delta"]), float(g["weight_decay"]), float(bc1), float(bc1_prev), float(bc2),
                    clip, _hip.ptr(f.decay_mask[lo // 64:]), _hip.stream()), "agd")

            self._run_update(launch)
            return loss
        grad, w, decay = self._cpu_inputs()
        agd_update_(w, grad, self.exp_avg, self.exp_avg_sq, lr=g["lr"], b1=b1, b2=b2, delta=g["delta"],
                    wd=g["weight_decay"], bc1=bc1, bc2=bc2, bc1_prev=bc1_prev, clip=clip, decay=decay)
        self._cpu_write_params()
        return loss


class FusedQAdamW(_FlatOptimizer):
    """AdamW / Adam-L2 on flat buffers with 8- or 4-bit block-quantized
    moments (``csrc/kernels/optim_qflat.hip``): the codec of
    ``optimizers/low_bit.py`` (groups of 128 consecutive flat elements, one
    fp32 scale each) instead of fp32 ``exp_avg`` / ``exp_avg_sq``.  With bf16
    parameters and an fp32 master the update moves 16 (8-bit) or 14 (4-bit)
    bytes per element instead of 28, and the resident optimizer state is 6 or
    5 bytes per element instead of 12 (``docs/quantized_flat_adam.md``).

    Buffers: ``exp_avg_q`` / ``exp_avg_sq_q`` (uint8 codes, two per byte at 4
    bits), ``exp_avg_scale`` / ``exp_avg_sq_scale`` (fp32, one per group) and
    ``master``.  A group may span two parameters; the arrays are padded to a
    multiple of 128 elements."""

    GROUP = 128

    def __init__(self, flat: FlatParams, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01,
                 adamw=True, q_bits=8, master_weights=None, max_grad_norm=0.0):
        if q_bits not in (4, 8):
            raise ValueError("q_bits must be 4 or 8")
        if master_weights is False and flat.dtype != torch.float32:
            raise ValueError("FusedQAdamW: parameters that are not fp32 need the fp32 master")
        self.q_bits = q_bits
        super().__init__(flat, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay), master_weights,
                         max_grad_norm)
        self.adamw = adamw

    def _alloc_moments(self, n: int, dev):
        self.npad = (n + self.GROUP - 1) // self.GROUP * self.GROUP
        nbytes = self.npad if self.q_bits == 8 else self.npad // 2
        self.exp_avg_q = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
        self.exp_avg_sq_q = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
        self.exp_avg_scale = torch.zeros(self.npad // self.GROUP, dtype=torch.float32, device=dev)
        self.exp_avg_sq_scale = torch.zeros(self.npad // self.GROUP, dtype=torch.float32, device=dev)

    def _moment_views(self, o: int, c: int) -> dict:
        return {}  # groups straddle parameters: the moments are the state dict's one "quantized" entry

    def _qbuffers(self):
        return {"exp_avg_q": self.exp_avg_q, "exp_avg_sq_q": self.exp_avg_sq_q,
                "exp_avg_scale": self.exp_avg_scale, "exp_avg_sq_scale": self.exp_avg_sq_scale}

    def overlap_with_forward(self, model, chunks: int = 24):
        raise NotImplementedError(
            "FusedQAdamW: the forward-overlapped update splits the buffer at parameter boundaries (64 elements), "
            "not at the 128-element quantization groups; run the plain step()")

    def checkpoint_safe_tensors(self):
        return [t for t in (self.flat.data, *self._qbuffers().values(), self.master) if t is not None]

    def state_bytes(self) -> int:
        """Bytes of the moment state, as ``Q_AdamW.state_bytes``: the codes and
        scales of both moments (what replaces FusedAdamW's 8 B per element of
        ``exp_avg`` + ``exp_avg_sq``).  The fp32 master is a copy of the
        weights and is NOT counted; with it the optimizer holds 4 B more per
        element of a non-fp32 model (``docs/quantized_flat_adam.md``)."""
        return sum(t.numel() * t.element_size() for t in self._qbuffers().values())

    # ------------------------------------------------------------- codec
    def decode_moments(self):
        """(exp_avg, exp_avg_sq) as fp32 tensors of ``npad`` elements."""
        from . import low_bit as lb

        G, bits = self.npad // self.GROUP, self.q_bits
        mc = lb._unpack4(self.exp_avg_q) if bits == 4 else self.exp_avg_q
        vc = lb._unpack4(self.exp_avg_sq_q) if bits == 4 else self.exp_avg_sq_q
        m = lb.dequant_m(mc.view(G, self.GROUP), self.exp_avg_scale, bits).reshape(-1)
        v = lb.dequant_v(vc.view(G, self.GROUP), self.exp_avg_sq_scale, bits).reshape(-1)
        return m, v

    def _encode_moments(self, m: torch.Tensor, v: torch.Tensor):
        from . import low_bit as lb

        G, bits = self.npad // self.GROUP, self.q_bits
        mcodes, ms = lb.quant_m(m.view(G, self.GROUP), bits)
        vcodes, vs = lb.quant_v(v.view(G, self.GROUP), bits)
        self.exp_avg_q.copy_(lb._pack4(mcodes.view(-1)) if bits == 4 else mcodes.view(-1))
        self.exp_avg_sq_q.copy_(lb._pack4(vcodes.view(-1)) if bits == 4 else vcodes.view(-1))
        self.exp_avg_scale.copy_(ms)
        self.exp_avg_sq_scale.copy_(vs)

    # -------------------------------------------------------------- step
    def _launch(self, lo: int, hi: int, gs, lr, b1, b2, eps, wd, bc1, bc2):
        """The update of flat elements [lo, hi), lo a multiple of 128 (groups
        are independent: a split there equals one launch)."""
        assert lo % self.GROUP == 0
        f, ms = self.flat, self.master
        cb = lo if self.q_bits == 8 else lo // 2
        _hip.check(_hip.lib().dw_qadam_flat(
            _hip.ptr(f.data[lo:hi]), _hip.dtype_code(f.data), _hip.ptr(None if ms is None else ms[lo:hi]),
            _hip.ptr(f.grad[lo:hi]), _hip.dtype_code(f.grad), _hip.ptr(self.exp_avg_q[cb:]),
            _hip.ptr(self.exp_avg_sq_q[cb:]), _hip.ptr(self.exp_avg_scale[lo // self.GROUP:]),
            _hip.ptr(self.exp_avg_sq_scale[lo // self.GROUP:]), _hip.ptr(gs), hi - lo, 0, float(lr), float(b1),
            float(b2), float(eps), float(wd), float(bc1), float(bc2), int(self.adamw),
            _hip.ptr(f.decay_mask[lo // 64:]), int(self.q_bits), _hip.stream()), "qadam_flat")

    @torch.no_grad()
    def step(self, closure=None):
        loss = closure() if closure is not None else None
        self.step_count += 1
        g = self.param_groups[0]
        b1, b2 = g["betas"]
        bc1 = 1.0 - b1 ** self.step_count
        bc2 = 1.0 - b2 ** self.step_count
        f = self.flat
        lr, wd, eps = g["lr"], g["weight_decay"], g["eps"]
        if f.data.is_cuda:
            self._launch(0, f.numel, self._gscale_ptr(), lr, b1, b2, eps, wd, bc1, bc2)
            return loss
        # CPU path (reference math): decode, the update of FusedAdamW's CPU path, encode
        n = f.numel
        grad, w, decay = self._cpu_inputs()
        mp, vp = self.decode_moments()
        # views: the padding beyond n stays in mp / vp
        adam_update_(w, grad, mp[:n], vp[:n], lr=lr, b1=b1, b2=b2, eps=eps, wd=wd, bc1=bc1, bc2=bc2,
                     adamw=self.adamw, decay=decay)
        self._cpu_write_params()
        mp[n:] = 0
        vp[n:] = 0
        self._encode_moments(mp, vp)
        return loss

    # -------------------------------------------------------- state dict
    def state_dict(self):
        """Torch-shaped; the moments are ONE top-level ``"quantized"`` entry
        (groups straddle parameters) whose tensors are the optimizer's own
        buffers, so an in-place flash-checkpoint restore lands in them."""
        sd = super().state_dict()
        sd["quantized"] = {"q_bits": self.q_bits, "group": self.GROUP, **self._qbuffers()}
        return sd

    def load_state_dict(self, sd):
        q = sd.get("quantized")
        if q is None:
            kind = "fp32 exp_avg / exp_avg_sq" if any("exp_avg" in s for s in sd.get("state", {}).values()) else "no"
            raise ValueError(f"FusedQAdamW.load_state_dict: the state dict carries {kind} moments, not the "
                             "'quantized' entry of a FusedQAdamW")
        if int(q["q_bits"]) != self.q_bits or int(q.get("group", self.GROUP)) != self.GROUP:
            raise ValueError(f"FusedQAdamW.load_state_dict: state of q_bits={q['q_bits']} group={q.get('group')}, "
                             f"this optimizer has q_bits={self.q_bits} group={self.GROUP}")
        mine = self._qbuffers()
        for k, dst in mine.items():
            if q[k].numel() != dst.numel() or q[k].dtype != dst.dtype:
                raise ValueError(f"FusedQAdamW.load_state_dict: {k} has {q[k].numel()} x {q[k].dtype}, "
                                 f"expected {dst.numel()} x {dst.dtype}")
        super().load_state_dict(sd)  # master, step, param groups; ordered after a pending deferred restore
        with torch.no_grad():
            for k, dst in mine.items():
                self._put(dst, q[k])
