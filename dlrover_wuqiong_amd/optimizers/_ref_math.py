"""The CPU reference math of the fused optimizers: one definition of the Adam
update, the AGD update and the clip coefficient, shared by the flat
(``fused.py``) and the multi-tensor (``multi_tensor.py``) classes.  It is the
CPU / gloo execution path and the numerics oracle of the GPU tests, and mirrors
``csrc/kernels/optim_elem.h`` (``adam_elem`` / ``agd_elem``).

``decay`` selects the elements that take weight decay: a bool tensor shaped
like ``w``, or ``None`` for all of them.  ``w``, ``m`` and ``v`` are updated in
place; ``grad`` is already scaled.
"""

import math

import torch


def adam_update_(w, grad, m, v, *, lr, b1, b2, eps, wd, bc1, bc2, adamw, decay=None):
    """AdamW (``adamw``: decoupled decay) or Adam with L2 decay; bc = 1 - beta^t."""
    if wd and not adamw:
        grad = grad + (wd * w if decay is None else wd * w * decay)
    m.mul_(b1).add_(grad, alpha=1 - b1)
    v.mul_(b2).addcmul_(grad, grad, value=1 - b2)
    denom = v.sqrt() / math.sqrt(bc2) + eps
    if wd and adamw:
        w.sub_(lr * wd * w if decay is None else lr * wd * w * decay)
    w.addcdiv_(m, denom, value=-lr / bc1)


def agd_update_(w, grad, m, v, *, lr, b1, b2, delta, wd, bc1, bc2, bc1_prev, clip, decay=None):
    """AGD (reference atorch/atorch/optimizers/agd.py, decoupled non-fixed
    decay); ``bc1_prev`` = 1 - b1^(t-1), 0 at the first step; ``clip``: None / 0 = off."""
    if wd:
        w.mul_(1.0 - lr * wd if decay is None else torch.where(decay, 1.0 - lr * wd, 1.0))
    m_old = m.clone()
    m.mul_(b1).add_(grad, alpha=1 - b1)
    s = m / bc1 - m_old / bc1_prev if bc1_prev > 0 else m / bc1
    v.mul_(b2).addcmul_(s, s, value=1 - b2)
    u = m / v.sqrt().clamp(min=delta * math.sqrt(bc2))
    if clip:
        u.clamp_(-clip, clip)
    w.add_(u, alpha=-lr * math.sqrt(bc2) / bc1)


def clip_scale(sumsq: torch.Tensor, grad_scale: float, max_grad_norm: float):
    """(gradient scale, global norm) from the sum of squared unscaled
    gradients: the norm is taken after ``grad_scale``, and the scale is
    ``grad_scale`` x the clip coefficient (``dw_clip_coef``)."""
    nrm = float(sumsq.sqrt()) * grad_scale
    return grad_scale * min(1.0, max_grad_norm / (nrm + 1e-6)), nrm
