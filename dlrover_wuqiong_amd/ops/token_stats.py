"""Log-prob of a label and entropy of ``softmax(logits)`` per position
(``csrc/kernels/token_logprob.hip``): the PPO actor's response log-probs and
entropy bonus from one read of the logits forward and one backward, without
the fp32 ``[B, R, V]`` log-softmax copies.

``logits`` is ``[..., V]``, bf16 or fp32, with the last dim contiguous.  A
2-D or 3-D view with arbitrary leading strides (``logits[:, P-1:-1, :]``) is
read in place; anything else is made contiguous first.  The gradient is a
dense ``[rows, V]`` tensor in the logits' dtype (autograd's slice backward
embeds it).  CPU tensors run the torch math.

Parity: reference ``atorch/rl/model_utils/model_util.py``
(``logprobs_of_labels``) and the entropy term of ``rl/ppo_utils/ppo_util.py``.
"""

import torch
import torch.nn.functional as F

from . import _hip


def _torch_stats(logits, labels, with_entropy):
    """The torch expressions (bitwise those of ``rl/ppo_utils`` for finite
    logits); a ``-inf`` logit adds 0 to the entropy and a label outside
    ``[0, V)`` gives 0, as in the kernel."""
    lp = F.log_softmax(logits.float(), dim=-1)
    if labels is None:
        logp = None
    else:
        valid = (labels >= 0) & (labels < logits.shape[-1])
        logp = lp.gather(-1, labels.clamp(0, logits.shape[-1] - 1).unsqueeze(-1)).squeeze(-1)
        if not bool(valid.all()):
            logp = torch.where(valid, logp, torch.zeros_like(logp))
    if not with_entropy:
        return logp, None
    neg_inf = lp == float("-inf")
    lp_safe = lp.masked_fill(neg_inf, 0.0) if bool(neg_inf.any()) else lp
    return logp, -(lp.exp() * lp_safe).sum(-1)


def backward_math(logits, labels, lse, ent, g_logp=None, g_ent=None):
    """The backward the kernel computes, in torch (any float dtype):

        dx_j = g_logp * ([j == label] - p_j) - g_ent * p_j * ((x_j - lse) + H),   p_j = exp(x_j - lse)

    ``lse`` / ``ent`` / the upstream gradients are shaped like ``labels``;
    either gradient may be None.  ``p_j = 0`` gives 0; a label outside
    ``[0, V)`` makes ``logp`` the constant 0, so its ``g_logp`` is dropped."""
    V = logits.shape[-1]
    d = logits - lse.unsqueeze(-1)
    p = d.exp()
    coef = torch.zeros_like(lse).unsqueeze(-1).expand_as(d)
    dx = torch.zeros_like(d)
    if g_logp is not None:
        valid = (labels >= 0) & (labels < V)
        g1 = torch.where(valid, g_logp.to(d.dtype), torch.zeros_like(lse))
        dx = dx.scatter_add(-1, labels.clamp(0, V - 1).unsqueeze(-1), g1.unsqueeze(-1))
        coef = coef + g1.unsqueeze(-1)
    if g_ent is not None:
        coef = coef + g_ent.to(d.dtype).unsqueeze(-1) * (d + ent.unsqueeze(-1))
    return dx - torch.where(p > 0, p * coef, torch.zeros_like(p))


def _rows(logits):
    """(tensor to read, rows, R, batch stride, row stride) of the kernel's
    two-level row addressing."""
    V = logits.shape[-1]
    if logits.dim() not in (2, 3) or (V > 1 and logits.stride(-1) != 1):
        logits = logits.contiguous().view(-1, V)
    if logits.dim() == 2:
        return logits, logits.shape[0], max(logits.shape[0], 1), 0, logits.stride(0)
    return logits, logits.shape[0] * logits.shape[1], max(logits.shape[1], 1), logits.stride(0), logits.stride(1)


class _TokenStatsFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, labels):
        x, rows, R, bs, rs = _rows(logits)
        V = x.shape[-1]
        t = None if labels is None else labels.contiguous().view(-1).to(torch.int64)
        out = torch.empty(3, rows, device=x.device, dtype=torch.float32)
        logp, lse, ent = out[0], out[1], out[2]
        _hip.check(_hip.lib().dw_token_logprob_fwd(_hip.ptr(x), _hip.dtype_code(x), _hip.ptr(t), _hip.ptr(logp),
                                                   _hip.ptr(lse), _hip.ptr(ent), rows, R, bs, rs, V, _hip.stream()),
                   "token_logprob_fwd")
        ctx.save_for_backward(x, t, lse, ent)
        ctx.geom = (rows, R, bs, rs, logits.shape)
        ctx.set_materialize_grads(False)
        shape = logits.shape[:-1]
        return logp.view(shape), ent.view(shape)

    @staticmethod
    def backward(ctx, g_logp, g_ent):
        if g_logp is None and g_ent is None:
            return None, None
        x, t, lse, ent = ctx.saved_tensors
        rows, R, bs, rs, shape = ctx.geom
        V = x.shape[-1]
        g1 = None if g_logp is None else g_logp.contiguous().view(-1).float()
        g2 = None if g_ent is None else g_ent.contiguous().view(-1).float()
        dx = torch.empty(rows, V, device=x.device, dtype=x.dtype)
        _hip.check(_hip.lib().dw_token_logprob_bwd(_hip.ptr(x), _hip.dtype_code(x), _hip.ptr(t), _hip.ptr(lse),
                                                   _hip.ptr(ent), _hip.ptr(g1), _hip.ptr(g2), _hip.ptr(dx), rows, R,
                                                   bs, rs, V, _hip.stream()), "token_logprob_bwd")
        return dx.view(shape), None


def _kernel_dtype(logits):
    return logits if logits.dtype in (torch.bfloat16, torch.float32) else logits.float()


def token_logprobs(logits, labels, with_entropy=False):
    """``log softmax(logits)[label]`` per position, fp32, shaped like
    ``labels``; with ``with_entropy`` also the entropy of ``softmax(logits)``
    from the same pass."""
    if _hip.use_hip(logits):
        logp, ent = _TokenStatsFn.apply(_kernel_dtype(logits), labels)
    else:
        logp, ent = _torch_stats(logits, labels, with_entropy)
    return (logp, ent) if with_entropy else logp


def token_entropy(logits):
    """Entropy of ``softmax(logits)`` per position, fp32."""
    if _hip.use_hip(logits):
        return _TokenStatsFn.apply(_kernel_dtype(logits), None)[1]
    return _torch_stats(logits, None, True)[1]
