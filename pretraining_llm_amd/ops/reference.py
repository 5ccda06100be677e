"""Pure-PyTorch reference implementations of every fused op.

These are (a) the CPU execution path and (b) the fp32 numerics oracle that
the HIP-kernel tests compare against.  They are written for clarity, in fp32
internally, and mirror the math of the reference repo where one exists:

* attention: `src/models/attention.py:47-57` (q@k^T * hd^-1/2, causal
  masked_fill(-inf), softmax, @v) -- here batched over heads.
* layer norm: `transformer_block.py:28-31` (nn.LayerNorm, affine).
* cross entropy: `transformer.py:72-77` (F.cross_entropy, mean).
* AdamW: `train_transformer.py:126` (torch.optim.AdamW defaults).
"""
from __future__ import annotations

import math
from typing import Optional, Tuple

import torch
import torch.nn.functional as F


def layer_norm(x, weight, bias, eps: float):
    xf = x.float()
    mu = xf.mean(-1, keepdim=True)
    var = (xf - mu).pow(2).mean(-1, keepdim=True)
    y = (xf - mu) * torch.rsqrt(var + eps)
    if weight is not None:
        y = y * weight.float()
    if bias is not None:
        y = y + bias.float()
    return y.to(x.dtype)


def rms_norm(x, weight, eps: float):
    xf = x.float()
    y = xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps)
    if weight is not None:
        y = y * weight.float()
    return y.to(x.dtype)


def qk_norm(x, weight, eps: float):
    """QK-norm: RMSNorm over the head dimension of x [B,T,H,D] with one gain vector ``weight`` [D]."""
    return rms_norm(x, weight, eps)


def _bounds_visible(bounds, causal: bool, T: int, S: int):
    """[B, 1, T, S] lower limit of per-row key bounds (kv_start, q_last): kv_start[b, i] <= j (the upper limit
    j <= i is the caller's causal mask)."""
    if not causal or S != T:
        raise ValueError("attention bounds need causal attention with S == T")
    kv_start = bounds[0]
    j = torch.arange(S, device=kv_start.device)
    return (j[None, None, :] >= kv_start[:, :, None]).unsqueeze(1)


def _with_sink(s, sinks):
    """Scores [B,H,T,S] with the heads' sink logits [H] appended as one more (always visible, unscaled) column."""
    B, H, T, _ = s.shape
    return torch.cat([s, sinks.to(s.dtype).view(1, H, 1, 1).expand(B, H, T, 1)], dim=-1)


def attention(q, k, v, causal: bool = True, scale: Optional[float] = None, bounds=None, sinks=None):
    """q: [B,T,H,D], k/v: [B,S,Hkv,D] -> out [B,T,H,D], lse [B,H,T] (natural log).
    ``bounds`` = (kv_start, q_last), int [B, T] each: query i sees keys kv_start[b, i] <= j <= i only.
    ``sinks`` [H]: attention sinks, one logit per query head that joins every row's softmax denominator (not
    multiplied by ``scale``, visible whatever the masks) and carries no value; ``lse`` includes it."""
    B, T, H, D = q.shape
    S, Hkv = k.shape[1], k.shape[2]
    scale = scale if scale is not None else 1.0 / math.sqrt(D)
    qf = q.float().transpose(1, 2)                      # B,H,T,D
    kf = k.float().transpose(1, 2)
    vf = v.float().transpose(1, 2)
    if Hkv != H:
        rep = H // Hkv
        kf = kf.repeat_interleave(rep, dim=1)
        vf = vf.repeat_interleave(rep, dim=1)
    s = torch.matmul(qf, kf.transpose(-1, -2)) * scale  # B,H,T,S
    if causal:
        # queries are aligned to the END of the key sequence (decode/KV-cache convention)
        off = S - T
        mask = torch.ones(T, S, dtype=torch.bool, device=q.device).tril(diagonal=off)
        s = s.masked_fill(~mask, float("-inf"))
    if bounds is not None:
        s = s.masked_fill(~_bounds_visible(bounds, causal, T, S), float("-inf"))
    lse = torch.logsumexp(s if sinks is None else _with_sink(s, sinks), dim=-1)  # B,H,T
    p = torch.exp(s - lse.unsqueeze(-1))
    o = torch.matmul(p, vf)                             # B,H,T,D
    return o.transpose(1, 2).to(q.dtype), lse


def attention_bwd(do, q, k, v, o, lse, causal: bool = True, scale: Optional[float] = None, bounds=None, sinks=None):
    """Flash-style backward of one attention block given the row statistics of the WHOLE
    softmax (``lse`` [B,H,T], natural log, and the final output ``o``), so partial key
    blocks (ring / context parallel) produce exact partial gradients.
    Returns fp32 (dq [B,T,H,D], dk [B,S,Hkv,D], dv [B,S,Hkv,D]).  With ``sinks`` [H] (``lse`` then includes the
    sink) also dsinks [H]: the sink's value row is zero, so dS_sink = -p_sink delta and
    dsinks[h] = -sum_{b,i} exp(sinks[h] - lse[b,h,i]) delta[b,h,i]; dq / dk / dv need nothing else."""
    B, T, H, D = q.shape
    S, Hkv = k.shape[1], k.shape[2]
    scale = scale if scale is not None else 1.0 / math.sqrt(D)
    rep = H // Hkv
    qf, dof, of = (t.float().transpose(1, 2) for t in (q, do, o))            # B,H,T,D
    kf = k.float().transpose(1, 2).repeat_interleave(rep, dim=1)             # B,H,S,D
    vf = v.float().transpose(1, 2).repeat_interleave(rep, dim=1)
    s = torch.matmul(qf, kf.transpose(-1, -2)) * scale
    if causal:
        mask = torch.ones(T, S, dtype=torch.bool, device=q.device).tril(diagonal=S - T)
        s = s.masked_fill(~mask, float("-inf"))
    if bounds is not None:
        s = s.masked_fill(~_bounds_visible(bounds, causal, T, S), float("-inf"))
    p = torch.exp(s - lse.float().unsqueeze(-1))
    dv = torch.matmul(p.transpose(-1, -2), dof)                              # B,H,S,D
    dp = torch.matmul(dof, vf.transpose(-1, -2))
    delta = (dof * of).sum(-1, keepdim=True)
    ds = p * (dp - delta)
    dq = torch.matmul(ds, kf) * scale
    dk = torch.matmul(ds.transpose(-1, -2), qf) * scale
    dk = dk.view(B, Hkv, rep, S, D).sum(2)
    dv = dv.view(B, Hkv, rep, S, D).sum(2)
    if sinks is not None:
        dsinks = -(torch.exp(sinks.float().view(1, H, 1) - lse.float()) * delta.squeeze(-1)).sum((0, 2))
        return dq.transpose(1, 2), dk.transpose(1, 2), dv.transpose(1, 2), dsinks
    return dq.transpose(1, 2), dk.transpose(1, 2), dv.transpose(1, 2)


def quantize_rows_fp8(w):
    """Per-row e4m3fn quantisation (csrc/quant_fp8.hip): scale = amax / 448 (1 for an all-zero row), codes =
    nearest e4m3fn value of w / scale (true divisions, ties to even) -> (uint8 [N, K], fp32 [N])."""
    wf = w.detach().float()
    amax = wf.abs().amax(dim=1)
    scale = torch.where(amax == 0, torch.ones_like(amax), amax / 448.0)
    q = (wf / scale[:, None]).to(torch.float8_e4m3fn)
    return q.view(torch.uint8), scale


def dequantize_fp8(q, scale):
    """fp32 [N, K]: the e4m3fn value of each code times its row's scale."""
    return q.view(torch.float8_e4m3fn).to(torch.float32) * scale[:, None].to(torch.float32)


def linear_fp8(x, q, scale, bias=None):
    """x dequantize(q, scale)^T + bias in fp32, rounded once to x.dtype."""
    y = x.float() @ dequantize_fp8(q, scale).t()
    if bias is not None:
        y = y + bias.float()
    return y.to(x.dtype)


def gelu_tanh(x):
    return F.gelu(x.float(), approximate="tanh").to(x.dtype)


def swiglu(gate_up):
    """gate_up [..., 2F] laid out [gate | up] -> silu(gate) * up  [..., F]."""
    g, u = gate_up.float().chunk(2, dim=-1)
    return (F.silu(g) * u).to(gate_up.dtype)


def relu(x):
    return torch.relu(x)


def rope_cos_sin(seq_len: int, head_dim: int, theta: float = 10000.0, device=None, offset: int = 0):
    inv = 1.0 / (theta ** (torch.arange(0, head_dim, 2, dtype=torch.float64, device=device) / head_dim))
    t = torch.arange(offset, offset + seq_len, dtype=torch.float64, device=device)
    freqs = torch.outer(t, inv)                         # T, D/2
    return freqs.cos().float(), freqs.sin().float()


def rope(x, cos, sin):
    """Rotate-half (GPT-NeoX / Llama HF) convention on x [B,T,H,D]; cos/sin [T, D/2]."""
    D = x.shape[-1]
    xf = x.float()
    x1, x2 = xf[..., : D // 2], xf[..., D // 2:]
    c = cos[None, :, None, :]
    s = sin[None, :, None, :]
    out = torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], dim=-1)
    return out.to(x.dtype)


def softcap(logits, cap):
    """``cap * tanh(logits / cap)`` in fp32, returned in the input's dtype (``cap`` None: unchanged)."""
    if cap is None:
        return logits
    return (torch.tanh(logits.float() / cap) * cap).to(logits.dtype)


def cross_entropy(logits, targets, ignore_index: int = -100, z_loss: float = 0.0, softcap=None, z_out=None):
    """Mean CE of ``softcap * tanh(logits / softcap)`` plus ``z_loss * logsumexp^2`` averaged over the valid rows.
    ``z_out``: a 1-element fp32 tensor that receives the z term (the second summand) without a graph."""
    y = logits.float()
    if softcap is not None:
        y = torch.tanh(y / softcap) * softcap  # fp32, not rounded back to the logits' dtype
    loss = F.cross_entropy(y, targets.long(), ignore_index=ignore_index)
    if z_loss:
        valid = (targets != ignore_index).to(y.dtype)
        zt = z_loss * (torch.logsumexp(y, -1).square() * valid).sum() / valid.sum().clamp_min(1)
        if z_out is not None:
            z_out.copy_(zt.detach().reshape(1))
        loss = loss + zt
    return loss


def embedding(idx, wte, wpe=None, pos_offset: int = 0):
    x = F.embedding(idx, wte)
    if wpe is not None:
        T = idx.shape[1]
        x = x + wpe[pos_offset:pos_offset + T].unsqueeze(0)
    return x


@torch.no_grad()
def adamw_(param, grad, exp_avg, exp_avg_sq, lr, beta1, beta2, eps, weight_decay, step,
           master: Optional[torch.Tensor] = None, grad_scale: float = 1.0):
    """In-place AdamW (torch.optim.AdamW semantics, decoupled weight decay)."""
    p = master if master is not None else param
    g = grad.float() * grad_scale
    p.mul_(1.0 - lr * weight_decay)
    exp_avg.lerp_(g, 1.0 - beta1)
    exp_avg_sq.mul_(beta2).addcmul_(g, g, value=1.0 - beta2)
    bc1 = 1.0 - beta1 ** step
    bc2 = 1.0 - beta2 ** step
    denom = (exp_avg_sq.sqrt() / math.sqrt(bc2)).add_(eps)
    p.addcdiv_(exp_avg, denom, value=-lr / bc1)
    if master is not None:
        param.copy_(master.to(param.dtype))
