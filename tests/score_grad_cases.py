"""Shared by test_cpu_score_grad.py and test_gpu_score_grad.py: the cases of the scoring call's backward
(vcap_gpt2_score_backward), its fp64 oracle and the two CPU runs its tolerances come from.

Oracle: torch autograd in fp64 of  sum over counted (b, i) of w[b, i] * lp[b, i]  through
score_cases.masked_forward (plain differentiable torch), lp = the target log-probs; w = -1 everywhere
for the NULL grad_logprob of the ABI (the gradient of nll_sum).

grad_of(kind="f32") is the same autograd in float32: its distance from the oracle is what float32 arithmetic
costs on the case.  grad_of(kind="bf16") is the fp64 run with bf16 (RNE) roundings where the device's bf16
path rounds: in the forward, masked_forward's points with a straight-through x + (rne(x) - x).detach()
and bf16-rounded weights; in the backward, register_hook roundings of the gradients that enter an MFMA
product as operands - d logits, the residual gradient entering the two c_proj^T products, du (the
gradient at the c_fc output) and dq | dk | dv.

Error measure: err(g) = max |g - g64| / max |g64| over the whole [B, S, E] gradient."""
from __future__ import annotations

from functools import lru_cache
from typing import Optional

import numpy as np
import torch
import torch.nn.functional as F

import decoder_shapes as DS
import score_cases as SC
from oracle import vcap_oracle as O

P = SC.P
Case = SC.Case

MASKS = [Case(f"13_{m}", 128, 1009, 3, 13, m) for m in ("none", "right", "interior")]
SHAPES = [
    Case("one_position", 128, 1009, 1, 1),
    Case("ctx64", 128, 1009, 2, 64),
    Case("ctx65", 128, 1009, 2, 65),
    Case("ctx70_right_edges", 128, 1009, 2, 70, "right", "edges"),
    Case("v1024", 128, 1024, 2, 12),
    Case("e256", 256, 1000, 3, 12),
    Case("e384", 384, 1000, 3, 12),
    Case("e768", 768, 1000, 3, 12),
    Case("e1024", 1024, 1000, 3, 12),
    Case("gpt2_vocab", 768, 50257, 2, 12),
    Case("rows512", 128, 1009, 4, 128),
]
CASES = MASKS + SHAPES
IGNORED = [Case("13_right_ignored", 128, 1009, 3, 13, "right", "ignored"),
           Case("13_interior_ignored", 128, 1009, 3, 13, "interior", "ignored")]
F32_FACTOR = 10.0    # device f32 err <= F32_FACTOR * err(torch CPU f32 autograd)
BF16_FACTOR = 3.0    # device bf16 err <= 3 * err(bf16 emulation): the project's bf16_tolerance convention


def targets(c: Case) -> torch.Tensor:
    """score_cases.targets; a sequence too short for its fixed edge columns (S < 8) takes seeded tokens."""
    if c.S >= 8:
        return SC.targets(c)
    g = torch.Generator().manual_seed(13 * c.E + c.B + 100 * c.S + c.V)
    return torch.randint(0, c.V, (c.B, c.S), generator=g)


def weights_w(c: Case, mode: str) -> Optional[torch.Tensor]:
    """mode "null": None (the ABI's NULL = -1 everywhere); "rand": seeded f32 [B, S] with positive and
    negative entries and every third entry (flat index % 3 == 2) exactly 0."""
    if mode == "null":
        return None
    g = torch.Generator().manual_seed(17 * c.E + 3 * c.B + 1000 * c.S + c.V)
    w = torch.randn(c.B, c.S, generator=g, dtype=torch.float32)
    flat = w.reshape(-1)
    flat[torch.arange(flat.numel()) % 3 == 2] = 0.0
    return w


def _objective(logits: torch.Tensor, targets: torch.Tensor, w: Optional[torch.Tensor]) -> torch.Tensor:
    t = targets.long()
    live = (t >= 0) & (t < logits.shape[-1])
    lp = F.log_softmax(logits, dim=-1).gather(2, t.clamp(min=0)[..., None])[..., 0]
    ww = -torch.ones_like(lp) if w is None else w.to(lp.dtype)
    return torch.where(live, ww * lp, torch.zeros_like(lp)).sum()


def _ste(x: torch.Tensor) -> torch.Tensor:
    return x + (DS.bf16_rne(x) - x).detach()


def _round_grad(t: torch.Tensor) -> torch.Tensor:
    if t.requires_grad:
        t.register_hook(DS.bf16_rne)
    return t


def hooked_forward(sd, ar, inputs_embeds, key_mask=None):
    """score_cases.masked_forward with rnd = the straight-through bf16 rounding, plus the backward's
    roundings as gradient hooks (module docstring)."""
    e, nh = ar.n_embd, ar.n_head
    hd = e // nh
    bsz, s, _ = inputs_embeds.shape
    h = inputs_embeds + sd[P + "wpe.weight"][torch.arange(0, s)].unsqueeze(0)
    mask = torch.ones(s, s, dtype=torch.bool).tril() if s > 1 else None
    if key_mask is not None:
        causal = torch.ones(s, s, dtype=torch.bool).tril()
        mask = causal[None, None] & (torch.as_tensor(key_mask) != 0)[:, None, None, :]
    for i in range(ar.n_layer):
        b = f"{P}h.{i}."
        a = _ste(F.layer_norm(h, (e,), sd[b + "ln_1.weight"], sd[b + "ln_1.bias"], ar.ln_eps))
        qkv = _round_grad(_ste(a @ sd[b + "attn.c_attn.weight"] + sd[b + "attn.c_attn.bias"]))
        q, k, v = (t.reshape(bsz, s, nh, hd).transpose(1, 2) for t in qkv.split(e, dim=2))
        att = _ste(F.scaled_dot_product_attention(q, k, v, attn_mask=mask))
        att = att.transpose(1, 2).reshape(bsz, s, e)
        h = h + _round_grad(att @ sd[b + "attn.c_proj.weight"] + sd[b + "attn.c_proj.bias"])
        m = _ste(F.layer_norm(h, (e,), sd[b + "ln_2.weight"], sd[b + "ln_2.bias"], ar.ln_eps))
        u = _round_grad(m @ sd[b + "mlp.c_fc.weight"] + sd[b + "mlp.c_fc.bias"])
        m = _ste(O._gelu_new(u))
        h = h + _round_grad(m @ sd[b + "mlp.c_proj.weight"] + sd[b + "mlp.c_proj.bias"])
    h = _ste(F.layer_norm(h, (e,), sd[P + "ln_f.weight"], sd[P + "ln_f.bias"], ar.ln_eps))
    return _round_grad(h @ sd["decoder.model.lm_head.weight"].t())


@lru_cache(maxsize=None)
def _sd32(E: int, V: int):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).float() for k, v in SC.state_dict(E, V).items()}


def grad_of(c: Case, wmode: str, kind: str, x: Optional[torch.Tensor] = None,
            km: Optional[torch.Tensor] = None, tg: Optional[torch.Tensor] = None,
            w: Optional[torch.Tensor] = None) -> torch.Tensor:
    """d objective / d embeds, float64 [B, S, E].  kind: "fp64" | "f32" | "bf16".  x / km / tg / w replace
    the case's own inputs (x None: all four come from the case)."""
    ar = SC.arch(c.E, c.V)
    if x is None:
        x, km, tg, w = SC.embeds(c), SC.key_mask(c), targets(c), weights_w(c, wmode)
    if kind == "f32":
        xe = x.float().clone().requires_grad_(True)
        logits = SC.masked_forward(_sd32(c.E, c.V), ar, xe, km)
    elif kind == "bf16":
        xe = x.double().clone().requires_grad_(True)
        logits = hooked_forward(SC.sd64(c.E, c.V, c.gain, rounded=True), ar, xe, km)
    else:
        xe = x.double().clone().requires_grad_(True)
        logits = SC.masked_forward(SC.sd64(c.E, c.V, c.gain), ar, xe, km)
    obj = _objective(logits, tg, w)
    if not obj.requires_grad:   # no counted position
        return torch.zeros_like(xe, dtype=torch.float64)
    (g,) = torch.autograd.grad(obj, xe)
    return g.double()


@lru_cache(maxsize=None)
def oracle_grad(c: Case, wmode: str = "rand") -> torch.Tensor:
    return grad_of(c, wmode, "fp64")


def err(g: torch.Tensor, g64: torch.Tensor) -> float:
    return float((g.double() - g64).abs().max() / g64.abs().max())


@lru_cache(maxsize=None)
def tolerance(c: Case, wmode: str, prec: str) -> float:
    """The device bound of the case, from CPU runs alone."""
    g64 = oracle_grad(c, wmode)
    if prec == "fp32":
        return F32_FACTOR * err(grad_of(c, wmode, "f32"), g64)
    return BF16_FACTOR * err(grad_of(c, wmode, "bf16"), g64)


def last_counted(tg: torch.Tensor, V: int) -> torch.Tensor:
    """[B]: each sequence's last counted position, -1 with none."""
    live = (tg >= 0) & (tg < V)
    idx = torch.arange(tg.shape[1])[None].expand_as(tg)
    return torch.where(live, idx, torch.full_like(idx, -1)).max(dim=1).values


def zero_positions(c: Case, km=None, tg=None) -> torch.Tensor:
    """bool [B, S]: where the gradient must be exactly +0 - after the sequence's last counted position (all
    of a sequence with none), and at a hidden key whose own target is ignored."""
    tg = targets(c) if tg is None else tg
    km = SC.key_mask(c) if km is None else km
    last = last_counted(tg, c.V)
    pos = torch.arange(c.S)[None]
    z = pos > last[:, None]
    if km is not None:
        live = (tg >= 0) & (tg < c.V)
        z = z | ((km == 0) & ~live)
    return z


def is_plus_zero(g: torch.Tensor) -> torch.Tensor:
    """elementwise: the value is +0 (not -0, not a denormal)"""
    return (g == 0) & ~torch.signbit(g)
