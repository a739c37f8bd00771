"""Shared by test_cpu_tail_grad.py and test_gpu_tail_grad.py: the cases of the GPT-2 tail's weight gradients
(vcap_gpt2_score_backward_tail), their fp64 oracle and the two CPU runs the tolerances come from.

Oracle: torch autograd in fp64 of score_grad_cases._objective through score_cases.masked_forward with the
12 tensors of each of the model's blocks as leaves (the sweep models have 2 layers, so one run with both
blocks as leaves serves n_tail = 1 and 2: a parameter's gradient does not depend on which other tensors are
leaves).  kind="f32" is the same autograd in float32; kind="bf16" goes through
score_grad_cases.hooked_forward with the bf16-rounded weights as leaves - its hooks round exactly the
gradients the device's weight-gradient products and bias sums read (du, dq | dk | dv and the residual
gradient where it enters the two c_proj), and its straight-through roundings make xn1, xn2, att and act
the bf16 values the device multiplies them with.

Error measure, per parameter tensor: err = max |g - g64| / max |g64|.  A tensor whose oracle is identically
zero must be exactly +0 on the device.

Shapes (B, S), rows M = B S, on the E = 128 model unless noted - the smallest at which the product kernel can
go wrong: M either side of every plausible reduction step (1, 31, 32, 33, 63, 64, 65, 129) and the row limit
512; 13 positions under no / right / interior masks; every width class at (3, 12), 2 to 64 output tiles per
axis of a product."""
from __future__ import annotations

from functools import lru_cache
from typing import Dict, List, Optional

import torch

import score_cases as SC
import score_grad_cases as G

Case = SC.Case
V = 1009
P = SC.P

ROWS = [Case(f"rows{b * s}_{b}x{s}", 128, V, b, s)
        for b, s in ((1, 1), (1, 31), (2, 16), (3, 11), (7, 9), (1, 64), (5, 13), (3, 43), (4, 128))]
MASKS = [Case(f"13_{m}", 128, V, 3, 13, m) for m in ("none", "right", "interior")]
WIDTHS = [Case(f"e{e}", e, V, 3, 12) for e in (128, 256, 384, 768, 1024)]
CASES = ROWS + MASKS + WIDTHS
IGNORED = Case("13_right_ignored", 128, V, 3, 13, "right", "ignored")
N_TAILS = (1, 2)
F32_FACTOR, BF16_FACTOR = G.F32_FACTOR, G.BF16_FACTOR

PARAMS = ("ln_1.weight", "ln_1.bias", "attn.c_attn.weight", "attn.c_attn.bias", "attn.c_proj.weight",
          "attn.c_proj.bias", "ln_2.weight", "ln_2.bias", "mlp.c_fc.weight", "mlp.c_fc.bias", "mlp.c_proj.weight",
          "mlp.c_proj.bias")


def tail_names(n_layer: int, n_tail: int) -> List[str]:
    return [f"{P}h.{i}.{k}" for i in range(n_layer - n_tail, n_layer) for k in PARAMS]


def inputs(c: Case, wmode: str = "rand"):
    return SC.embeds(c), SC.key_mask(c), G.targets(c), G.weights_w(c, wmode)


def leaves_of(sd: Dict[str, torch.Tensor], names: List[str]) -> Dict[str, torch.Tensor]:
    """A copy of sd whose `names` are fresh leaves requiring grad (the cached dict stays as it is)."""
    out = dict(sd)
    for k in names:
        out[k] = sd[k].detach().clone().requires_grad_(True)
    return out


def param_grads_of(c: Case, wmode: str, kind: str, x: Optional[torch.Tensor] = None, km=None, tg=None, w=None,
                   sd: Optional[Dict[str, torch.Tensor]] = None) -> Dict[str, torch.Tensor]:
    """{name: d objective / d parameter, float64} for every block parameter.  kind: "fp64" | "f32" | "bf16";
    x / km / tg / w replace the case's own inputs; sd replaces the kind's state dict (same dtype)."""
    ar = SC.arch(c.E, c.V)
    names = tail_names(ar.n_layer, ar.n_layer)
    if x is None:
        x, km, tg, w = inputs(c, wmode)
    if kind == "f32":
        s = leaves_of(G._sd32(c.E, c.V) if sd is None else sd, names)
        logits = SC.masked_forward(s, ar, x.float(), km)
    elif kind == "bf16":
        s = leaves_of(SC.sd64(c.E, c.V, c.gain, rounded=True) if sd is None else sd, names)
        logits = G.hooked_forward(s, ar, x.double(), km)
    else:
        s = leaves_of(SC.sd64(c.E, c.V, c.gain) if sd is None else sd, names)
        logits = SC.masked_forward(s, ar, x.double(), km)
    obj = G._objective(logits, tg, w)
    gs = torch.autograd.grad(obj, [s[k] for k in names], allow_unused=True)
    return {k: (torch.zeros_like(s[k]) if g is None else g).double() for k, g in zip(names, gs)}


@lru_cache(maxsize=None)
def oracle(c: Case, wmode: str = "rand") -> Dict[str, torch.Tensor]:
    """The fp64 gradients of the case: computed once, shared by every test, never modified."""
    return param_grads_of(c, wmode, "fp64")


def err(g: torch.Tensor, g64: torch.Tensor) -> float:
    return float((g.double() - g64).abs().max() / g64.abs().max())


@lru_cache(maxsize=None)
def tolerance(c: Case, wmode: str, prec: str) -> Dict[str, float]:
    """{name: the device bound of that tensor}, from CPU runs alone: 10 x the float32 autograd's error (fp32),
    3 x the bf16 emulation's error (bf16).  A tensor whose oracle is identically zero gets 0.0 (exact)."""
    g64 = oracle(c, wmode)
    kind, factor = ("f32", F32_FACTOR) if prec == "fp32" else ("bf16", BF16_FACTOR)
    got = param_grads_of(c, wmode, kind)
    return {k: (factor * err(got[k], g64[k]) if bool((g64[k] != 0).any()) else 0.0) for k in g64}


def check(name: str, g: torch.Tensor, g64: torch.Tensor, tol: float):
    """-> (ok, measured error).  An identically zero oracle demands exact +0."""
    if not bool((g64 != 0).any()):
        return bool(G.is_plus_zero(g).all()), 0.0
    e = err(g, g64)
    return bool(torch.isfinite(g).all()) and e <= tol, e
