"""Shared by test_cpu_text_grad.py and test_gpu_text_grad.py: the cases of the text tower's backward
(vcap_text_encode_backward), its fp64 oracle and the two CPU runs its tolerances come from.

Oracle: torch autograd in fp64 of  sum(G * out)  through the reference's modules in eval mode
(text_tower_cases._double(name): nn.Embedding(padding_idx), nn.TransformerEncoder, nn.Linear) followed by the
pool, proj and normalize lines of ViTTextAlignModel.encode_text in torch.  G [B, P] is seeded randn.

grads_of(kind="f32") is the same autograd through the float32 modules: its distance from the oracle is what
float32 arithmetic costs on the case.  grads_of(kind="bf16") is an fp64 restatement of the tower in plain torch
with bf16 (RNE) roundings where the device's bf16 mode rounds: in the forward, straight-through roundings
x + (rne(x) - x).detach() of the projection weights, the GEMV operands, the stored q | k | v, the attention
output and the ReLU output; in the backward, register_hook roundings of the gradient at the output of each of
the four projections of a layer before its bias is added - the row gradient that enters dx = dy . W and
dW = dy^T . x as an MFMA operand (the bias gradient sums the unrounded rows).  With rounding off the same
restatement must equal the modules (test_cpu_text_grad.py).

Error measure, per parameter TENSOR: err = max |g - g64| / max |g64|.  in_proj_bias is one tensor (its key
third is mathematically zero: a softmax does not see a shift of its scores).  Where the oracle tensor is
identically zero the device must give exact +0 instead.

Bounds (the conventions of score_grad_cases.py): f32 <= F32_FACTOR x err(float32 autograd), bf16 <=
BF16_FACTOR x err(bf16 emulation), both CPU quantities of the case and tensor."""
from __future__ import annotations

import copy
from functools import lru_cache
from typing import Dict

import numpy as np
import torch
import torch.nn.functional as F

import decoder_shapes as DS
import text_tower_cases as TC

F32_FACTOR = 10.0
BF16_FACTOR = 3.0

Case = TC.Case

# (B, L) -> pad pattern per caption (text_tower_cases.ids_of)
SHAPES = {
    (1, 1): ("none",),
    (1, 17): ("interior",),
    (2, 16): ("none", "allpad"),                                   # M = 32: one f32 K tile, half a bf16 one
    (3, 11): ("trailing", "interior", "none"),                     # M = 33: one row into the second f32 tile
    (5, 33): ("none", "trailing", "interior", "allpad", "trailing"),   # M = 165 > V = 97 on e128
    (8, 64): ("none", "trailing", "interior", "allpad", "trailing", "none", "interior", "trailing"),  # the row limit
    (1, 4): ("allpad",),                                           # no non-pad position anywhere
}
TOWERS = ("e128", "ref", "ref_0layers")
CASES = [Case(t, B, L, p) for t in TOWERS for (B, L), p in SHAPES.items()]
REPEAT = "repeat"   # the crafted case: one id at every non-pad position of three captions (33 positions)
CRAFTED = [Case(t, 3, 12, (REPEAT,)) for t in TOWERS]
ALL_CASES = CASES + CRAFTED


def case_id(c: Case) -> str:
    return f"{c.tower}-B{c.B}-L{c.L}" + ("-repeat" if c.pads == (REPEAT,) else "-padonly" if c.pads == ("allpad",) else "")


def find(tower: str, B: int, L: int) -> Case:
    return next(c for c in CASES if (c.tower, c.B, c.L) == (tower, B, L))


@lru_cache(maxsize=None)
def ids_of(c: Case) -> np.ndarray:
    if c.pads != (REPEAT,):
        return TC.ids_of(c)
    pad = TC.PAD_ID[c.tower]
    ids = np.full((3, 12), pad + 2, np.int64)
    ids[1, 10:] = pad
    ids[2, 5] = pad
    return ids


@lru_cache(maxsize=None)
def grad_out(c: Case) -> torch.Tensor:
    """G [B, P] float32, seeded."""
    g = torch.Generator().manual_seed(31 * c.B + 7 * c.L + len(c.tower))
    return torch.randn(c.B, TC.TOWERS[c.tower][4], generator=g, dtype=torch.float32)


def pool_normalize(hidden: torch.Tensor, ids: torch.Tensor, pad_id: int, pw: torch.Tensor, pb: torch.Tensor):
    """vit_text_align.py:72-78 in torch: masked mean (count >= 1), proj, F.normalize (eps 1e-12)."""
    mask = (ids != pad_id).to(hidden.dtype)
    pooled = (hidden * mask[..., None]).sum(1) / mask.sum(1, keepdim=True).clamp(min=1.0)
    return F.normalize(pooled @ pw.t() + pb, dim=-1, eps=1e-12)


def module_out(m, ids: torch.Tensor) -> torch.Tensor:
    return pool_normalize(m.txt_enc(m.txt_emb(ids)), ids, m.pad_id, m.txt_proj.weight, m.txt_proj.bias)


def _ste(x: torch.Tensor) -> torch.Tensor:
    return x + (DS.bf16_rne(x) - x).detach()


def _hook(t: torch.Tensor) -> torch.Tensor:
    if t.requires_grad:
        t.register_hook(DS.bf16_rne)
    return t


def _ident(x):
    return x


def functional_out(p: Dict[str, torch.Tensor], ids: torch.Tensor, pad_id: int, nhead: int, bf16: bool) -> torch.Tensor:
    """The tower restated in plain torch over the parameter dict p; bf16: the device's rounding points
    (module docstring)."""
    rnd, hook = (_ste, _hook) if bf16 else (_ident, _ident)
    x = F.embedding(ids, p["txt_emb.weight"], padding_idx=pad_id)
    B, L, E = x.shape
    n_layer = 1 + max((int(k.split(".")[2]) for k in p if k.startswith("txt_enc.layers.")), default=-1)
    for i in range(n_layer):
        b = f"txt_enc.layers.{i}."
        qkv = rnd(hook(rnd(x) @ rnd(p[b + "self_attn.in_proj_weight"]).t()) + p[b + "self_attn.in_proj_bias"])
        q, k, v = (t.reshape(B, L, nhead, E // nhead).transpose(1, 2) for t in qkv.split(E, dim=-1))
        a = torch.softmax((q / 8.0) @ k.transpose(-1, -2), dim=-1) @ v
        a = rnd(a.transpose(1, 2).reshape(B, L, E))
        s1 = x + hook(a @ rnd(p[b + "self_attn.out_proj.weight"]).t()) + p[b + "self_attn.out_proj.bias"]
        x = F.layer_norm(s1, (E,), p[b + "norm1.weight"], p[b + "norm1.bias"], 1e-5)
        h = rnd(torch.relu(hook(rnd(x) @ rnd(p[b + "linear1.weight"]).t()) + p[b + "linear1.bias"]))
        s2 = x + hook(h @ rnd(p[b + "linear2.weight"]).t()) + p[b + "linear2.bias"]
        x = F.layer_norm(s2, (E,), p[b + "norm2.weight"], p[b + "norm2.bias"], 1e-5)
    return pool_normalize(x, ids, pad_id, p["txt_proj.weight"], p["txt_proj.bias"])


def _grads(scalar: torch.Tensor, named) -> Dict[str, torch.Tensor]:
    names, params = zip(*named)
    gs = torch.autograd.grad(scalar, params, allow_unused=True)
    return {k: (torch.zeros_like(p) if g is None else g).detach().double() for k, p, g in zip(names, params, gs)}


def _forward(tower: str, ids: np.ndarray, kind: str):
    """(out [B, P], [(name, parameter)]) of one run.  kind: "fp64" | "f32" | "bf16" | "restated"."""
    t = torch.from_numpy(np.asarray(ids, np.int64))
    if kind in ("fp64", "f32"):
        m = copy.deepcopy(TC._double(tower) if kind == "fp64" else TC.tower(tower)).eval()
        return module_out(m, t), list(m.named_parameters())
    p = {k: v.detach().clone().requires_grad_(True) for k, v in TC._double(tower).state_dict().items()}
    return functional_out(p, t, TC.PAD_ID[tower], TC.TOWERS[tower][1], bf16=(kind == "bf16")), list(p.items())


def grads_from(tower: str, ids: np.ndarray, G: torch.Tensor, kind: str) -> Dict[str, torch.Tensor]:
    """{state-dict name: float64 gradient of sum(G * out)}."""
    out, named = _forward(tower, ids, kind)
    return _grads((G.to(out.dtype) * out).sum(), named)


def align_loss_grads(tower: str, ids: np.ndarray, feat: torch.Tensor, vid_w: torch.Tensor, vid_b: torch.Tensor,
                     kind: str):
    """(loss, {name: float64 gradient}) of the alignment model's training loss on one batch:
    cosine_embedding_loss(normalize(vid_proj(feat)), encode_text(ids), ones), over the tower's parameters and
    vid_proj.weight / vid_proj.bias.  vid_proj runs in the run's own dtype (it is torch on every path)."""
    out, named = _forward(tower, ids, kind)
    w = vid_w.detach().to(out.dtype).clone().requires_grad_(True)
    b = vid_b.detach().to(out.dtype).clone().requires_grad_(True)
    v = F.normalize(feat.to(out.dtype) @ w.t() + b, dim=-1, eps=1e-12)
    loss = F.cosine_embedding_loss(v, out, torch.ones(v.shape[0], dtype=out.dtype))
    return float(loss), _grads(loss, named + [("vid_proj.weight", w), ("vid_proj.bias", b)])


@lru_cache(maxsize=None)
def grads_of(c: Case, kind: str = "fp64"):
    return grads_from(c.tower, ids_of(c), grad_out(c), kind)


def oracle_grads(c: Case):
    return grads_of(c, "fp64")


def err(g: torch.Tensor, g64: torch.Tensor) -> float:
    return float((g.double() - g64).abs().max() / g64.abs().max())


def is_zero_tensor(g64: torch.Tensor) -> bool:
    return bool((g64 == 0).all())


def is_plus_zero(g: torch.Tensor) -> torch.Tensor:
    """elementwise: the value is +0 (not -0, not a denormal)"""
    return (g == 0) & ~torch.signbit(g)


def errors(gs: Dict[str, torch.Tensor], g64s: Dict[str, torch.Tensor]) -> Dict[str, float]:
    """per tensor err; tensors whose oracle is identically zero are left out"""
    return {k: err(gs[k], g64) for k, g64 in g64s.items() if not is_zero_tensor(g64)}


def tolerances_from(tower: str, ids: np.ndarray, G: torch.Tensor, prec: str, g64s=None) -> Dict[str, float]:
    g64s = grads_from(tower, ids, G, "fp64") if g64s is None else g64s
    if prec == "f32":
        return {k: F32_FACTOR * e for k, e in errors(grads_from(tower, ids, G, "f32"), g64s).items()}
    return {k: BF16_FACTOR * e for k, e in errors(grads_from(tower, ids, G, "bf16"), g64s).items()}


@lru_cache(maxsize=None)
def tolerances(c: Case, prec: str):
    """{tensor: the device bound of the case}, from CPU runs alone.  prec: "f32" | "bf16"."""
    g64s = oracle_grads(c)
    ref = grads_of(c, "f32" if prec == "f32" else "bf16")
    factor = F32_FACTOR if prec == "f32" else BF16_FACTOR
    return {k: factor * e for k, e in errors(ref, g64s).items()}


def dense_embedding_grad(ids: torch.Tensor, rows: torch.Tensor, vocab: int) -> torch.Tensor:
    """The sparse-to-dense helper of the trainer (vcap.train_align.scatter_embedding_grad) restated."""
    return torch.zeros(vocab, rows.shape[1], dtype=rows.dtype).index_copy_(0, ids, rows)
