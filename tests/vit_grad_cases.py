"""Shared by test_cpu_vit_grad.py and test_gpu_vit_grad.py: the cases of the ViT encoder's backward
(vcap_vit_encode_backward, vcap_vit_attention_backward), its fp64 oracle and the two CPU runs its bounds come from.

Oracle: torch autograd in fp64 of  sum(G * enc_out)  through oracle.vcap_oracle.encoder (plain differentiable
torch over the tensors of `sd`).  G [B, video_dim] is seeded randn.

grads_of(kind="f32") is the same autograd in float32: its distance from the oracle is what float32 arithmetic
costs on the case.  grads_of(kind="bf16") is an fp64 restatement of the encoder with bf16 (RNE) roundings where
the device's bf16 mode rounds.  Forward, straight-through x + (rne(x) - x).detach(): the frames and the patch
kernel, each LayerNorm output, the four Linear weights of a block, the stored q | k | v, the attention output and
the GELU output; inside the attention the un-normalised exp(s - max) is rounded and the output is
sum(e_r v) / sum(e_r), as the forward kernel forms it.  Backward, register_hook roundings of the gradient at the
output of each Linear before its bias is added - the row gradient that enters dx = dy . W and dW = dy^T . x as an
MFMA operand (bias gradients sum the unrounded rows) - and of the gradient at the attention output (dO); the
attention's own backward (AttnEmu.backward) is written out: P = e / sum(e) unrounded, dP = dO V^T, delta =
rowsum(P dP), dS = P (dP - delta) / 8, then dQ = rne(dS) K, dK = rne(dS)^T Q, dV = rne(P)^T dO.  With rounding off
the restatement must equal the oracle (test_cpu_vit_grad.py).

Error measure, per parameter TENSOR: err = max |g - g64| / max |g64|.  Where the oracle tensor is identically
zero the device must give exact +0 instead.  Bounds (text_grad_cases.py's factors, reused): f32 <= F32_FACTOR x
err(float32 autograd), bf16 <= BF16_FACTOR x err(bf16 emulation), both CPU quantities of the case and tensor."""
from __future__ import annotations

from dataclasses import dataclass
from functools import lru_cache
from typing import Dict, Tuple

import numpy as np
import torch
import torch.nn.functional as F

import decoder_shapes as DS
import text_grad_cases as TG
from oracle import vcap_oracle as O
from vcap.configs import ViTArch
from vcap.weights import synthetic_vit

F32_FACTOR = TG.F32_FACTOR
BF16_FACTOR = TG.BF16_FACTOR
VIDEO_DIM = 256


@dataclass(frozen=True)
class Case:
    name: str
    dim: int
    heads: int
    patch: int
    image: int
    depth: int
    B: int
    T: int
    mlp_ratio: int = 4

    @property
    def arch(self) -> ViTArch:
        return ViTArch("vit_grad_" + self.name, self.dim, self.depth, self.heads, self.patch, self.image, self.mlp_ratio)


CASES = {
    "G1": Case("G1", 128, 2, 16, 16, 2, 2, 3),               # one patch, 2 tokens; M = 12
    "G2": Case("G2", 128, 2, 8, 32, 2, 1, 1),                # BT = 1; 17 tokens: M below every tile
    "G3": Case("G3", 128, 2, 16, 224, 3, 2, 2),              # 197 tokens, M = 788: several slabs, a ragged last one
    "G4": Case("G4", 256, 4, 14, 224, 1, 1, 2),              # the only block is the CLS tail; 257 tokens
    "G5": Case("G5", 384, 6, 8, 40, 2, 3, 1, mlp_ratio=2),   # mlp_ratio 2; 384 = 1.5 tiles of 256
    # the production widths, at few rows: the reused kernels' width limits (LayerNorm backward E <= 1024, the
    # dx GEMM's N % 128, the forward LayerNorm's D % 256 vector path) at ViT-B's and ViT-L's dim and mlp
    "G6": Case("G6", 768, 12, 16, 32, 2, 1, 2),              # ViT-B width, mlp 3072; 5 tokens
    "G7": Case("G7", 1024, 16, 16, 32, 1, 1, 1),             # ViT-L width, mlp 4096; the widest served
}
# every (case, n_tail) of the accuracy test
RUNS = [(n, k) for n, c in CASES.items() for k in range(1, c.depth + 1)]
PRECISIONS = ("f32", "bf16")

ATTN_TOKENS = (1, 2, 31, 32, 33, 64, 65, 197, 257, 288)
ATTN_HEADS = (1, 3)
ATTN_FRAMES = (1, 3)


@lru_cache(maxsize=None)
def weights(name: str) -> Dict[str, np.ndarray]:
    c = CASES[name]
    return synthetic_vit(1000 + len(name) + c.dim + c.depth, c.arch, VIDEO_DIM)


@lru_cache(maxsize=None)
def frames(name: str) -> torch.Tensor:
    c = CASES[name]
    g = torch.Generator().manual_seed(17 * c.dim + c.image + c.B)
    return torch.randn(c.B, c.T, 3, c.image, c.image, generator=g, dtype=torch.float32)


@lru_cache(maxsize=None)
def grad_out(name: str) -> torch.Tensor:
    c = CASES[name]
    g = torch.Generator().manual_seed(31 * c.B + 7 * c.T + c.dim)
    return torch.randn(c.B, VIDEO_DIM, generator=g, dtype=torch.float32)


def param_names(arch: ViTArch, n_tail: int):
    """The parameters trained with the last n_tail blocks unfrozen (HipViTEncoder.param_names restated)."""
    p = "encoder.backbone."
    names = []
    if n_tail == arch.depth:
        names += [p + "cls_token", p + "pos_embed", p + "patch_embed.proj.weight", p + "patch_embed.proj.bias"]
    for i in range(arch.depth - n_tail, arch.depth):
        names += [f"{p}blocks.{i}.{k}.{w}" for k in ("norm1", "attn.qkv", "attn.proj", "norm2", "mlp.fc1", "mlp.fc2")
                  for w in ("weight", "bias")]
    return names + [p + "norm.weight", p + "norm.bias", "encoder.proj.weight", "encoder.proj.bias"]


# ---- the attention, written out ------------------------------------------------------------------------
def _ident(x):
    return x


def attention_formulas(q, k, v, dO, rnd=_ident):
    """(out, dq, dk, dv) of softmax(q k^T / 8) v per leading index, by the issue's formulas; rnd rounds the
    MFMA operands the device's bf16 mode rounds (e in the forward, P and dS in the backward)."""
    s = (q @ k.transpose(-1, -2)) / 8.0
    e = torch.exp(s - s.amax(-1, keepdim=True))
    er = rnd(e)
    out = (er @ v) / er.sum(-1, keepdim=True)
    P = e / e.sum(-1, keepdim=True)
    dP = dO @ v.transpose(-1, -2)
    delta = (P * dP).sum(-1, keepdim=True)
    dS = P * (dP - delta) / 8.0
    dSr, Pr = rnd(dS), rnd(P)
    return out, dSr @ k, dSr.transpose(-1, -2) @ q, Pr.transpose(-1, -2) @ dO


class AttnEmu(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, bf16):
        ctx.save_for_backward(q, k, v)
        ctx.bf16 = bf16
        s = (q @ k.transpose(-1, -2)) / 8.0
        e = torch.exp(s - s.amax(-1, keepdim=True))
        if bf16:
            e = DS.bf16_rne(e)
        return (e @ v) / e.sum(-1, keepdim=True)

    @staticmethod
    def backward(ctx, dO):
        q, k, v = ctx.saved_tensors
        _, dq, dk, dv = attention_formulas(q, k, v, dO, DS.bf16_rne if ctx.bf16 else _ident)
        return dq, dk, dv, None


def functional_encoder(p: Dict[str, torch.Tensor], arch: ViTArch, video: torch.Tensor, bf16: bool) -> torch.Tensor:
    """oracle.vcap_oracle.encoder restated over the parameter dict p; bf16: the device's rounding points."""
    rnd, hook = (TG._ste, TG._hook) if bf16 else (_ident, _ident)
    pre, d, H = "encoder.backbone.", arch.dim, arch.heads
    B, T = video.shape[:2]
    fr = rnd(video.reshape(B * T, *video.shape[2:]))
    g = arch.grid
    # im2col in the conv kernel's (c, i, j) order
    pat = fr.reshape(B * T, 3, g, arch.patch, g, arch.patch).permute(0, 2, 4, 1, 3, 5).reshape(B * T, g * g, -1)
    w = rnd(p[pre + "patch_embed.proj.weight"]).reshape(d, -1)
    x = hook(pat @ w.t()) + p[pre + "patch_embed.proj.bias"]
    x = torch.cat([p[pre + "cls_token"].expand(B * T, -1, -1), x], dim=1) + p[pre + "pos_embed"]
    n = x.shape[1]
    for i in range(arch.depth):
        b = f"{pre}blocks.{i}."
        h = rnd(F.layer_norm(x, (d,), p[b + "norm1.weight"], p[b + "norm1.bias"], arch.ln_eps))
        qkv = rnd(hook(h @ rnd(p[b + "attn.qkv.weight"]).t()) + p[b + "attn.qkv.bias"])
        q, k, v = qkv.reshape(B * T, n, 3, H, d // H).permute(2, 0, 3, 1, 4).unbind(0)
        a = AttnEmu.apply(q, k, v, bf16).transpose(1, 2).reshape(B * T, n, d)
        a = rnd(hook(a))
        x = x + hook(a @ rnd(p[b + "attn.proj.weight"]).t()) + p[b + "attn.proj.bias"]
        h = rnd(F.layer_norm(x, (d,), p[b + "norm2.weight"], p[b + "norm2.bias"], arch.ln_eps))
        h = rnd(F.gelu(hook(h @ rnd(p[b + "mlp.fc1.weight"]).t()) + p[b + "mlp.fc1.bias"], approximate="tanh"))
        x = x + hook(h @ rnd(p[b + "mlp.fc2.weight"]).t()) + p[b + "mlp.fc2.bias"]
    x = F.layer_norm(x, (d,), p[pre + "norm.weight"], p[pre + "norm.bias"], arch.ln_eps)
    pooled = x.reshape(B, T, n, d)[:, :, 0, :].mean(1)
    return pooled @ p["encoder.proj.weight"].t() + p["encoder.proj.bias"]


def grads_from(sd: Dict[str, np.ndarray], arch: ViTArch, video: torch.Tensor, G: torch.Tensor, kind: str,
               names=None) -> Dict[str, torch.Tensor]:
    """{state-dict name: float64 gradient of sum(G * enc_out)}.  kind: "fp64" | "f32" | "bf16" | "restated"."""
    dt = torch.float32 if kind == "f32" else torch.float64
    p = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dt).requires_grad_(True) for k, v in sd.items()}
    if kind in ("fp64", "f32"):
        out = O.encoder(p, arch, video.to(dt))
    else:
        out = functional_encoder(p, arch, video.to(dt), bf16=(kind == "bf16"))
    names = list(p) if names is None else list(names)
    gs = torch.autograd.grad((G.to(out.dtype) * out.to(dt)).sum(), [p[k] for k in names], allow_unused=True)
    return {k: (torch.zeros_like(p[k]) if g is None else g).detach().double() for k, g in zip(names, gs)}


@lru_cache(maxsize=None)
def grads_of(name: str, kind: str = "fp64") -> Dict[str, torch.Tensor]:
    c = CASES[name]
    return grads_from(weights(name), c.arch, frames(name), grad_out(name), kind)


err = TG.err
is_zero_tensor = TG.is_zero_tensor
is_plus_zero = TG.is_plus_zero
errors = TG.errors


@lru_cache(maxsize=None)
def tolerances(name: str, prec: str) -> Dict[str, float]:
    """{tensor: the device bound of the case}, from CPU runs alone.  prec: "f32" | "bf16"."""
    factor = F32_FACTOR if prec == "f32" else BF16_FACTOR
    return {k: factor * e for k, e in errors(grads_of(name, prec), grads_of(name, "fp64")).items()}


# ---- vcap_vit_attention_backward alone ------------------------------------------------------------------
def attn_inputs(tokens: int, heads: int, nframes: int, prec: str) -> Tuple[torch.Tensor, torch.Tensor]:
    """(qkv [frames*tokens, 3*64*heads], dout [frames*tokens, 64*heads]) float32, seeded; bf16: representable."""
    g = torch.Generator().manual_seed(tokens * 131 + heads * 17 + nframes)
    qkv = torch.randn(nframes * tokens, 3 * 64 * heads, generator=g, dtype=torch.float32)
    dout = torch.randn(nframes * tokens, 64 * heads, generator=g, dtype=torch.float32)
    if prec == "bf16":
        qkv, dout = DS.bf16_rne(qkv), DS.bf16_rne(dout)
    return qkv, dout


def attn_reference(qkv: torch.Tensor, dout: torch.Tensor, tokens: int, heads: int, nframes: int, dtype, rnd=_ident):
    """dqkv [frames*tokens, 3*64*heads] by attention_formulas in `dtype`."""
    D = 64 * heads
    q, k, v = qkv.to(dtype).reshape(nframes, tokens, 3, heads, 64).permute(2, 0, 3, 1, 4).unbind(0)
    dO = dout.to(dtype).reshape(nframes, tokens, heads, 64).transpose(1, 2)
    _, dq, dk, dv = attention_formulas(q, k, v, dO, rnd)
    return torch.stack([t.transpose(1, 2).reshape(nframes * tokens, D) for t in (dq, dk, dv)], 1).reshape(
        nframes * tokens, 3 * D)


def attn_bounds(tokens: int, heads: int, nframes: int, prec: str):
    """(dqkv fp64, {"dq" | "dk" | "dv": bound}): f32 against the formulas in float32, bf16 against the formulas
    with P and dS rounded."""
    qkv, dout = attn_inputs(tokens, heads, nframes, prec)
    g64 = attn_reference(qkv, dout, tokens, heads, nframes, torch.float64)
    if prec == "f32":
        ref, factor = attn_reference(qkv, dout, tokens, heads, nframes, torch.float32).double(), F32_FACTOR
    else:
        ref, factor = attn_reference(qkv, dout, tokens, heads, nframes, torch.float64, DS.bf16_rne), BF16_FACTOR
    return g64, {k: factor * err(t, t64) for k, t, t64 in zip(("dq", "dk", "dv"), split3(ref, heads), split3(g64, heads))}


def split3(dqkv: torch.Tensor, heads: int):
    D = 64 * heads
    return dqkv[:, :D], dqkv[:, D:2 * D], dqkv[:, 2 * D:]
