"""Shared by test_cpu_attention_edges.py and test_gpu_attention_edges.py: ViT attention inputs on which a key
masking or a key / row indexing fault moves the output by O(|v|), not by a fraction of a bf16 tolerance.

Random q / k / v with an absolute tolerance of 3e-2 (tests/test_gpu_ops.py) and the end-to-end encoder checks
cannot tell a padding key admitted to a 197-key softmax from rounding (tests/test_cpu_encoder_shapes.py prints
the measured table).  Here every q / k entry is 0, +-1 or +-2 - exact in bf16, fp16 and f32, so the scores are
exact integers / 8 - and v is random, rounded to the element type:

  1 "dominant": every query scores +8 on key j and -8 on every other key (q = c, k_j = +c, the others -c, c a
     +-1 vector per (frame, head)); j runs over dominant_keys(N).  The output is v_j to within exp(-16) N: a
     dropped, shifted or doubled key changes it by O(|v|).
  2 "uniform": every key scores -8: the output is the mean of v.  An admitted padding key (score 0) would take
     1 / (1 + N exp(-8)) of the weight, 0.94 at N = 197.
  3 "permutation": q_i = 2 code(pi(i)), pi(i) = (7 i + 3) mod N, k_j = code(j), code a random +-1 vector: the
     match scores 16, the rest spread with std 2, so every output row depends on its own row index and on one
     particular key.

The fused kernel gets the same q / k from xn, W: the two codes sit in columns [0, 64) and [64, 128) of xn, W_q
and W_k are signed selections of them (entries 0, +-1, +-2; one sign vector per head), W_v is random.

Reference: fp64 softmax(q k^T / 8) v.  Tolerance of a 2-byte type: 3 x max |emulated - fp64|, the emulation
rounding the unnormalised P and the output to the type as the kernels do (tests/encoder_shapes.py, module
docstring); f32: 1e-5."""
from __future__ import annotations

from typing import Optional

import torch

from encoder_shapes import ROUND, generic_attention

WINDOW_EDGES = (1, 2, 17, 32, 193, 197, 208, 209, 224, 257, 272, 273, 288)
FP16_MORE = (33, 64, 65, 128, 129, 192, 225, 256)           # the generic kernel's key paddings, both sides
TOKENS = {"bf16": WINDOW_EDGES, "fp32": WINDOW_EDGES, "fp16": tuple(sorted(WINDOW_EDGES + FP16_MORE))}
MX_TOKENS = (2, 17, 32, 197, 208, 209, 224, 257, 272, 273, 288)   # two or three per instance of the MXFP8-out kernel
MX_HEADS = 4
FUSED_TOKENS = (193, 197, 208, 257, 272)
F32_TOL = 1e-5
TORCH = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}
PATTERNS = ("dominant", "uniform", "permutation")


def dominant_keys(n: int):
    return sorted({j for j in (0, 1, 15, 16, 31, 32, n - 17, n - 16, n - 2, n - 1) if 0 <= j < n})


def _signs(shape, gen):
    return torch.randint(0, 2, shape, generator=gen).double() * 2 - 1


def _round_to(prec: str, x: torch.Tensor) -> torch.Tensor:
    return x.to(torch.float32).to(TORCH[prec]).double()


def code_rows(pattern: str, n: int, frames: int, j: Optional[int], seed: int):
    """-> (qc, kc) float64 [frames, n, 64]: the q- and k-side codes before the per-head sign and the factor on
    q (1, or 2 for the permutation pattern)."""
    g = torch.Generator().manual_seed(seed)
    if pattern == "permutation":
        code = _signs((frames, n, 64), g)
        pi = (7 * torch.arange(n) + 3) % n
        return code[:, pi], code
    c = _signs((frames, 1, 64), g)
    kc = -c.expand(frames, n, 64).clone()
    if pattern == "dominant":
        kc[:, j] = c[:, 0]
    return c.expand(frames, n, 64).clone(), kc


def qfactor(pattern: str) -> float:
    return 2.0 if pattern == "permutation" else 1.0


def qkv(pattern: str, prec: str, n: int, frames: int = 2, heads: int = 2, j: Optional[int] = None, seed: int = 0):
    """-> float64 [frames, n, 3, heads, 64] (the layout of a [frames * n, 3 * heads * 64] qkv buffer): q / k of
    the pattern, v = randn rounded to the type."""
    qc, kc = code_rows(pattern, n, frames, j, 1000 * n + seed)
    g = torch.Generator().manual_seed(77 * n + 13 * heads + seed)
    s = _signs((1, 1, heads, 64), g)
    out = torch.empty(frames, n, 3, heads, 64, dtype=torch.float64)
    out[:, :, 0] = qfactor(pattern) * qc[:, :, None] * s
    out[:, :, 1] = kc[:, :, None] * s
    out[:, :, 2] = _round_to(prec, torch.randn(frames, n, heads, 64, generator=g))
    return out


def fused_inputs(pattern: str, prec: str, n: int, frames: int = 2, heads: int = 2, j: Optional[int] = None,
                 seed: int = 0):
    """-> (xn [frames * n, D], w [3 D, D], b [3 D], qk [frames, n, 2, heads, 64]) float64, D = heads * 64 >= 128:
    LayerNorm-output rows, QKV weight and bias from which the QKV projection gives exactly the q / k of
    qkv(...) (returned as qk) and a random v."""
    d = heads * 64
    assert heads >= 2
    qc, kc = code_rows(pattern, n, frames, j, 1000 * n + seed)
    g = torch.Generator().manual_seed(77 * n + 13 * heads + seed)
    s = _signs((heads, 64), g)
    xn = torch.zeros(frames, n, d, dtype=torch.float64)
    xn[..., :64], xn[..., 64:128] = qc, kc
    w = torch.zeros(3 * d, d, dtype=torch.float64)
    eye = torch.arange(64)
    for h in range(heads):
        w[h * 64 + eye, eye] = qfactor(pattern) * s[h]
        w[d + h * 64 + eye, 64 + eye] = s[h]
    w[2 * d:] = _round_to(prec, 0.05 * torch.randn(d, d, generator=g))
    b = torch.zeros(3 * d, dtype=torch.float64)
    b[2 * d:] = (0.05 * torch.randn(d, generator=g)).float().double()
    qk = torch.stack([qfactor(pattern) * qc[:, :, None] * s, kc[:, :, None] * s], dim=2)
    return xn.reshape(frames * n, d), w, b, qk


def attend(x: torch.Tensor, mode: str = "fp64", generic: bool = False, fault: Optional[str] = None) -> torch.Tensor:
    """x [frames, n, 3, heads, 64] float64 -> softmax(q k^T / 8) v as [frames, n, heads * 64] float64.
    mode "bf16" / "fp16": the unnormalised P and the output rounded to the type; the row sum is taken over the
    rounded P, or (generic: the fp16 kernel outside the frame windows) over the unrounded one.
    fault "drop_key": the last key left out; "pad_key": one extra key with k = v = 0."""
    rnd = ROUND[mode]
    q, k, v = x.permute(2, 0, 3, 1, 4).unbind(0)          # [frames, heads, n, 64]
    if fault == "drop_key":
        k, v = k[:, :, :-1], v[:, :, :-1]
    if fault == "pad_key":
        z = torch.zeros_like(k[:, :, :1])
        k, v = torch.cat([k, z], 2), torch.cat([v, z], 2)
    s = q @ k.transpose(-1, -2) / 8.0
    e = torch.exp(s - s.max(-1, keepdim=True).values)
    p = rnd(e)
    den = (e if generic else p).sum(-1, keepdim=True)
    o = rnd((p @ v) / den)
    return o.transpose(1, 2).reshape(x.shape[0], x.shape[1], -1)


def tolerance(x: torch.Tensor, prec: str, ref: Optional[torch.Tensor] = None) -> float:
    """f32: 1e-5.  bf16 / fp16: 3 x max |emulated - fp64| on these inputs (module docstring)."""
    if prec == "fp32":
        return F32_TOL
    ref = attend(x) if ref is None else ref
    return 3.0 * float((attend(x, prec, generic_attention(prec, x.shape[1])) - ref).abs().max())


def variants(n: int):
    """(pattern, j) of every input the tests build at n tokens."""
    return [("dominant", j) for j in dominant_keys(n)] + [("uniform", None), ("permutation", None)]
