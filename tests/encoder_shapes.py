"""Shared by test_cpu_encoder_shapes.py and test_gpu_encoder_shapes.py: the synthetic ViT encoders of the
shape sweep (architectures, seeds, q / k scales, frames, prefixes), the fp64 oracle run, and a second CPU
forward that is the fp64 oracle with round-to-nearest-even bf16 (or fp16) applied exactly where the kernels
round.  The same forward takes the injected faults of the "is the net tight enough" table and records the
attention score statistics; with the identity as rounding it reproduces oracle.encoder.

Where the 2-byte encoder rounds to its element type T (csrc/runtime_vit.hip vcap_vit_encode and the kernels
it launches):
  * vcap_patchify*_kernel stores the im2col patches as T; the patch-embed weight is T in HBM;
  * vcap_layernorm_kernel stores norm1 / norm2 as T (csrc/layernorm.hip);
  * the QKV GEMM stores q / k / v as T (the fused kernel writes the same values into its LDS images);
  * attention (csrc/vit_attention.hip): scores, max and exp stay f32; the unnormalised P = exp(s - max) is
    packed to T for the PV MFMA, and the output (sum P v) / rowsum is stored as T.  The LDS-DMA kernel
    (N <= 32, 193..224, 257..288, and the fused kernels) takes rowsum from the rounded P (a ones operand in
    the PV MFMA); the generic kernel (fp16 at the other token counts) sums the unrounded P;
  * the fc1 epilogue stores GELU(acc + bias) as T;
  * the block weights (qkv, attn-proj, fc1, fc2) are T in HBM.
fp16 adds the Autocast<f16_t> points of csrc/vcap_common.h - every Linear returns fp16 under torch.autocast:
accumulator + bias is rounded to fp16 in the patch-embed GEMM (before pos is added), in attn-proj and fc2
(before the f32 residual add; after the split-K sum in the CLS tail) and in fc1 before the GELU - and the
H16 head (csrc/vit_misc.hip vcap_vit_head_kernel<true>): the pooled row and encoder.proj's weight are
rounded on the way in, the embedding on the way out.
The residual stream, the biases, pos, cls, the final LayerNorm, the temporal mean, and the prefix
normalisation + mapper stay f32 (unrounded here).

Mode "fp8" (precision="fp8": dtype MXFP8 in the descriptor) takes the subset `mx_gemms` of the block GEMMs that
run in MXFP8; the others, the patch embedding and the QK^T / PV products are the bf16 encoder's.  MXFP8 rounding
(mxq below: per 32 consecutive elements one scale 2^(floor(log2 max) - 7), elements to e4m3 nearest-even):
  * patches, the patch-embed weight, q / k / v and P are bf16 as above;
  * vcap_layernorm_mx_kernel stores norm1 as MXFP8 when qkv is an MXFP8 GEMM, norm2 when fc1 is (else bf16);
  * vcap_vit_attention_mx writes the attention output as MXFP8 when attn-proj is an MXFP8 GEMM: per 32 of a
    head's 64 dims, quantised from the f32 value (sum P v) / rowsum, not from its bf16 rounding;
  * the fc1 epilogue stores GELU(acc + bias) as MXFP8, from the f32 value, when fc1 and fc2 are both MXFP8; an
    MXFP8 fc2 after a bf16 fc1 quantises the bf16 activation (vcap_mx_quantize);
  * the weights of an MXFP8 GEMM are mx_quantize of the f32 weights (not of their bf16 rounding).
With no GEMM selected the mode is the bf16 emulation exactly (asserted in test_cpu_encoder_shapes.py).  `kflip`
runs every matrix product with its K axis reversed: a second f32 summation order for the bound on
|gpu - emulated|.  Fault "fc2_scale" (fp8 only): K-block 0 of the last block's fc2 activation doubled - one
scale byte off by one."""
from __future__ import annotations

import math
from dataclasses import dataclass
from functools import lru_cache
from typing import Dict, Optional, Tuple

import numpy as np
import torch
import torch.nn.functional as F

from oracle import vcap_oracle as O
from vcap import weights
from vcap.configs import ViTArch

P = "encoder.backbone."
FP32_TOL = 1e-4                       # the project's fp32 encoder bar (tests/test_gpu_parity.py)
LN_SCALE, IN_WEIGHT = 0.6, 0.4        # the engine's prefix normalisation (HipPrefix defaults)
PRECS = ("fp32", "bf16", "fp16")
MX_GEMMS = ("qkv", "proj", "fc1", "fc2")      # HipViTEncoder.MX_GEMMS
FAULTS = ("drop_key", "pad_key", "row_tile", "pos_late", "fc2_ktile", "frame_missing")
ASSERTED_16 = ("fc2_ktile", "frame_missing")   # the faults a half-precision end-to-end check must see
SCORE_STD, MAXP_MEDIAN = (1.0, 4.0), (0.05, 0.9)


@dataclass(frozen=True)
class Case:
    cid: int
    dim: int
    heads: int
    patch: int
    image: int
    depth: int
    B: int
    T: int
    what: str
    mlp_ratio: int = 4
    video_dim: int = 256
    prefix: Optional[Tuple[int, int]] = None    # (prefix_len, n_embd) of the mapper, None: encoder output only
    precs: Tuple[str, ...] = PRECS
    seed: int = 0                                # 0: 100 + cid
    qk: float = 0.0                              # 0: sqrt(2 / (4e-4 dim)), see qk_scale()

    @property
    def arch(self) -> ViTArch:
        return ViTArch(f"sweep_{self.cid}", self.dim, self.depth, self.heads, self.patch, self.image, self.mlp_ratio)

    @property
    def tokens(self) -> int:
        return self.arch.tokens

    @property
    def name(self) -> str:
        return f"c{self.cid:02d}-d{self.dim}-n{self.tokens}-l{self.depth}-{self.B}x{self.T}"


CASES = (
    # qk: with two keys the scores of block 1 spread more than block 0's (std 1.75 / 2.75 at the formula's 8.84,
    # median row max-probability 0.91 in block 1); 7.5 brings both blocks inside the asserted ranges
    Case(1, 64, 1, 16, 16, 2, 2, 3, "one patch; bf16 K = 64 (one K-tile); LN with one column per lane", qk=7.5),
    # seed: with 102 and 1102 the fp16 bound on |gpu - emulated| (8.6e-4, 9.4e-4) is below one fp16 ulp of the
    # outputs in [1, 2) (9.8e-4), and the emulation's own f32-arithmetic noise carries outputs across rounding
    # ties (fp16_tie_margin below); 2102 is the next seed tried, chosen on the CPU alone
    Case(2, 64, 1, 8, 32, 2, 2, 3, "kt = 2 attention kernels, unfused bf16 incl. CLS-only; patchify8 at p = 8", seed=2102),
    Case(3, 320, 5, 8, 40, 2, 1, 1, "BT = 1; LN scalar path; mlp_ratio = 2", mlp_ratio=2),
    Case(4, 128, 2, 16, 224, 3, 2, 3, "anchor to a golden-pinned width, three blocks", prefix=(4, 128)),
    Case(5, 192, 3, 16, 224, 1, 2, 3, "the only block is the CLS tail"),
    Case(6, 192, 3, 16, 224, 2, 2, 4, "BT = 8: the fused kernel's XCD order; fc2 split 4"),
    Case(7, 384, 6, 16, 224, 2, 2, 3, "ViT-S/16; proj split 2, fc2 split 8; video_dim = 100; prefix 3 x 40 (MO = 120)",
         video_dim=100, prefix=(3, 40)),
    Case(8, 512, 8, 14, 224, 2, 1, 3, "the fused L kernel at H = 8; LN nv = 2; scalar patchify"),
    Case(9, 1024, 16, 16, 224, 2, 1, 2, "ViT-L/16"),
    Case(10, 768, 12, 16, 224, 2, 1, 2, "anchor"),
    Case(11, 128, 2, 32, 224, 2, 2, 3, "fp16 only: generic kernel KT = 4; patchify8 at p = 32", precs=("fp16",)),
    Case(12, 128, 2, 8, 64, 2, 2, 3, "fp16 only: KT = 8 (one key past 64)", precs=("fp16",)),
    Case(13, 128, 2, 16, 240, 2, 1, 2, "fp16 only: KT = 16", precs=("fp16",)),
)
BY_ID = {c.cid: c for c in CASES}
RUNS = [(c.cid, p) for c in CASES for p in c.precs]
# The fp8 sweep: its own cases and run list (the table above and its assertions are untouched).  B * T <= 8.
FP8_CASES = (
    Case(21, 256, 4, 16, 16, 2, 2, 3, "fp8: M = 12, a 6-row CLS tail; LN-MX nv = 1", precs=("fp8",), qk=7.5),
    Case(22, 256, 4, 8, 32, 1, 2, 2, "fp8: the only block is the CLS tail", precs=("fp8",)),
    Case(23, 256, 4, 16, 224, 2, 1, 2, "fp8: M = 394, two 256-row scale groups; the per-GEMM mixes", precs=("fp8",)),
    # B = 2 so that the last row encoded alone has fewer 256-row scale groups than the batch: 5 -> 3 at 257 tokens
    # (M = 1028 -> 514), 4 -> 2 at 197 tokens (788 -> 394).  Case 23 is the issue's 1 x 2: its row alone IS the batch.
    Case(24, 512, 8, 14, 224, 2, 2, 2, "fp8: case 8's architecture, 257 tokens; LN-MX nv = 2", precs=("fp8",)),
    Case(25, 768, 12, 16, 224, 2, 2, 2, "fp8: case 10's architecture; LN-MX nv = 3", precs=("fp8",)),
    Case(26, 1024, 16, 16, 224, 2, 2, 2, "fp8: case 9's architecture; LN-MX nv = 4", precs=("fp8",)),
)
BY_ID.update({c.cid: c for c in FP8_CASES})
FP8_MIXES = (("qkv",), ("proj",), ("fc1",), ("fc2",), ("qkv", "proj"))
FP8_RUNS = [(c.cid, MX_GEMMS) for c in FP8_CASES] + [(23, m) for m in FP8_MIXES]


def fp8_run_id(run) -> str:
    return f"{BY_ID[run[0]].name}-fp8-{'+'.join(run[1]) if run[1] != MX_GEMMS else 'all'}"
# (case, precision) pairs the descriptor check refuses (tests/test_cpu_abi_refusals.py pins code and text)
REFUSED = [(c.cid, p) for c in CASES for p in ("fp32", "bf16") if p not in c.precs]


def run_id(run) -> str:
    return f"{BY_ID[run[0]].name}-{run[1]}"


def qk_scale(c: Case) -> float:
    """The factor on the q and k rows of every block's attn.qkv.weight.  The synthetic init (weights
    normal(0.02), LayerNorm output of unit variance) gives q, k entries of variance 4e-4 dim, so the scaled
    scores q.k / 8 have std about 4e-4 dim f^2: f = sqrt(2 / (4e-4 dim)) aims at std 2, where the softmax is
    neither uniform nor one-hot.  test_cpu_encoder_shapes.py asserts the outcome per block."""
    return c.qk or math.sqrt(2.0 / (4e-4 * c.dim))


@lru_cache(maxsize=None)
def state_dict(cid: int) -> Dict[str, np.ndarray]:
    """f32 numpy state dict of the case (what HipViTEncoder / HipPrefix load): synthetic_vit, the q / k rows
    scaled, and - for a case with a prefix - a mapper with torch's Linear default init."""
    c = BY_ID[cid]
    sd = dict(weights.synthetic_vit(c.seed or 100 + cid, c.arch, c.video_dim))
    f = np.float32(qk_scale(c))
    for i in range(c.depth):
        key = f"{P}blocks.{i}.attn.qkv.weight"
        w = sd[key].copy()
        w[:2 * c.dim] *= f
        sd[key] = w
    if c.prefix:
        g = torch.Generator().manual_seed(7000 + cid)
        mo, bound = c.prefix[0] * c.prefix[1], 1.0 / math.sqrt(c.video_dim)
        sd["decoder.mapper.0.weight"] = ((torch.rand(mo, c.video_dim, generator=g) * 2 - 1) * bound).numpy()
        sd["decoder.mapper.0.bias"] = ((torch.rand(mo, generator=g) * 2 - 1) * bound).numpy()
    return sd


@lru_cache(maxsize=None)
def video(cid: int) -> torch.Tensor:
    """[B, T, 3, image, image] f32 standard-normal frames (the value range of ImageNet-normalised pixels)
    from a fixed CPU generator: the same frames on every machine."""
    c = BY_ID[cid]
    g = torch.Generator().manual_seed(9000 + cid)
    return torch.randn(c.B, c.T, 3, c.image, c.image, generator=g, dtype=torch.float32)


def _rne(dtype):
    def rnd(x: torch.Tensor) -> torch.Tensor:
        """Round to the nearest value of the type (ties to even; fp16 subnormals kept, overflow -> inf),
        returned in x's dtype.  f64 -> f32 -> T rounds twice; a double-rounding flip needs the f64 value
        within 2^-29 relative of a T tie, which an f32 accumulator cannot resolve either."""
        return x.to(torch.float32).to(dtype).to(x.dtype)
    return rnd


def _ident(x):
    return x


def mxq(x: torch.Tensor) -> torch.Tensor:
    """MXFP8 quantise-dequantise along the last axis (blocks of 32), in x's dtype: oracle.mx_quantize's rule."""
    shp = x.shape
    b = x.reshape(*shp[:-1], shp[-1] // 32, 32)
    _, e = torch.frexp(b.abs().amax(-1, keepdim=True))           # max = m 2^e, m in [0.5, 1): floor(log2) = e - 1
    scale = torch.ldexp(torch.ones_like(b[..., :1]), (e - 8).clamp(min=-127))
    return ((b / scale).to(torch.float32).to(torch.float8_e4m3fn).to(x.dtype) * scale).reshape(shp)


ROUND = {"fp64": _ident, "bf16": _rne(torch.bfloat16), "fp16": _rne(torch.float16)}
_MX_KEY = {"qkv": "attn.qkv.weight", "proj": "attn.proj.weight", "fc1": "mlp.fc1.weight", "fc2": "mlp.fc2.weight"}
_MATS = ("attn.qkv.weight", "attn.proj.weight", "mlp.fc1.weight", "mlp.fc2.weight", "patch_embed.proj.weight")


@lru_cache(maxsize=None)
def sd64(cid: int, mode: str = "fp64") -> Dict[str, torch.Tensor]:
    """The state dict as float64 tensors; mode bf16 / fp16: the weights the device holds in that type on its
    grid (patch-embed and block matrices; fp16 also encoder.proj.weight, rounded by the H16 head)."""
    rnd = ROUND[mode]
    out = {}
    for k, v in state_dict(cid).items():
        t = torch.from_numpy(np.ascontiguousarray(v)).double()
        if k.endswith(_MATS) or (mode == "fp16" and k == "encoder.proj.weight"):
            t = rnd(t)
        out[k] = t
    return out


@lru_cache(maxsize=None)
def sd64_fp8(cid: int, mx_gemms: Tuple[str, ...]) -> Dict[str, torch.Tensor]:
    """sd64(cid, "bf16") with the weights of the MXFP8 GEMMs replaced by mx_quantize of the f32 weights."""
    out = dict(sd64(cid, "bf16"))
    raw = state_dict(cid)
    for i in range(BY_ID[cid].depth):
        for g in mx_gemms:
            k = f"{P}blocks.{i}.{_MX_KEY[g]}"
            out[k] = mxq(torch.from_numpy(np.ascontiguousarray(raw[k])).double())
    return out


def generic_attention(mode: str, tokens: int) -> bool:
    """Whether vcap_vit_attention_dispatch gives this (precision, token count) the generic kernel, whose
    row sum is taken over the unrounded P (module docstring)."""
    kt = 2 * ((tokens + 31) // 32)
    return mode == "fp16" and kt not in (2, 14, 18)


def forward(cid: int, mode: str = "fp64", fault: Optional[str] = None, stats: Optional[list] = None,
            frames: Optional[torch.Tensor] = None, arith: torch.dtype = torch.float64, raw: Optional[list] = None,
            mx_gemms: Optional[Tuple[str, ...]] = None, kflip: bool = False):
    """-> (enc_out [B, video_dim], prefix [B, P, E] or None), float64.

    mode "fp64": no rounding (oracle.encoder + prefix_norm + mapper, asserted on the CPU); "bf16" / "fp16":
    the roundings of the module docstring.  `fault` injects one of FAULTS.  `stats`, a list, receives per
    block (std of the scaled scores q.k / 8, median over rows of the row's largest probability).
    `frames` [b, T, 3, H, W] replaces the case's video.  `arith` = torch.float32 runs the same forward with f32
    arithmetic between the roundings (what any kernel with f32 accumulators does, in another order).  `raw`, a
    list, receives encoder.proj's output before the fp16 head rounds it.  mode "fp8": `mx_gemms` (default all
    four) run in MXFP8, the rest as bf16; `kflip`: every matrix product sums its K axis in reverse."""
    c = BY_ID[cid]
    mxg = () if mode != "fp8" else MX_GEMMS if mx_gemms is None else tuple(g for g in MX_GEMMS if g in mx_gemms)
    if mode == "fp8":
        mode = "bf16"
        sd0 = sd64_fp8(cid, mxg)
    else:
        sd0 = sd64(cid, mode)
    ar, rnd = c.arch, ROUND[mode]
    sd = sd0 if arith == torch.float64 else {k: v.to(arith) for k, v in sd0.items()}

    def mm(a, w):                                # a @ w^T
        return a.flip(-1) @ w.flip(-1).t() if kflip else a @ w.t()

    def rnd_for(gemm):                           # the rounding of the A operand of a block GEMM
        return mxq if gemm in mxg else rnd
    lin = rnd if mode == "fp16" else _ident      # Autocast<f16_t>: a Linear's accumulator + bias is fp16
    d, heads, n, npatch = ar.dim, ar.heads, ar.tokens, ar.num_patches
    vid = (video(cid) if frames is None else frames).to(arith)
    bsz, t = vid.shape[:2]
    bt = bsz * t
    with torch.no_grad():
        # im2col in the conv weight's (c, i, j) order, patches row-major over the grid
        patches = rnd(F.unfold(vid.reshape(bt, 3, ar.image, ar.image), ar.patch, stride=ar.patch).transpose(1, 2))
        pw = sd[P + "patch_embed.proj.weight"].reshape(d, ar.patch_k)
        pos = sd[P + "pos_embed"][0]
        ppos = pos[1:]
        if fault == "pos_late" and npatch > 1:
            ppos = torch.roll(ppos, -1, 0)       # patch p takes the row of patch p + 1
        x = lin(mm(patches, pw) + sd[P + "patch_embed.proj.bias"]) + ppos
        cls = (sd[P + "cls_token"].reshape(d) + pos[0]).expand(bt, 1, d)
        x = torch.cat([cls, x], dim=1)
        for i in range(ar.depth):
            b = f"{P}blocks.{i}."
            last = i == ar.depth - 1
            h = rnd_for("qkv")(F.layer_norm(x, (d,), sd[b + "norm1.weight"], sd[b + "norm1.bias"], ar.ln_eps))
            qkv = rnd(mm(h, sd[b + "attn.qkv.weight"]) + sd[b + "attn.qkv.bias"])
            q, k, v = qkv.reshape(bt, n, 3, heads, 64).permute(2, 0, 3, 1, 4).unbind(0)
            if fault == "drop_key" and n > 1:
                k, v = k[:, :, :-1], v[:, :, :-1]
            if fault == "pad_key":
                z = torch.zeros(bt, heads, 1, 64, dtype=arith)
                k, v = torch.cat([k, z], 2), torch.cat([v, z], 2)
            s = (q.flip(-1) @ k.flip(-1).transpose(-1, -2) if kflip else q @ k.transpose(-1, -2)) / 8.0
            e = torch.exp(s - s.max(-1, keepdim=True).values)
            if stats is not None:
                stats.append((float(s.std()), float((e / e.sum(-1, keepdim=True)).max(-1).values.median())))
            pr = rnd(e)
            den = (e if generic_attention(mode, n) else pr).sum(-1, keepdim=True)
            a = rnd_for("proj")((pr.flip(-1) @ v.flip(-2) if kflip else pr @ v) / den).transpose(1, 2).reshape(bt, n, d)
            upd = lin(mm(a, sd[b + "attn.proj.weight"]) + sd[b + "attn.proj.bias"])
            if fault == "row_tile" and i == 0 and not last:
                upd = upd.clone()
                upd[:, n - (n % 16 or 16):] = 0.0   # the residual rows keep what they held
            x = x + upd
            h = rnd_for("fc1")(F.layer_norm(x, (d,), sd[b + "norm2.weight"], sd[b + "norm2.bias"], ar.ln_eps))
            h = F.gelu(lin(mm(h, sd[b + "mlp.fc1.weight"]) + sd[b + "mlp.fc1.bias"]), approximate="tanh")
            # MXFP8 fc2: from the f32 value when fc1 is MXFP8 too (its epilogue), else from the bf16 activation
            h = mxq(h) if "fc1" in mxg and "fc2" in mxg else mxq(rnd(h)) if "fc2" in mxg else rnd(h)
            if fault == "fc2_ktile" and last:
                h = h.clone()
                h[..., -64:] = 0.0
            if fault == "fc2_scale" and last:
                h = h.clone()
                h[..., :32] *= 2.0
            x = x + lin(mm(h, sd[b + "mlp.fc2.weight"]) + sd[b + "mlp.fc2.bias"])
        feat = F.layer_norm(x[:, 0], (d,), sd[P + "norm.weight"], sd[P + "norm.bias"], ar.ln_eps).reshape(bsz, t, d)
        pooled = (feat[:, :-1] if fault == "frame_missing" else feat).sum(1) / t
        if mode == "fp16":
            pooled = rnd(pooled)
        emb = mm(pooled, sd["encoder.proj.weight"]) + sd["encoder.proj.bias"]
        if raw is not None:
            raw.append(emb.double())
        emb = lin(emb)
        pre = None
        if c.prefix:
            pre = O.mapper(sd, O.prefix_norm(emb, LN_SCALE, IN_WEIGHT), c.prefix[1], c.prefix[0])
    return emb.double(), (None if pre is None else pre.double())


def fault_defined(c: Case, fault: str) -> bool:
    """pos_late is nothing with one patch, row_tile nothing when block 0 is the CLS tail (depth 1)."""
    return not ((fault == "pos_late" and c.arch.num_patches == 1) or (fault == "row_tile" and c.depth == 1))


def oracle(cid: int, dtype=torch.float64):
    """oracle.vcap_oracle.encoder (+ prefix_norm + mapper) on tensors of `dtype` -> float64 outputs."""
    c = BY_ID[cid]
    sd = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dtype) for k, v in state_dict(cid).items()}
    with torch.no_grad():
        feat = O.vit_forward_features(sd, c.arch, video(cid).to(dtype).reshape(c.B * c.T, 3, c.image, c.image))
        emb = F.linear(O.cls_temporal_pool(feat, c.B, c.T), sd["encoder.proj.weight"], sd["encoder.proj.bias"])
        pre = O.mapper(sd, O.prefix_norm(emb, LN_SCALE, IN_WEIGHT), c.prefix[1], c.prefix[0]) if c.prefix else None
    return emb.double(), (None if pre is None else pre.double())


@lru_cache(maxsize=None)
def reference(cid: int):
    """The fp64 forward of the case, computed once and shared: (enc_out, prefix | None)."""
    return forward(cid, "fp64")


@lru_cache(maxsize=None)
def emulated(cid: int, mode: str):
    return forward(cid, mode)


@lru_cache(maxsize=None)
def emulated_fp8(cid: int, mx_gemms: Tuple[str, ...]):
    return forward(cid, "fp8", mx_gemms=mx_gemms)


def tolerance_fp8(cid: int, mx_gemms: Tuple[str, ...]) -> float:
    """3 x max |emulated - fp64| on enc_out of an fp8 run, as tolerance() below: from two CPU forwards alone."""
    return 3.0 * _maxdiff(emulated_fp8(cid, mx_gemms)[0], reference(cid)[0])


def expect_fused_fp8(c: Case, mx_gemms: Tuple[str, ...]) -> bool:
    """fp8: the fused QKV + attention kernel runs where bf16's does unless qkv or attn-proj is an MXFP8 GEMM."""
    return expect_fused(c, "bf16") and "qkv" not in mx_gemms and "proj" not in mx_gemms


def _maxdiff(a, b) -> float:
    return float((a - b).abs().max())


@lru_cache(maxsize=None)
def tolerance(cid: int, mode: str) -> Tuple[float, Optional[float]]:
    """(tol on enc_out, tol on prefix | None) of a 2-byte precision: 3 x max |emulated - fp64|, the operand
    roundings' own effect with a factor 3 for rounding flips where the kernels' f32 accumulation order (and
    their exp2 / sigmoid-form GELU) differ from fp64.  From the two CPU forwards alone."""
    (r, rp), (e, ep) = reference(cid), emulated(cid, mode)
    return 3.0 * _maxdiff(e, r), (None if rp is None else 3.0 * _maxdiff(ep, rp))


@lru_cache(maxsize=None)
def fp16_tie_margin(cid: int) -> Tuple[float, float]:
    """-> (margin, noise) of the fp16 run's enc_out.  The fp16 head rounds the embedding to fp16, so two correct
    runs that differ by f32 summation noise differ by a whole output ulp wherever that noise carries a value
    across a rounding tie: 2^-10 for |value| in [1, 2).  Where `max |gpu - emulated| <= tol / 3 + 1e-4` is below
    that ulp, such an output makes the check a coin toss on the summation order, not a check of the kernels:
    the emulated forward in f32 arithmetic then misses the bound against itself in f64 arithmetic (case 2 with
    its first seed: 9.77e-4 against 8.59e-4).  `noise` is max |f32-arithmetic - f64-arithmetic| of the emulated
    forward's unrounded embedding; `margin` is the smallest distance to a tie among the outputs whose ulp
    exceeds the bound (inf when there is none).  test_cpu_encoder_shapes.py asserts margin > 4 noise for every
    case; a case that misses it gets another seed, chosen there on the CPU alone (case 2)."""
    r64, r32 = [], []
    forward(cid, "fp16", raw=r64)
    forward(cid, "fp16", raw=r32, arith=torch.float32)
    y = r64[0]
    noise = _maxdiff(r32[0], y)
    bound = tolerance(cid, "fp16")[0] / 3 + 1e-4
    ulp = torch.pow(2.0, torch.floor(torch.log2(y.abs().clamp_min(2.0 ** -14))) - 10)
    t = y / ulp
    dist = ((t - torch.floor(t)) - 0.5).abs() * ulp
    risky = ulp > bound
    return (float(dist[risky].min()) if bool(risky.any()) else math.inf), noise


def outputs(pair):
    """(name, tensor) of the outputs a case has."""
    return [(nm, t) for nm, t in zip(("enc_out", "prefix"), pair) if t is not None]


def expect_fused(c: Case, prec: str) -> bool:
    """DESIGN.md "Encoder shapes": QKV + attention run as one kernel in bf16 / fp16 at 193..208 and
    257..272 tokens, nowhere else."""
    n = c.tokens
    return prec in ("bf16", "fp16") and (192 < n <= 208 or 256 < n <= 272)
