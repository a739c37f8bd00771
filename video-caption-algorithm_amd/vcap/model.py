"""Device-resident ViT encoder and GPT-2 decoder driven through the C ABI.

`HipViTEncoder` and `HipGPT2Decoder` own the packed weights in HBM (operand dtype bf16 for
throughput or fp32 for the parity mode; the ViT also fp16, the reference's autocast dtype, and MXFP8), build the include/vcap.h descriptors once, keep a
reusable workspace, and issue one ABI call per encode / per whole decode.

Weight packing from the reference's state-dict layout:
  * ViT Linear weights keep torch's [out, in] layout (K contiguous), the patch-embed conv
    weight is flattened to [D, 3*p*p] and zero-padded in K to the GEMM K step;
  * GPT-2 Conv1D weights ([in, out], x @ W + b) are transposed to [out, in];
  * wte is shared by the embedding lookup and the tied lm_head (text_decoder.py:28);
  * LayerNorm affines, biases, positional tables, encoder.proj and the mapper stay fp32.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _native as N
from .configs import VIDEO_DIM, GPT2Arch, ViTArch

_DTYPES = {"bf16": (N.DT_BF16, torch.bfloat16), "fp32": (N.DT_F32, torch.float32)}
# ViT only: "fp8" = MXFP8 block GEMMs (QKV / attn-proj / fc1 / fc2: e4m3 + E8M0 per 32 K elements,
# the gfx950 scaled-MFMA format; BASELINE configs[4]); patch-embed and QK^T / PV run in bf16.
# "fp16" = the reference's own ViT precision (torch.autocast(dtype=float16), video_encoder.py:261-264):
# fp16 operands at the bf16 MFMA rate, rounded where autocast rounds.  The decoder has no fp16 mode
# (the reference keeps GPT-2 in fp32).
_VIT_DTYPES = dict(_DTYPES, fp8=(N.DT_MXFP8, torch.bfloat16), fp16=(N.DT_F16, torch.float16))


def _dtype(mode: str):
    if mode not in _DTYPES:
        raise ValueError(f"precision must be one of {sorted(_DTYPES)}, got {mode!r}")
    return _DTYPES[mode]


def _stream(device) -> int:
    return torch.cuda.current_stream(device).cuda_stream


class _Workspace:
    def __init__(self, device):
        self.device = device
        self.buf: Optional[torch.Tensor] = None

    def get(self, nbytes: int) -> torch.Tensor:
        if self.buf is None or self.buf.numel() < nbytes:
            self.buf = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=self.device)
        return self.buf


class HipViTEncoder:
    """ViTFrameEncoder.forward (src/models/video_encoder.py:288-326) on the HIP path."""

    MX_GEMMS = ("qkv", "proj", "fc1", "fc2")

    def __init__(self, sd: Dict[str, np.ndarray], arch: ViTArch, precision: str = "bf16", device="cuda",
                 video_dim: int = VIDEO_DIM, mx_gemms: Sequence[str] = MX_GEMMS):
        """precision "fp8": the block GEMMs named in `mx_gemms` run in MXFP8, the others in bf16
        (their weights bf16, their scales NULL in the descriptor: csrc/runtime_vit.hip picks per GEMM)."""
        N.lib()
        self.arch, self.precision, self.device = arch, precision, torch.device(device)
        if precision not in _VIT_DTYPES:
            raise ValueError(f"precision must be one of {sorted(_VIT_DTYPES)}, got {precision!r}")
        bad = set(mx_gemms) - set(self.MX_GEMMS)
        if bad:
            raise ValueError(f"mx_gemms: unknown GEMM(s) {sorted(bad)}; choose from {self.MX_GEMMS}")
        self.dt, tdt = _VIT_DTYPES[precision]
        mx = self.dt == N.DT_MXFP8
        self.mx_gemms = tuple(g for g in self.MX_GEMMS if g in mx_gemms) if mx else ()
        self.video_dim = video_dim
        p = "encoder.backbone."
        dev = self.device

        def f32(k, shape=None):
            t = torch.from_numpy(np.ascontiguousarray(sd[k], dtype=np.float32))
            if shape is not None:
                t = t.reshape(shape)
            return t.to(dev).contiguous()

        def wt(k, shape=None):
            return f32(k, shape).to(tdt).contiguous()

        def wmx(k):
            """-> (e4m3 [N, K] uint8, E8M0 scales) through vcap_mx_quantize (kept alive in _keep)."""
            w = f32(k)
            n, kk = w.shape
            q = torch.empty(n, kk, dtype=torch.uint8, device=dev)
            sc = torch.empty(int(N.lib().vcap_mx_scale_bytes(n, kk)), dtype=torch.uint8, device=dev)
            N.check(N.lib().vcap_mx_quantize(N.DT_F32, w.data_ptr(), kk, n, kk, q.data_ptr(), sc.data_ptr(),
                                             _stream(dev)), "vcap_mx_quantize")
            return q, sc

        kstep = 128 // tdt.itemsize   # one 128-byte K-tile row of the patch-embed operand dtype
        K = arch.patch_k
        self.kpad = ((K + kstep - 1) // kstep) * kstep
        pw = torch.zeros(arch.dim, self.kpad, dtype=torch.float32)
        pw[:, :K] = torch.from_numpy(np.ascontiguousarray(sd[p + "patch_embed.proj.weight"])).reshape(arch.dim, K)
        self._keep: List[torch.Tensor] = []
        keep = self._keep.append
        self.patch_w = pw.to(dev).to(tdt).contiguous()
        keep(self.patch_w)
        t = {
            "patch_b": f32(p + "patch_embed.proj.bias"),
            "cls": f32(p + "cls_token", (arch.dim,)),
            "pos": f32(p + "pos_embed", (arch.tokens, arch.dim)),
            "norm_g": f32(p + "norm.weight"), "norm_b": f32(p + "norm.bias"),
            "proj_w": f32("encoder.proj.weight"), "proj_b": f32("encoder.proj.bias"),
        }
        for v in t.values():
            keep(v)
        self.proj_w, self.proj_b = t["proj_w"], t["proj_b"]   # encoder.proj, rewritable in place (train_align)
        self.layers = (N.VitLayer * arch.depth)()
        for i in range(arch.depth):
            b = f"{p}blocks.{i}."
            lt = dict(ln1_g=f32(b + "norm1.weight"), ln1_b=f32(b + "norm1.bias"),
                      qkv_b=f32(b + "attn.qkv.bias"), proj_b=f32(b + "attn.proj.bias"),
                      ln2_g=f32(b + "norm2.weight"), ln2_b=f32(b + "norm2.bias"),
                      fc1_b=f32(b + "mlp.fc1.bias"), fc2_b=f32(b + "mlp.fc2.bias"))
            for name, key in (("qkv", "attn.qkv.weight"), ("proj", "attn.proj.weight"), ("fc1", "mlp.fc1.weight"),
                              ("fc2", "mlp.fc2.weight")):
                if name in self.mx_gemms:
                    lt[name + "_w"], lt[name + "_ws"] = wmx(b + key)
                else:
                    lt[name + "_w"] = wt(b + key)
            for k, v in lt.items():
                keep(v)
                setattr(self.layers[i], k, v.data_ptr())
        self.desc = N.VitDesc(dtype=self.dt, dim=arch.dim, depth=arch.depth, heads=arch.heads, patch=arch.patch,
                              image=arch.image, mlp=arch.mlp, video_dim=video_dim, kpad=self.kpad,
                              ln_eps=arch.ln_eps, patch_w=self.patch_w.data_ptr(), patch_b=t["patch_b"].data_ptr(),
                              cls=t["cls"].data_ptr(), pos=t["pos"].data_ptr(), norm_g=t["norm_g"].data_ptr(),
                              norm_b=t["norm_b"].data_ptr(), proj_w=t["proj_w"].data_ptr(),
                              proj_b=t["proj_b"].data_ptr(), layers=self.layers)
        self.ws = _Workspace(dev)

    def workspace_bytes(self, B: int, T: int) -> int:
        return int(N.lib().vcap_vit_workspace_bytes(C.byref(self.desc), B, T))

    def fuses_qkv_attention(self, layer: int = 0) -> bool:
        """Whether vcap_vit_encode runs this block's QKV projection + attention as one kernel (the
        library's own predicate, vcap_vit_layer_fuses_qkv_attention)."""
        rc = int(N.lib().vcap_vit_layer_fuses_qkv_attention(C.byref(self.desc), int(layer)))
        N.check(min(rc, 0), "vcap_vit_layer_fuses_qkv_attention")
        return rc == 1

    def encode(self, video: torch.Tensor, prefix: Optional["HipPrefix"] = None,
               out_prefix: Optional[torch.Tensor] = None):
        """video [B,T,3,H,W] (or [B,3,H,W]) f32 on device -> (enc_out [B,256] f32, prefix [B,P,E] f32|None)."""
        if video.dim() == 4:
            video = video.unsqueeze(1)
        if video.dim() != 5:
            raise ValueError(f"expect [B,T,3,H,W], got {tuple(video.shape)}")
        B, T, Cc, H, W = video.shape
        a = self.arch
        if Cc != 3 or H != a.image or W != a.image:
            raise ValueError(f"expect frames of 3x{a.image}x{a.image}, got {tuple(video.shape)}")
        if video.device != self.device and not (video.is_cuda and self.device.type == "cuda"):
            raise ValueError("video must be on the encoder's device")
        video = video.to(torch.float32).contiguous()
        enc = torch.empty(B, self.video_dim, dtype=torch.float32, device=video.device)
        pre = None
        pd = None
        if prefix is not None:
            shape = (B, prefix.prefix_len, prefix.n_embd)
            if out_prefix is not None:
                if tuple(out_prefix.shape) != shape or out_prefix.dtype != torch.float32 or not out_prefix.is_contiguous():
                    raise ValueError(f"out_prefix must be contiguous f32 {shape}")
                pre = out_prefix
            else:
                pre = torch.empty(*shape, dtype=torch.float32, device=video.device)
            pd = C.byref(prefix.desc)
        nbytes = self.workspace_bytes(B, T)
        ws = self.ws.get(nbytes)
        N.check(N.lib().vcap_vit_encode(C.byref(self.desc), pd, video.data_ptr(), B, T, enc.data_ptr(),
                                        N.ptr(pre), ws.data_ptr(), ws.numel(), _stream(video.device)),
                "vcap_vit_encode")
        return enc, pre

    # ---- training: parameter gradients on the device (vcap_vit_encode_backward) -------------------------
    _BLOCK_FIELDS = (("norm1.weight", "ln1_g"), ("norm1.bias", "ln1_b"), ("attn.qkv.weight", "qkv_w"),
                     ("attn.qkv.bias", "qkv_b"), ("attn.proj.weight", "proj_w"), ("attn.proj.bias", "proj_b"),
                     ("norm2.weight", "ln2_g"), ("norm2.bias", "ln2_b"), ("mlp.fc1.weight", "fc1_w"),
                     ("mlp.fc1.bias", "fc1_b"), ("mlp.fc2.weight", "fc2_w"), ("mlp.fc2.bias", "fc2_b"))
    _LINEARS = ("qkv", "proj", "fc1", "fc2")
    GRAD_WORKSPACE_CAP = 12 << 30   # bytes of workspace one encode_backward chunk may take

    def _check_n_tail(self, n_tail: int) -> int:
        n_tail = int(n_tail)
        if not 1 <= n_tail <= self.arch.depth:
            raise ValueError(f"n_tail must be in 1..{self.arch.depth}, got {n_tail}")
        return n_tail

    def param_names(self, n_tail: int) -> List[str]:
        """The reference's state-dict names of the parameters encode_backward(n_tail=n_tail) returns gradients
        of: the last n_tail blocks, the final norm, encoder.proj and, with every block, the embedding."""
        n_tail = self._check_n_tail(n_tail)
        p = "encoder.backbone."
        names = []
        if n_tail == self.arch.depth:
            names += [p + "cls_token", p + "pos_embed", p + "patch_embed.proj.weight", p + "patch_embed.proj.bias"]
        for i in range(self.arch.depth - n_tail, self.arch.depth):
            names += [f"{p}blocks.{i}.{k}" for k, _ in self._BLOCK_FIELDS]
        return names + [p + "norm.weight", p + "norm.bias", "encoder.proj.weight", "encoder.proj.bias"]

    def _param_shape(self, name: str) -> Tuple[int, ...]:
        a, D = self.arch, self.arch.dim
        tail = name.split(".", 2)[-1] if name.startswith("encoder.backbone.") else name
        if ".blocks." in name:
            leaf = name.split(".", 4)[-1]
            out = {"attn.qkv": 3 * D, "attn.proj": D, "mlp.fc1": a.mlp, "mlp.fc2": D, "norm1": D, "norm2": D}[
                leaf.rsplit(".", 1)[0]]
            inn = a.mlp if leaf.startswith("mlp.fc2") else D
            return (out, inn) if leaf.endswith("weight") and "norm" not in leaf else (out,)
        return {"cls_token": (1, 1, D), "pos_embed": (1, a.tokens, D), "patch_embed.proj.weight": (D, 3, a.patch, a.patch),
                "patch_embed.proj.bias": (D,), "norm.weight": (D,), "norm.bias": (D,),
                "encoder.proj.weight": (self.video_dim, D), "encoder.proj.bias": (self.video_dim,)}[tail]

    def _device_params(self) -> Dict[str, torch.Tensor]:
        """name -> the device tensor the descriptor points at (the Linear weights in the operand dtype)."""
        byptr = {t.data_ptr(): t for t in self._keep}
        p = "encoder.backbone."
        out = {p + "patch_embed.proj.weight": self.patch_w, p + "patch_embed.proj.bias": byptr[self.desc.patch_b],
               p + "cls_token": byptr[self.desc.cls], p + "pos_embed": byptr[self.desc.pos],
               p + "norm.weight": byptr[self.desc.norm_g], p + "norm.bias": byptr[self.desc.norm_b],
               "encoder.proj.weight": self.proj_w, "encoder.proj.bias": self.proj_b}
        for i in range(self.arch.depth):
            for key, field in self._BLOCK_FIELDS:
                out[f"{p}blocks.{i}.{key}"] = byptr[getattr(self.layers[i], field)]
        return out

    def enable_grad(self, sd: Dict[str, np.ndarray], n_tail: int) -> int:
        """Upload what encode_backward needs for the last n_tail blocks beyond the inference operands: the f32
        masters of their four Linear weights and the operand-dtype transposed copies.  Only this call pays for
        them; returns the bytes it added."""
        if self.dt not in (N.DT_F32, N.DT_BF16):
            raise ValueError(f"ViT training serves precision fp32 and bf16, not {self.precision!r}")
        n_tail = self._check_n_tail(n_tail)
        tdt = _VIT_DTYPES[self.precision][1]
        a = self.arch
        self.grad_layers = (N.VitGradLayer * a.depth)()
        self._grad_keep: Dict[str, torch.Tensor] = {}
        added = 0
        for i in range(a.depth - n_tail, a.depth):
            for lin, key in zip(self._LINEARS, ("attn.qkv", "attn.proj", "mlp.fc1", "mlp.fc2")):
                name = f"encoder.backbone.blocks.{i}.{key}.weight"
                m = torch.from_numpy(np.ascontiguousarray(sd[name], dtype=np.float32)).to(self.device)
                t = m.t().contiguous().to(tdt)
                self._grad_keep[name + "/master"], self._grad_keep[name + "/t"] = m, t
                setattr(self.grad_layers[i], lin + "_t", t.data_ptr())
                setattr(self.grad_layers[i], lin + "_m", m.data_ptr())
                added += m.numel() * 4 + t.numel() * t.element_size()
        self.grad_desc = N.VitGradDesc(dtype=self.dt, dim=a.dim, mlp=a.mlp, depth=a.depth, layers=self.grad_layers)
        self.grad_n_tail = n_tail
        self.grad_ws = _Workspace(self.device)
        return added

    def backward_workspace_bytes(self, B: int, T: int, n_tail: int) -> int:
        return int(N.lib().vcap_vit_backward_workspace_bytes(C.byref(self.desc), B, T, n_tail))

    def _backward_chunk(self, video: torch.Tensor, grad_out: torch.Tensor, n_tail: int):
        B, T = video.shape[:2]
        a, dev = self.arch, video.device
        names = self.param_names(n_tail)
        g = {k: torch.empty(self._param_shape(k), dtype=torch.float32, device=dev) for k in names}
        p = "encoder.backbone."
        pw = None
        if n_tail == a.depth:   # the device's patch-embed gradient is [dim, kpad]
            pw = torch.empty(a.dim, self.kpad, dtype=torch.float32, device=dev)
        layers = (N.VitParamGradsLayer * n_tail)()
        for j, i in enumerate(range(a.depth - n_tail, a.depth)):
            for key, field in self._BLOCK_FIELDS:
                setattr(layers[j], field, g[f"{p}blocks.{i}.{key}"].data_ptr())
        pg = N.VitParamGrads(proj_w=g["encoder.proj.weight"].data_ptr(), proj_b=g["encoder.proj.bias"].data_ptr(),
                             norm_g=g[p + "norm.weight"].data_ptr(), norm_b=g[p + "norm.bias"].data_ptr(),
                             patch_w=N.ptr(pw), patch_b=N.ptr(g.get(p + "patch_embed.proj.bias")),
                             cls=N.ptr(g.get(p + "cls_token")), pos=N.ptr(g.get(p + "pos_embed")), layers=layers)
        enc = torch.empty(B, self.video_dim, dtype=torch.float32, device=dev)
        ws = self.grad_ws.get(self.backward_workspace_bytes(B, T, n_tail))
        N.check(N.lib().vcap_vit_encode_backward(C.byref(self.desc), C.byref(self.grad_desc), video.data_ptr(), B, T,
                                                 n_tail, grad_out.data_ptr(), enc.data_ptr(), C.byref(pg),
                                                 ws.data_ptr(), ws.numel(), _stream(dev)),
                "vcap_vit_encode_backward")
        if pw is not None:
            g[p + "patch_embed.proj.weight"] = pw[:, :a.patch_k].reshape(a.dim, 3, a.patch, a.patch).contiguous()
        return enc, g

    def grad_chunk_clips(self, B: int, T: int, n_tail: int) -> int:
        """The most clips (<= B) whose backward workspace fits GRAD_WORKSPACE_CAP (at least one)."""
        c = B
        while c > 1 and self.backward_workspace_bytes(c, T, n_tail) > self.GRAD_WORKSPACE_CAP:
            c -= 1
        return c

    def encode_backward(self, video: torch.Tensor, grad_out: torch.Tensor, n_tail: Optional[int] = None,
                        chunk: Optional[int] = None):
        """video [B,T,3,H,W] f32, grad_out [B, video_dim] = d loss / d enc_out -> (enc_out with encode's bits,
        {reference parameter name: f32 gradient}).  Clips go to the device `chunk` at a time (default: what fits
        GRAD_WORKSPACE_CAP); the chunks' gradients are added in chunk order."""
        if not hasattr(self, "grad_desc"):
            raise RuntimeError("call enable_grad(sd, n_tail) before encode_backward")
        n_tail = self._check_n_tail(self.grad_n_tail if n_tail is None else n_tail)
        if n_tail > self.grad_n_tail:
            raise ValueError(f"enable_grad prepared {self.grad_n_tail} block(s), n_tail = {n_tail}")
        if video.dim() == 4:
            video = video.unsqueeze(1)
        a = self.arch
        if video.dim() != 5 or tuple(video.shape[2:]) != (3, a.image, a.image):
            raise ValueError(f"expect [B,T,3,{a.image},{a.image}], got {tuple(video.shape)}")
        B, T = video.shape[:2]
        if tuple(grad_out.shape) != (B, self.video_dim):
            raise ValueError(f"grad_out must be [{B}, {self.video_dim}], got {tuple(grad_out.shape)}")
        video = video.to(torch.float32).contiguous()
        grad_out = grad_out.to(device=video.device, dtype=torch.float32).contiguous()
        chunk = self.grad_chunk_clips(B, T, n_tail) if chunk is None else max(1, int(chunk))
        encs, total = [], None
        for b0 in range(0, B, chunk):
            enc, g = self._backward_chunk(video[b0:b0 + chunk], grad_out[b0:b0 + chunk], n_tail)
            encs.append(enc)
            if total is None:
                total = g
            else:
                for k in total:
                    total[k] += g[k]
        return (encs[0] if len(encs) == 1 else torch.cat(encs)), total

    def load_state_dict(self, state: Dict[str, torch.Tensor]) -> None:
        """Refresh the device operands from f32 tensors (reference names) IN PLACE: the same device pointers,
        the operand-dtype weights and, where enable_grad made them, the masters and transposed copies repacked."""
        params = self._device_params()
        a = self.arch
        for name, src in state.items():
            if name not in params:
                raise KeyError(f"not an encoder parameter: {name}")
            src = torch.as_tensor(src).detach().to(device=self.device, dtype=torch.float32)
            dst = params[name]
            if name.endswith("patch_embed.proj.weight"):
                dst[:, :a.patch_k].copy_(src.reshape(a.dim, a.patch_k))
            else:
                dst.copy_(src.reshape(dst.shape))
            keep = getattr(self, "_grad_keep", {})
            if name + "/master" in keep:
                keep[name + "/master"].copy_(src)
                keep[name + "/t"].copy_(src.t())


class HipPrefix:
    """Engine prefix normalisation (core/engine.py:44-50) + mapper (text_decoder.py:249)."""

    def __init__(self, sd: Dict[str, np.ndarray], n_embd: int, prefix_len: int = 4, ln_scale: float = 0.6,
                 in_weight: float = 0.4, device="cuda"):
        dev = torch.device(device)
        self.prefix_len, self.n_embd = prefix_len, n_embd
        self.mapper_w = torch.from_numpy(np.ascontiguousarray(sd["decoder.mapper.0.weight"], np.float32)).to(dev)
        self.mapper_b = torch.from_numpy(np.ascontiguousarray(sd["decoder.mapper.0.bias"], np.float32)).to(dev)
        if self.mapper_w.shape[0] != prefix_len * n_embd:
            raise ValueError(f"mapper out {self.mapper_w.shape[0]} != prefix_len*n_embd {prefix_len * n_embd}")
        self.set_scales(ln_scale, in_weight)

    def set_scales(self, ln_scale: Optional[float], in_weight: Optional[float]) -> None:
        self.ln_scale = float(ln_scale) if ln_scale is not None else 0.0
        self.in_weight = float(in_weight) if in_weight is not None else 0.0
        self.desc = N.PrefixDesc(ln_scale=self.ln_scale, in_weight=self.in_weight, prefix_len=self.prefix_len,
                                 n_embd=self.n_embd, mapper_w=self.mapper_w.data_ptr(),
                                 mapper_b=self.mapper_b.data_ptr())

    def project(self, emb: torch.Tensor) -> torch.Tensor:
        """emb [B,256] or [B,1,256] f32 -> prefix embeds [B, P, E] (vcap_prefix_project)."""
        B = emb.shape[0]
        e = emb.reshape(B, -1).to(torch.float32).contiguous()
        out = torch.empty(B, self.prefix_len, self.n_embd, dtype=torch.float32, device=e.device)
        N.check(N.lib().vcap_prefix_project(e.data_ptr(), B, e.shape[1], C.byref(self.desc), out.data_ptr(),
                                            _stream(e.device)), "vcap_prefix_project")
        return out


@dataclass
class GenConfig:
    max_new_tokens: int = 24
    min_new_tokens: int = 8
    no_repeat_ngram_size: int = 3
    repetition_penalty: float = 1.1
    eos_token_id: int = 50256
    pad_token_id: int = 50256
    use_graph: bool = True
    max_blocks: int = 0      # >0: narrower decode grids (decode sharing the GPU with an encode)
    num_beams: int = 1       # >1: device beam search (vcap_gpt2_beam_search, presets precise / detailed)
    length_penalty: float = 1.0
    # sampling (presets natural / safe_sample): HF's do_sample = (num_beams == 1 and temperature != 1),
    # text_decoder.py:137; top_k 50 is the generation-config default the reference inherits
    temperature: float = 1.0
    top_k: int = 50
    top_p: float = 1.0
    seed: int = 0

    @property
    def do_sample(self) -> bool:
        return self.num_beams == 1 and self.temperature != 1.0

    @classmethod
    def raw_greedy(cls, max_new_tokens: int = 24, eos: int = 50256, use_graph: bool = True) -> "GenConfig":
        """benchmark_baseline.run_decoder_steps semantics: argmax, no processors, no min length."""
        return cls(max_new_tokens, 0, 0, 1.0, eos, eos, use_graph)


@dataclass
class ScoreResult:
    """HipGPT2Decoder.score's outputs (device tensors; None where not requested)."""
    logits: Optional[torch.Tensor]     # [B, S, V] f32
    logprobs: Optional[torch.Tensor]   # [B, S] f32: log p(targets[b, i] | inputs up to i), 0 where ignored
    nll_sum: Optional[torch.Tensor]    # 0-dim f32: sum of -logprob over the counted positions
    count: Optional[torch.Tensor]      # 0-dim f32: how many positions were counted

    @property
    def loss(self) -> Optional[torch.Tensor]:
        """Mean cross-entropy (NaN with no counted position, as F.cross_entropy gives)."""
        return None if self.nll_sum is None else self.nll_sum / self.count


def split_prompts(prompt_ids, B: int, merge_equal: bool = True) -> Tuple[List[int], Optional[List[List[int]]]]:
    """What a decode call's `prompt_ids` means: (ids, None) for one prompt shared by the B rows - a flat
    sequence of ids, or B equal sequences - else (all ids concatenated, the B per-row id lists): ragged.
    merge_equal=False keeps B equal sequences ragged (HipGPT2Decoder.force_ragged)."""
    items = list(prompt_ids)
    if not any(isinstance(x, (list, tuple, np.ndarray, torch.Tensor)) for x in items):
        return [int(i) for i in items], None
    rows = []
    for x in items:
        if not isinstance(x, (list, tuple, np.ndarray, torch.Tensor)):
            raise ValueError("prompt_ids mixes ids and sequences: give one flat prompt or one sequence per row")
        rows.append([int(i) for i in (x.tolist() if hasattr(x, "tolist") else x)])
    if len(rows) != B:
        raise ValueError(f"prompt_ids has {len(rows)} prompts for {B} rows")
    if merge_equal and all(r == rows[0] for r in rows):
        return rows[0], None
    return [i for r in rows for i in r], rows


def _prompts_arg(rows: List[List[int]]):
    """vcap_prompts of per-row id lists + the ctypes arrays it points into (keep them for the call)."""
    flat = [i for r in rows for i in r]
    offs = [0]
    for r in rows:
        offs.append(offs[-1] + len(r))
    ids_arr = (C.c_int * max(len(flat), 1))(*flat)
    off_arr = (C.c_int * len(offs))(*offs)
    return N.Prompts(ids=ids_arr, offsets=off_arr), ids_arr, off_arr


class HipGPT2Decoder:
    """GPT2LMHeadModel greedy generate from inputs_embeds (text_decoder.py:131-144) on the HIP path."""

    # |bf16-screen score - exact f32 score| <= SCREEN_C * ||h||_2 * ||w_v||_2.  bf16 round-to-nearest
    # has unit roundoff u = 2^-8 PER OPERAND, so rounding h and w gives |h~w~ - hw| <= (2u + u^2) |h||w|
    # per element (7.83e-3 summed, Cauchy-Schwarz); the two f32 dot products (the screen's MFMA sum and
    # the rescoring's fma chain, n_embd <= 1024 terms) add 2 x 1024 x 2^-24 each, doubled for an
    # accumulator that truncates (2.44e-4): 8.07e-3, and 1.6 % over it.  The runtime multiplies the
    # bound by max(rep, 1/rep) when a repetition penalty is active (a penalised negative score is
    # scaled by rep, its error with it: csrc/runtime_gpt2.hip issue_decode).  Round 5 shipped c = 0.0043,
    # which counted 2^-8 for BOTH roundings; tests/test_gpu_lm_screen.py builds a near-tie that the
    # old constant gets wrong and this one does not.
    SCREEN_C = 0.0082
    # True: per-row prompts go through the _ragged entry points even when they are all equal (or B = 1);
    # by default equal prompts take the one-prompt call.  For tests and A/B measurements.
    force_ragged = False

    def __init__(self, sd: Dict[str, np.ndarray], arch: GPT2Arch, precision: str = "bf16", device="cuda",
                 prefix_len: int = 4, screen: bool = True):
        """precision "fp32" with `screen`: a greedy step without requested logits runs the lm_head
        in bf16 as a screen and rescores the tokens it cannot rule out in f32 (csrc/decode.hip,
        vcap_decode_finalize_kernel<float, true>): the same exact-f32 argmax for half the bytes."""
        N.lib()
        self.arch, self.precision, self.device = arch, precision, torch.device(device)
        self.dt, tdt = _dtype(precision)
        self.prefix_len = prefix_len
        dev = self.device
        p = "decoder.model.transformer."
        self._keep: List[torch.Tensor] = []
        # state-dict name -> its device copy: the f32 tensor of a bias / LayerNorm affine, the rows-packed
        # buffer of a Conv1D weight.  load_tail() rewrites these in place.
        self._named: Dict[str, torch.Tensor] = {}

        def f32(k):
            t = torch.from_numpy(np.ascontiguousarray(sd[k], dtype=np.float32)).to(dev).contiguous()
            self._keep.append(t)
            self._named[k] = t
            return t

        def conv_t(k):  # Conv1D [in, out] -> [out, in] -> rows-packed (vcap_rows_pack)
            t = torch.from_numpy(np.ascontiguousarray(sd[k], dtype=np.float32)).t().contiguous()
            self._named[k] = self._pack(t.to(dev).to(tdt).contiguous())
            return self._named[k]

        self.wte = torch.from_numpy(np.ascontiguousarray(sd[p + "wte.weight"], np.float32)).to(dev).to(tdt)
        self.wte = self.wte.contiguous()
        self._keep.append(self.wte)
        self.lm_head = self._pack(self.wte)   # tied lm_head, packed copy
        screen_w, screen_bound = None, 0.0
        if self.dt == N.DT_F32 and screen:
            screen_w = self._pack(self.wte.to(torch.bfloat16).contiguous(), N.DT_BF16)
            wmax = float(torch.linalg.vector_norm(self.wte.double(), dim=1).max())
            screen_bound = self.SCREEN_C * wmax * (1.0 + 1e-6)
        self.screen = screen_w is not None
        self.wpe = f32(p + "wpe.weight")
        lnf_g, lnf_b = f32(p + "ln_f.weight"), f32(p + "ln_f.bias")
        self.layers = (N.GPT2Layer * arch.n_layer)()
        for i in range(arch.n_layer):
            b = f"{p}h.{i}."
            ly = self.layers[i]
            ly.ln1_g, ly.ln1_b = f32(b + "ln_1.weight").data_ptr(), f32(b + "ln_1.bias").data_ptr()
            ly.attn_w, ly.attn_b = conv_t(b + "attn.c_attn.weight").data_ptr(), f32(b + "attn.c_attn.bias").data_ptr()
            ly.aproj_w = conv_t(b + "attn.c_proj.weight").data_ptr()
            ly.aproj_b = f32(b + "attn.c_proj.bias").data_ptr()
            ly.ln2_g, ly.ln2_b = f32(b + "ln_2.weight").data_ptr(), f32(b + "ln_2.bias").data_ptr()
            ly.fc_w, ly.fc_b = conv_t(b + "mlp.c_fc.weight").data_ptr(), f32(b + "mlp.c_fc.bias").data_ptr()
            ly.mproj_w = conv_t(b + "mlp.c_proj.weight").data_ptr()
            ly.mproj_b = f32(b + "mlp.c_proj.bias").data_ptr()
        self.desc = N.GPT2Desc(dtype=self.dt, n_embd=arch.n_embd, n_layer=arch.n_layer, n_head=arch.n_head,
                               vocab=arch.vocab, n_positions=arch.n_positions, prefix_len=prefix_len,
                               ln_eps=arch.ln_eps, wte=self.wte.data_ptr(), lm_head=self.lm_head.data_ptr(),
                               wpe=self.wpe.data_ptr(),
                               lnf_g=lnf_g.data_ptr(), lnf_b=lnf_b.data_ptr(), layers=self.layers,
                               lm_head_screen=screen_w.data_ptr() if screen_w is not None else None,
                               screen_bound=screen_bound)
        self.ws = _Workspace(dev)
        self._stable = {}             # (B, max_new) -> persistent prefix / ids buffers (graph reuse)
        torch.cuda.synchronize(dev)   # packing ran on the current stream; decodes may use others

    def _pack(self, w: torch.Tensor, dt: Optional[int] = None) -> torch.Tensor:
        """[N, K] device weight -> rows-packed copy (MFMA-fragment order, csrc/decode.hip)."""
        dt = self.dt if dt is None else dt
        rows, k = w.shape
        nbytes = int(N.lib().vcap_rows_packed_bytes(dt, rows, k))
        if nbytes == 0:
            raise ValueError(f"cannot pack a [{rows}, {k}] weight (K must be a multiple of 32 bf16 / 16 f32)")
        packed = torch.empty(nbytes, dtype=torch.uint8, device=w.device)
        self._pack_into(w, packed, dt)
        self._keep.append(packed)
        return packed

    def _pack_into(self, w: torch.Tensor, packed: torch.Tensor, dt: Optional[int] = None) -> None:
        dt = self.dt if dt is None else dt
        rows, k = w.shape
        if packed.numel() != int(N.lib().vcap_rows_packed_bytes(dt, rows, k)):
            raise ValueError(f"packed buffer of {packed.numel()} bytes does not hold a [{rows}, {k}] weight")
        N.check(N.lib().vcap_rows_pack(dt, w.data_ptr(), w.stride(0), rows, k, packed.data_ptr(),
                                       _stream(w.device)), "vcap_rows_pack")

    def workspace_bytes(self, B: int, prompt_len: int, max_new: int) -> int:
        return int(N.lib().vcap_gpt2_workspace_bytes(C.byref(self.desc), B, self.prefix_len + prompt_len, max_new))

    def ragged_workspace_bytes(self, rows: List[List[int]], max_new: int, num_beams: int = 1) -> int:
        """Workspace of a ragged call (0: the device refuses the shape - see include/vcap.h)."""
        _, _, off = _prompts_arg(rows)
        if num_beams > 1:
            return int(N.lib().vcap_gpt2_beam_search_ragged_workspace_bytes(C.byref(self.desc), off, len(rows),
                                                                            int(num_beams), int(max_new)))
        return int(N.lib().vcap_gpt2_ragged_workspace_bytes(C.byref(self.desc), off, len(rows), int(max_new)))

    def generate_ids(self, prefix: torch.Tensor, prompt_ids: Sequence, cfg: GenConfig,
                     out: Optional[torch.Tensor] = None, logits_out: Optional[torch.Tensor] = None,
                     workspace: Optional["_Workspace"] = None, lengths_out: Optional[torch.Tensor] = None,
                     warped_out: Optional[torch.Tensor] = None, force_ids: Optional[torch.Tensor] = None
                     ) -> torch.Tensor:
        """prefix [B,P,E] f32 device, prompt ids (BOS-only prompt = [eos]) -> int32 [B, max_new] EOS-padded.

        `prompt_ids` is one flat sequence of ids for the whole batch, or B sequences, one per row (ragged
        prompts: row b gives what a B = 1 call with prefix row b and prompt b gives).  B equal sequences
        take the one-prompt path.

        `workspace` (KV pages + decode scratch) defaults to the decoder's own; concurrent decodes on
        different streams pass one each (the captured graph is keyed on it).  cfg.num_beams > 1 runs
        the device beam search instead of greedy; `lengths_out` (int32 [B]) then receives each best
        hypothesis' length (HF returns the first max(lengths) columns)."""
        if cfg.num_beams > 1:
            return self._beam_ids(prefix, prompt_ids, cfg, out, workspace, lengths_out)
        B, P, E = prefix.shape
        if P != self.prefix_len or E != self.arch.n_embd:
            raise ValueError(f"prefix shape {tuple(prefix.shape)} != [B,{self.prefix_len},{self.arch.n_embd}]")
        prefix = prefix.to(torch.float32).contiguous()
        ids, rows = split_prompts(prompt_ids, B, not self.force_ragged)
        mx = int(cfg.max_new_tokens)
        fresh = (out is None and logits_out is None and workspace is None and warped_out is None and force_ids is None
                 and cfg.use_graph)
        if fresh:
            # A replayed graph bakes in the prefix / ids addresses: a caller that hands over new
            # tensors every call (the engine path) decodes through persistent per-shape buffers,
            # so one captured graph serves every call of that shape; the caller gets a copy.
            key = (B, mx)
            if key not in self._stable:
                self._stable[key] = (torch.empty(B, P, E, dtype=torch.float32, device=self.device),
                                     torch.empty(B, mx, dtype=torch.int32, device=self.device))
            sp, so = self._stable[key]
            sp.copy_(prefix)
            self.generate_ids(sp, ids if rows is None else rows, cfg, out=so)
            return so.clone()
        if out is None:
            out = torch.empty(B, mx, dtype=torch.int32, device=prefix.device)
        if logits_out is not None and tuple(logits_out.shape) != (mx, B, self.arch.vocab):
            raise ValueError("logits_out must be [max_new, B, vocab] f32")
        if (warped_out is not None or force_ids is not None) and not cfg.do_sample:
            raise ValueError("warped_out / force_ids belong to the sampling mode (temperature != 1)")
        gp = N.GenParams(max_new_tokens=mx, min_new_tokens=int(cfg.min_new_tokens),
                         no_repeat_ngram_size=int(cfg.no_repeat_ngram_size),
                         repetition_penalty=float(cfg.repetition_penalty), eos_token_id=int(cfg.eos_token_id),
                         pad_token_id=int(cfg.pad_token_id), use_graph=int(bool(cfg.use_graph)),
                         max_blocks=int(cfg.max_blocks))
        arr = (C.c_int * max(len(ids), 1))(*ids)
        if rows is not None:
            nbytes = self.ragged_workspace_bytes(rows, mx)
            if nbytes == 0:
                raise N.VcapError("vcap_gpt2_ragged_workspace_bytes: unsupported shape (prompts over 64 ids, more "
                                  "rows than vcap_gpt2_max_rows(), or a context past n_positions)", N.E_UNSUPPORTED)
            ws = (workspace or self.ws).get(nbytes)
            pr, _ids_keep, _off_keep = _prompts_arg(rows)
        else:
            ws = (workspace or self.ws).get(self.workspace_bytes(B, len(ids), mx))
        if cfg.do_sample:
            if warped_out is not None and (tuple(warped_out.shape) != (mx, B, self.arch.vocab)
                                           or warped_out.dtype != torch.float32 or not warped_out.is_contiguous()):
                raise ValueError("warped_out must be contiguous f32 [max_new, B, vocab]")
            if force_ids is not None:
                if tuple(force_ids.shape) != (B, mx):
                    raise ValueError("force_ids must be [B, max_new]")
                force_ids = force_ids.to(device=prefix.device, dtype=torch.int32).contiguous()
            sp = N.SampleParams(temperature=float(cfg.temperature), top_k=int(cfg.top_k), top_p=float(cfg.top_p),
                                seed=int(cfg.seed) & 0xFFFFFFFFFFFFFFFF)
            if rows is not None:
                N.check(N.lib().vcap_gpt2_sample_ragged(C.byref(self.desc), C.byref(gp), C.byref(sp),
                                                        prefix.data_ptr(), C.byref(pr), B, out.data_ptr(),
                                                        N.ptr(logits_out), N.ptr(warped_out), N.ptr(force_ids),
                                                        ws.data_ptr(), ws.numel(), _stream(prefix.device)),
                        "vcap_gpt2_sample_ragged")
                return out
            N.check(N.lib().vcap_gpt2_sample(C.byref(self.desc), C.byref(gp), C.byref(sp), prefix.data_ptr(), arr,
                                             len(ids), B, out.data_ptr(), N.ptr(logits_out), N.ptr(warped_out),
                                             N.ptr(force_ids), ws.data_ptr(), ws.numel(), _stream(prefix.device)),
                    "vcap_gpt2_sample")
            return out
        if rows is not None:
            N.check(N.lib().vcap_gpt2_generate_ragged(C.byref(self.desc), C.byref(gp), prefix.data_ptr(), C.byref(pr),
                                                      B, out.data_ptr(), N.ptr(logits_out), ws.data_ptr(), ws.numel(),
                                                      _stream(prefix.device)), "vcap_gpt2_generate_ragged")
            return out
        N.check(N.lib().vcap_gpt2_generate(C.byref(self.desc), C.byref(gp), prefix.data_ptr(), arr, len(ids), B,
                                           out.data_ptr(), N.ptr(logits_out), ws.data_ptr(), ws.numel(),
                                           _stream(prefix.device)), "vcap_gpt2_generate")
        return out


    @torch.no_grad()
    def score(self, embeds: torch.Tensor, key_mask: Optional[torch.Tensor] = None,
              targets: Optional[torch.Tensor] = None, want_logits: bool = False,
              check_mask: bool = True) -> "ScoreResult":
        """Teacher-forced forward over embeds [B, S, E] (inputs_embeds: prefix + token embeddings), one
        vcap_gpt2_score call per chunk of sequences with B_chunk * S <= vcap_gpt2_max_rows().

        key_mask [B, S] (nonzero = visible): query i attends to the visible keys j <= i; positions stay
        0..S-1.  Column 0 must be visible: checked here (one small device read) unless the caller built
        the mask with ones in front itself and passes check_mask=False.  targets [B, S]: the token to
        predict at each position (already shifted), -100 = ignored.  Returns logits [B, S, V] when
        want_logits, logprobs [B, S] (0 where ignored) and the (nll_sum, count) pair when targets are
        given - the chunks' pairs added in chunk order - all on the device."""
        x = embeds.to(self.device, torch.float32).contiguous()
        if x.dim() != 3 or x.shape[2] != self.arch.n_embd:
            raise ValueError(f"embeds shape {tuple(x.shape)} != [B, S, {self.arch.n_embd}]")
        B, S, _ = x.shape
        V = self.arch.vocab
        max_rows = int(N.lib().vcap_gpt2_max_rows())
        if B < 1 or S < 1 or S > max_rows or S > self.arch.n_positions:
            raise N.VcapError(f"score: S = {S} exceeds vcap_gpt2_max_rows() = {max_rows} or n_positions",
                              N.E_UNSUPPORTED)
        if targets is None and not want_logits:
            raise ValueError("score: give targets, want_logits, or both")
        km = tg = logits = logprobs = None
        if key_mask is not None:
            km = (key_mask != 0).to(self.device, torch.uint8).contiguous()
            if tuple(km.shape) != (B, S):
                raise ValueError(f"key_mask shape {tuple(km.shape)} != {(B, S)}")
            if check_mask and not bool(km[:, 0].all()):
                raise N.VcapError("score: key_mask[:, 0] must be nonzero (a row with no visible key)", N.E_ARG)
        if targets is not None:
            tg = targets.to(self.device, torch.int32).contiguous()
            if tuple(tg.shape) != (B, S):
                raise ValueError(f"targets shape {tuple(tg.shape)} != {(B, S)}")
            logprobs = torch.empty(B, S, dtype=torch.float32, device=self.device)
        if want_logits:
            logits = torch.empty(B, S, V, dtype=torch.float32, device=self.device)
        per = max(1, max_rows // S)
        starts = list(range(0, B, per))
        pairs = torch.empty(len(starts), 2, dtype=torch.float32, device=self.device) if tg is not None else None
        stream = _stream(self.device)
        for ci, b0 in enumerate(starts):
            nb = min(per, B - b0)
            ws = self.ws.get(int(N.lib().vcap_gpt2_score_workspace_bytes(C.byref(self.desc), nb, S)))
            N.check(N.lib().vcap_gpt2_score(C.byref(self.desc), x[b0:].data_ptr(), nb, S,
                                            N.ptr(None if km is None else km[b0:]),
                                            N.ptr(None if tg is None else tg[b0:]),
                                            N.ptr(None if logits is None else logits[b0:]),
                                            N.ptr(None if logprobs is None else logprobs[b0:]),
                                            N.ptr(None if pairs is None else pairs[ci]),
                                            ws.data_ptr(), ws.numel(), stream), "vcap_gpt2_score")
        nll_sum = count = None
        if pairs is not None:
            nll_sum, count = pairs[0, 0], pairs[0, 1]
            for ci in range(1, len(starts)):   # chunk order: the same sum on every run
                nll_sum, count = nll_sum + pairs[ci, 0], count + pairs[ci, 1]
        return ScoreResult(logits, logprobs, nll_sum, count)

    def enable_grad(self, sd: Dict[str, np.ndarray]) -> int:
        """Upload the weight copies vcap_gpt2_score_backward reads and build its grad desc (once; later
        calls return at once).  `sd` is the state dict the decoder was built from.  Inference memory is
        unchanged until this is called.  Returns the bytes added: per layer the four Conv1D [in, out]
        matrices as stored (12 E^2 elements) and the Linear-layout copies of c_attn and c_fc (7 E^2), plus wte
        transposed and padded ([E, ceil(V / 128) * 128]) - GPT-2-small: 0.35 GB in bf16 (0.25 GB of it the
        Conv1D copies and wte^T), 0.70 GB in fp32."""
        if getattr(self, "grad_desc", None) is not None:
            return self.grad_bytes
        dev, tdt = self.device, _dtype(self.precision)[1]
        p = "decoder.model.transformer."
        keep: List[torch.Tensor] = []
        # state-dict name of a Conv1D weight -> its [in, out] copy (and, for c_attn / c_fc, the Linear-layout
        # one): what load_tail() rewrites
        named: Dict[str, List[torch.Tensor]] = {}

        def up(a: torch.Tensor, name: Optional[str] = None) -> int:
            t = a.to(dev).to(tdt).contiguous()
            keep.append(t)
            if name is not None:
                named.setdefault(name, []).append(t)
            return t.data_ptr()

        def mat(k):
            return torch.from_numpy(np.ascontiguousarray(sd[k], dtype=np.float32))

        V, E = self.arch.vocab, self.arch.n_embd
        vpad = (V + 127) // 128 * 128
        wte_t = torch.zeros(E, vpad, dtype=torch.float32)
        wte_t[:, :V] = mat(p + "wte.weight").t()
        layers = (N.GPT2GradLayer * self.arch.n_layer)()
        for i in range(self.arch.n_layer):
            b = f"{p}h.{i}."
            ly = layers[i]
            na, nf = b + "attn.c_attn.weight", b + "mlp.c_fc.weight"
            attn, fc = mat(na), mat(nf)
            ly.attn_c = up(attn, na)
            ly.aproj_c = up(mat(b + "attn.c_proj.weight"), b + "attn.c_proj.weight")
            ly.fc_c = up(fc, nf)
            ly.mproj_c = up(mat(b + "mlp.c_proj.weight"), b + "mlp.c_proj.weight")
            ly.attn_l, ly.fc_l = up(attn.t(), na), up(fc.t(), nf)
        self._grad_layers = layers
        self._grad_named = named
        self.grad_desc = N.GPT2GradDesc(dtype=self.dt, n_embd=E, n_layer=self.arch.n_layer, vocab_pad=vpad,
                                        wte_t=up(wte_t), layers=layers)
        self._grad_keep = keep
        self.grad_bytes = sum(t.numel() * t.element_size() for t in keep)
        torch.cuda.synchronize(dev)
        return self.grad_bytes

    @torch.no_grad()
    def score_backward(self, embeds: torch.Tensor, key_mask: Optional[torch.Tensor] = None,
                       targets: Optional[torch.Tensor] = None, grad_logprob: Optional[torch.Tensor] = None,
                       check_mask: bool = True) -> Tuple["ScoreResult", torch.Tensor]:
        """score() with targets, plus grad_embeds [B, S, E] = sum over the counted positions of
        grad_logprob[b, i] * d logprobs[b, i] / d embeds (grad_logprob None: -1 everywhere, the gradient of
        nll_sum) - one vcap_gpt2_score_backward call per chunk of sequences, chunked exactly as score()
        chunks.  A sequence's gradient bits do not depend on the other sequences of its call, so the chunked
        result equals the one-call bits.  Needs enable_grad(sd) first.  Returns (ScoreResult without
        logits, grad_embeds); logprobs and the loss pair are score()'s bits."""
        res, grad, _ = self._score_backward("score_backward", embeds, key_mask, targets, grad_logprob, check_mask, 0)
        return res, grad

    TAIL_PARAMS = ("ln_1.weight", "ln_1.bias", "attn.c_attn.weight", "attn.c_attn.bias", "attn.c_proj.weight",
                   "attn.c_proj.bias", "ln_2.weight", "ln_2.bias", "mlp.c_fc.weight", "mlp.c_fc.bias",
                   "mlp.c_proj.weight", "mlp.c_proj.bias")   # vcap_gpt2_param_grads_layer's field order

    def tail_names(self, n_tail: int) -> List[str]:
        """State-dict names of every parameter of the last n_tail blocks, layer by layer in TAIL_PARAMS order."""
        L = self.arch.n_layer
        if not 1 <= int(n_tail) <= L:
            raise N.VcapError(f"n_tail = {n_tail} outside 1 .. n_layer = {L}", N.E_ARG)
        return [f"decoder.model.transformer.h.{i}.{k}" for i in range(L - int(n_tail), L) for k in self.TAIL_PARAMS]

    def _tail_shape(self, name: str) -> Tuple[int, ...]:
        E = self.arch.n_embd
        mod, kind = name.split(".", 5)[5].rsplit(".", 1)   # "attn.c_attn", "weight"
        fan_in, fan_out = {"attn.c_attn": (E, 3 * E), "attn.c_proj": (E, E), "mlp.c_fc": (E, 4 * E),
                           "mlp.c_proj": (4 * E, E)}.get(mod, (E, E))
        return (fan_in, fan_out) if kind == "weight" and not mod.startswith("ln_") else (fan_out,)

    @torch.no_grad()
    def score_backward_tail(self, embeds: torch.Tensor, key_mask: Optional[torch.Tensor] = None,
                            targets: Optional[torch.Tensor] = None, grad_logprob: Optional[torch.Tensor] = None,
                            n_tail: int = 1, check_mask: bool = True
                            ) -> Tuple["ScoreResult", torch.Tensor, Dict[str, torch.Tensor]]:
        """score_backward plus the gradient of the same objective with respect to every parameter of the last
        n_tail blocks (vcap_gpt2_score_backward_tail): {state-dict name: f32 device tensor in HF's layout}.
        The ScoreResult and grad_embeds are score_backward's bits.  Chunked as score_backward chunks; the
        chunks' parameter gradients are added in chunk order."""
        names = self.tail_names(n_tail)
        res, grad, pg = self._score_backward("score_backward_tail", embeds, key_mask, targets, grad_logprob,
                                             check_mask, int(n_tail))
        return res, grad, dict(zip(names, pg))

    def _score_backward(self, who: str, embeds, key_mask, targets, grad_logprob, check_mask: bool, n_tail: int):
        if getattr(self, "grad_desc", None) is None:
            raise N.VcapError(f"{who}: call enable_grad(sd) first", N.E_ARG)
        if targets is None:
            raise ValueError(f"{who}: targets are required")
        x = embeds.to(self.device, torch.float32).contiguous()
        if x.dim() != 3 or x.shape[2] != self.arch.n_embd:
            raise ValueError(f"embeds shape {tuple(x.shape)} != [B, S, {self.arch.n_embd}]")
        B, S, _ = x.shape
        max_rows = int(N.lib().vcap_gpt2_max_rows())
        if B < 1 or S < 1 or S > max_rows or S > self.arch.n_positions:
            raise N.VcapError(f"{who}: S = {S} exceeds vcap_gpt2_max_rows() = {max_rows} or n_positions",
                              N.E_UNSUPPORTED)
        km = gw = None
        if key_mask is not None:
            km = (key_mask != 0).to(self.device, torch.uint8).contiguous()
            if tuple(km.shape) != (B, S):
                raise ValueError(f"key_mask shape {tuple(km.shape)} != {(B, S)}")
            if check_mask and not bool(km[:, 0].all()):
                raise N.VcapError(f"{who}: key_mask[:, 0] must be nonzero (a row with no visible key)", N.E_ARG)
        tg = targets.to(self.device, torch.int32).contiguous()
        if tuple(tg.shape) != (B, S):
            raise ValueError(f"targets shape {tuple(tg.shape)} != {(B, S)}")
        if grad_logprob is not None:
            gw = grad_logprob.to(self.device, torch.float32).contiguous()
            if tuple(gw.shape) != (B, S):
                raise ValueError(f"grad_logprob shape {tuple(gw.shape)} != {(B, S)}")
        logprobs = torch.empty(B, S, dtype=torch.float32, device=self.device)
        grad = torch.empty_like(x)
        per = max(1, max_rows // S)
        starts = list(range(0, B, per))
        pairs = torch.empty(len(starts), 2, dtype=torch.float32, device=self.device)
        stream = _stream(self.device)
        lib = N.lib()
        total = None   # the tail call: the chunks' parameter gradients, added in chunk order
        if n_tail:
            shapes = [self._tail_shape(k) for k in self.tail_names(n_tail)]
            per_layer = len(self.TAIL_PARAMS)
        for ci, b0 in enumerate(starts):
            nb = min(per, B - b0)
            args = (x[b0:].data_ptr(), nb, S, N.ptr(None if km is None else km[b0:]), tg[b0:].data_ptr(),
                    N.ptr(None if gw is None else gw[b0:]), grad[b0:].data_ptr())
            outs = (logprobs[b0:].data_ptr(), pairs[ci].data_ptr())
            if not n_tail:
                ws = self.ws.get(int(lib.vcap_gpt2_score_backward_workspace_bytes(C.byref(self.desc),
                                                                                  C.byref(self.grad_desc), nb, S)))
                N.check(lib.vcap_gpt2_score_backward(C.byref(self.desc), C.byref(self.grad_desc), *args, *outs,
                                                     ws.data_ptr(), ws.numel(), stream), "vcap_gpt2_score_backward")
                continue
            pgs = [torch.empty(sh, dtype=torch.float32, device=self.device) for sh in shapes]
            layers = (N.GPT2ParamGradsLayer * n_tail)()
            for i in range(n_tail):
                for j, (field, _) in enumerate(N.GPT2ParamGradsLayer._fields_):
                    setattr(layers[i], field, pgs[i * per_layer + j].data_ptr())
            pg = N.GPT2ParamGrads(n_tail=n_tail, layers=layers)
            ws = self.ws.get(int(lib.vcap_gpt2_score_backward_tail_workspace_bytes(
                C.byref(self.desc), C.byref(self.grad_desc), nb, S, n_tail)))
            N.check(lib.vcap_gpt2_score_backward_tail(C.byref(self.desc), C.byref(self.grad_desc), *args, C.byref(pg),
                                                      *outs, ws.data_ptr(), ws.numel(), stream),
                    "vcap_gpt2_score_backward_tail")
            total = pgs if total is None else [a + b for a, b in zip(total, pgs)]
        nll_sum, count = pairs[0, 0], pairs[0, 1]
        for ci in range(1, len(starts)):   # chunk order, as score()
            nll_sum, count = nll_sum + pairs[ci, 0], count + pairs[ci, 1]
        return ScoreResult(None, logprobs, nll_sum, count), grad, total

    @torch.no_grad()
    def load_tail(self, state: Dict[str, torch.Tensor]) -> None:
        """Rewrite, in place, every device copy of the transformer-block parameters named in `state`
        (decoder.model.transformer.h.{i}.*, f32 values in HF's layouts; other keys are ignored): the
        rows-packed forward weights (vcap_rows_pack into the same buffers), the f32 biases and LayerNorm
        affines, and - after enable_grad - the grad desc's Conv1D and Linear-layout copies.  No pointer in
        desc, layers or grad_desc changes, so captured decode graphs stay valid and replay with the new
        weights.  A bf16 decoder stores the RNE rounding of the f32 values, as __init__ does."""
        tdt = _dtype(self.precision)[1]
        grad_named = getattr(self, "_grad_named", {})
        prefix = "decoder.model.transformer.h."
        for name, v in state.items():
            if not name.startswith(prefix) or name not in self._named:
                continue
            v = torch.as_tensor(v).detach().to(self.device, torch.float32)
            if name.endswith(".weight") and v.dim() == 2:   # Conv1D [in, out]
                self._pack_into(v.t().contiguous().to(tdt).contiguous(), self._named[name])
                for t, src in zip(grad_named.get(name, []), (v, v.t())):   # [in, out], then [out, in]
                    t.copy_(src.to(tdt))
            else:
                if tuple(v.shape) != tuple(self._named[name].shape):
                    raise ValueError(f"{name}: shape {tuple(v.shape)} != {tuple(self._named[name].shape)}")
                self._named[name].copy_(v)
        torch.cuda.synchronize(self.device)   # the copies ran on the current stream; decodes may use others

    def _beam_ids(self, prefix, prompt_ids, cfg: GenConfig, out, workspace, lengths_out):
        B, P, E = prefix.shape
        if P != self.prefix_len or E != self.arch.n_embd:
            raise ValueError(f"prefix shape {tuple(prefix.shape)} != [B,{self.prefix_len},{self.arch.n_embd}]")
        ids, rows = split_prompts(prompt_ids, B, not self.force_ragged)
        mx = int(cfg.max_new_tokens)
        prefix = prefix.to(torch.float32).contiguous()
        out = out if out is not None else torch.empty(B, mx, dtype=torch.int32, device=prefix.device)
        if lengths_out is None:
            lengths_out = torch.empty(B, dtype=torch.int32, device=prefix.device)
        S0 = self.prefix_len + len(ids)
        if rows is not None:
            nbytes = self.ragged_workspace_bytes(rows, mx, int(cfg.num_beams))
        else:
            nbytes = int(N.lib().vcap_gpt2_beam_search_workspace_bytes(C.byref(self.desc), B, int(cfg.num_beams), S0,
                                                                       mx))
        if nbytes == 0 and rows is not None:
            raise N.VcapError("vcap_gpt2_beam_search_ragged_workspace_bytes: unsupported shape (B > 8, num_beams "
                              "outside 2..8, too many prefill rows, or a context past 128)", N.E_UNSUPPORTED)
        if nbytes == 0:
            raise ValueError("vcap_gpt2_beam_search_workspace_bytes: unsupported shape")
        ws = (workspace or self.ws).get(nbytes)
        bp = N.BeamParams(num_beams=int(cfg.num_beams), max_new_tokens=mx, min_new_tokens=int(cfg.min_new_tokens),
                          no_repeat_ngram_size=int(cfg.no_repeat_ngram_size),
                          repetition_penalty=float(cfg.repetition_penalty), length_penalty=float(cfg.length_penalty),
                          early_stopping=0, eos_token_id=int(cfg.eos_token_id), use_graph=int(bool(cfg.use_graph)),
                          max_blocks=int(cfg.max_blocks))
        if rows is not None:
            pr, _ids_keep, _off_keep = _prompts_arg(rows)
            N.check(N.lib().vcap_gpt2_beam_search_ragged(C.byref(self.desc), C.byref(bp), prefix.data_ptr(),
                                                         C.byref(pr), B, out.data_ptr(), lengths_out.data_ptr(),
                                                         ws.data_ptr(), ws.numel(), _stream(prefix.device)),
                    "vcap_gpt2_beam_search_ragged")
            return out
        arr = (C.c_int * max(len(ids), 1))(*ids)
        N.check(N.lib().vcap_gpt2_beam_search(C.byref(self.desc), C.byref(bp), prefix.data_ptr(), arr, len(ids), B,
                                              out.data_ptr(), lengths_out.data_ptr(), ws.data_ptr(), ws.numel(),
                                              _stream(prefix.device)), "vcap_gpt2_beam_search")
        return out


def trim_generated(ids: torch.Tensor, eos: int) -> List[List[int]]:
    """HF generate output length: it stops after the first step where every row has finished
    (generation/utils.py stopping criteria); rows finished earlier are EOS-padded."""
    a = ids.cpu().numpy()
    B, L = a.shape
    fin = np.zeros(B, dtype=bool)
    stop = L
    for s in range(L):
        fin |= a[:, s] == eos
        if fin.all():
            stop = s + 1
            break
    return [list(map(int, a[b, :stop])) for b in range(B)]


def raw_greedy_tokens(ids: torch.Tensor, eos: int) -> List[List[int]]:
    """benchmark_baseline.run_decoder_steps bookkeeping: tokens up to and including the first EOS."""
    out = []
    for row in ids.cpu().numpy().tolist():
        toks = []
        for t in row:
            toks.append(int(t))
            if t == eos:
                break
        out.append(toks)
    return out
