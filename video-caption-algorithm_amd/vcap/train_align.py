"""Alignment-model training on the device path: the reference's src/cli/train_full.py --model vit
--freeze_vit recipe (ViTTextAlignModel, AdamW, CosineEmbeddingLoss(encode_video, encode_text, +1)) with the
whole text tower's forward and backward on the HIP kernels.

With the ViT frozen the video side is the cached clip feature - the frame mean of the ViT's CLS output -
through vid_proj, a 768 -> 256 nn.Linear that stays an ordinary torch module (as decoder.mapper does in
vcap/train.py).  The text side is HipTextEmbedder: EncodeText wraps encode_text / encode_text_backward
(vcap_text_encode_backward) as a torch.autograd.Function whose inputs are the tower's parameters - f32
masters under the reference's names - so torch's AdamW updates them; after each step the masters are written
back into the device weights in place (HipTextEmbedder.load_state_dict).

grad_out is arbitrary, so any loss of the unit-norm text rows trains through the same Function; an in-batch
contrastive loss, for instance:
    F.cross_entropy(v @ encode(ids).t() / 0.07, torch.arange(len(v), device=v.device))

With a video encoder (AlignTrainer(..., video_encoder=HipViTEncoder)) the recipe is the reference's default,
train_full.py --model vit without --freeze_vit: the batch holds frames, EncodeVideo wraps HipViTEncoder.encode /
encode_backward (vcap_vit_encode_backward) the way EncodeText wraps the text tower, vid_proj lives on the device
as encoder.proj (video_dim = proj_dim), and AdamW also updates the f32 masters of the last `unfreeze_vit_last`
ViT blocks (0: every block, plus the patch embedding, class token and positional table).  F.normalize, the loss
and AdamW stay in torch.

Differences from the reference, all deliberate:
  * The device towers are deterministic: no dropout.  The reference's .train() applies p = 0.1 inside the
    text encoder layers (the same choice as for the mapper, vcap/train.py); timm's ViT has none in this recipe.
  * ViT training serves fp32 and bf16 operands; fp16 / MXFP8 encoders are refused (HipViTEncoder.enable_grad).
  * --model simple (SimpleAlignModel) is not ported.
"""
from __future__ import annotations

from typing import Dict, List, Optional

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from .retrieval import F_NORMALIZE_EPS, HipTextEmbedder, text_tower_state_dict

VID_W, VID_B = "vid_proj.weight", "vid_proj.bias"


def align_param_name(name: str) -> str:
    """The encoder's state-dict name -> ViTTextAlignModel's: encoder.backbone.* -> vit.*, encoder.proj.* ->
    vid_proj.* (the inverse of vcap.retrieval.remap_alignment_state_dict's renaming)."""
    if name.startswith("encoder.backbone."):
        return "vit." + name[len("encoder.backbone."):]
    if name.startswith("encoder.proj."):
        return "vid_proj." + name[len("encoder.proj."):]
    raise KeyError(f"not an encoder parameter: {name}")


def encoder_param_name(name: str) -> str:
    """ViTTextAlignModel's name -> the encoder's: vit.* -> encoder.backbone.*, vid_proj.* -> encoder.proj.*."""
    if name.startswith("vit."):
        return "encoder.backbone." + name[len("vit."):]
    if name.startswith("vid_proj."):
        return "encoder.proj." + name[len("vid_proj."):]
    raise KeyError(f"not a video-side parameter of the alignment model: {name}")


def scatter_embedding_grad(sparse, vocab: int) -> torch.Tensor:
    """(ids [count] distinct, rows [count, E]) -> the dense [vocab, E] gradient of txt_emb.weight: zeros with
    the listed rows copied in.  The ids are distinct, so index_copy_ is deterministic; the pad row and every
    id the batch does not hold stay zero."""
    ids, rows = sparse
    dense = torch.zeros(vocab, rows.shape[1], dtype=rows.dtype, device=rows.device)
    return dense.index_copy_(0, ids, rows)


class EncodeText(torch.autograd.Function):
    """out [B, proj_dim] = embedder.encode_text(ids), differentiable with respect to the tower's parameters:
    `params` are tensors in embedder.param_names() order whose values the embedder's device weights hold
    (the caller keeps them equal: HipTextEmbedder.load_state_dict).  backward calls encode_text_backward
    with the incoming grad_output and hands each parameter its gradient; the forward runs once more inside
    that call (no activation is kept between the two)."""

    @staticmethod
    def forward(ctx, embedder: HipTextEmbedder, ids, *params: torch.Tensor) -> torch.Tensor:
        ctx.embedder, ctx.ids = embedder, ids
        ctx.devices = [p.device for p in params]
        return embedder.encode_text(ids)

    @staticmethod
    def backward(ctx, grad_output: torch.Tensor):
        emb = ctx.embedder
        _, grads = emb.encode_text_backward(ctx.ids, grad_output)
        out = []
        for name, dev in zip(emb.param_names(), ctx.devices):
            g = grads[name]
            if isinstance(g, tuple):
                g = scatter_embedding_grad(g, emb.vocab)
            out.append(g.to(dev))
        return (None, None, *out)


class EncodeVideo(torch.autograd.Function):
    """enc_out [B, video_dim] = encoder.encode(video), differentiable with respect to the encoder's trainable
    parameters: `params` are tensors in encoder.param_names(n_tail) order whose values the encoder's device
    operands hold (the caller keeps them equal: HipViTEncoder.load_state_dict).  backward calls
    encode_backward with the incoming grad_output; the forward runs once more inside that call."""

    @staticmethod
    def forward(ctx, encoder, video, n_tail: int, *params: torch.Tensor) -> torch.Tensor:
        ctx.encoder, ctx.video, ctx.n_tail = encoder, video, n_tail
        ctx.devices = [p.device for p in params]
        return encoder.encode(video)[0]

    @staticmethod
    def backward(ctx, grad_output: torch.Tensor):
        enc = ctx.encoder
        _, grads = enc.encode_backward(ctx.video, grad_output, ctx.n_tail)
        return (None, None, None, *(grads[k].to(d) for k, d in zip(enc.param_names(ctx.n_tail), ctx.devices)))


class AlignTrainer:
    """vid_proj (torch nn.Linear) and the text tower (device) trained as the reference trains them:
    AdamW(lr) over vid_proj plus every txt_* parameter on cosine_embedding_loss(normalize(vid_proj(feat)),
    encode_text(ids), ones).  `sd` holds vid_proj.* and txt_* under the reference's checkpoint names.

    video_encoder (a HipViTEncoder built from the same `sd`, video_dim = the tower's proj_dim): the ViT trains
    too.  step / loss / evaluate then take frames [B, T, 3, H, W] instead of cached features, vid_proj is the
    encoder's own encoder.proj, and the last unfreeze_vit_last blocks (0: all of them) are updated with it;
    `sd` must also hold the alignment model's vit.* tensors."""

    def __init__(self, text_embedder: HipTextEmbedder, sd: Dict[str, np.ndarray], lr: float = 5e-4,
                 video_encoder=None, unfreeze_vit_last: int = 0):
        if isinstance(sd, dict) and "model_state" in sd:
            sd = sd["model_state"]
        self.text = text_embedder.enable_grad()
        dev = self.text.device
        tower = text_tower_state_dict(sd)
        self.names: List[str] = self.text.param_names()
        self.params = [nn.Parameter(torch.from_numpy(tower[k]).to(dev)) for k in self.names]
        self.video = video_encoder
        if video_encoder is not None:
            self._init_video(sd, lr, int(unfreeze_vit_last))
            return
        if unfreeze_vit_last:
            raise ValueError("unfreeze_vit_last needs a video_encoder")
        w, b = (torch.as_tensor(np.asarray(sd[k], dtype=np.float32)) for k in (VID_W, VID_B))
        if w.shape[0] != self.text.proj_dim:
            raise ValueError(f"vid_proj.weight {tuple(w.shape)} does not project to the tower's {self.text.proj_dim}")
        self.vid_proj = nn.Linear(w.shape[1], w.shape[0]).to(dev)
        with torch.no_grad():
            self.vid_proj.weight.copy_(w)
            self.vid_proj.bias.copy_(b)
        self.optimizer = torch.optim.AdamW(list(self.vid_proj.parameters()) + self.params, lr=lr)
        self.steps = 0
        self._push()

    def _init_video(self, sd, lr: float, unfreeze_vit_last: int) -> None:
        from .retrieval import remap_alignment_state_dict
        enc = self.video
        if enc.video_dim != self.text.proj_dim:
            raise ValueError(f"the encoder projects to {enc.video_dim}, the text tower to {self.text.proj_dim}")
        self.vit_n_tail = unfreeze_vit_last or enc.arch.depth
        self._vit_sd = remap_alignment_state_dict(sd)   # encoder.* names; the frozen tensors stay as they are here
        enc.enable_grad(self._vit_sd, self.vit_n_tail)
        self.vit_names: List[str] = enc.param_names(self.vit_n_tail)
        self.vit_params = [nn.Parameter(torch.from_numpy(self._vit_sd[k]).to(enc.device)) for k in self.vit_names]
        self.vid_proj = None
        self.optimizer = torch.optim.AdamW(self.vit_params + self.params, lr=lr)
        self.steps = 0
        self._push()

    def _push(self) -> None:
        self.text.load_state_dict(dict(zip(self.names, self.params)))
        if self.video is not None:
            self.video.load_state_dict({k: p.detach() for k, p in zip(self.vit_names, self.vit_params)})

    def encode_text(self, ids) -> torch.Tensor:
        return EncodeText.apply(self.text, ids, *self.params)

    def encode_video(self, feat: torch.Tensor) -> torch.Tensor:
        """feat [B, vid_dim]: the cached frame mean of the frozen ViT's CLS output; with a video encoder:
        frames [B, T, 3, H, W]."""
        if self.video is not None:
            frames = feat.to(self.video.device, torch.float32)
            enc = EncodeVideo.apply(self.video, frames, self.vit_n_tail, *self.vit_params)
            return F.normalize(enc, dim=-1, eps=F_NORMALIZE_EPS)
        feat = feat.to(self.text.device, torch.float32)
        return F.normalize(self.vid_proj(feat), dim=-1, eps=F_NORMALIZE_EPS)

    def loss(self, feat: torch.Tensor, ids) -> torch.Tensor:
        v, t = self.encode_video(feat), self.encode_text(ids)
        return F.cosine_embedding_loss(v, t, torch.ones(v.shape[0], device=v.device))

    def step(self, feat: torch.Tensor, ids) -> float:
        """One optimiser step on a batch; returns the batch's loss before the step."""
        loss = self.loss(feat, ids)
        self.optimizer.zero_grad()
        loss.backward()
        self.optimizer.step()
        self._push()
        self.steps += 1
        return float(loss)

    @torch.no_grad()
    def evaluate(self, feat: torch.Tensor, ids) -> float:
        v, t = self.encode_video(feat), self.text.encode_text(ids)
        return float(F.cosine_embedding_loss(v, t, torch.ones(v.shape[0], device=v.device)))

    def state_dict(self) -> Dict[str, torch.Tensor]:
        """vid_proj.* and txt_* on the CPU under the reference's checkpoint names; with a video encoder also
        every vit.* tensor, the trained ones as trained and the frozen ones as they were loaded."""
        if self.video is not None:
            out = {align_param_name(k): torch.from_numpy(np.array(v, dtype=np.float32)) for k, v in self._vit_sd.items()}
            out.update({align_param_name(k): p.detach().cpu().clone() for k, p in zip(self.vit_names, self.vit_params)})
            out.update({k: p.detach().cpu().clone() for k, p in zip(self.names, self.params)})
            return out
        out = {VID_W: self.vid_proj.weight.detach().cpu().clone(), VID_B: self.vid_proj.bias.detach().cpu().clone()}
        out.update({k: p.detach().cpu().clone() for k, p in zip(self.names, self.params)})
        return out

    def load(self, model) -> None:
        """Write the trained weights into a live HipAlignModel in place: its text embedder's device weights
        and its video encoder's projection (encoder.proj = vid_proj)."""
        state = self.state_dict()
        if model.text_embedder is not self.text:
            model.text_embedder.load_state_dict({k: v for k, v in state.items() if k.startswith("txt_")})
        enc = model.video_embedder.encoder
        if self.video is not None:
            if enc is not self.video:
                enc.load_state_dict({encoder_param_name(k): v for k, v in state.items() if not k.startswith("txt_")})
            return
        if tuple(enc.proj_w.shape) != tuple(state[VID_W].shape):
            raise ValueError(f"vid_proj.weight {tuple(state[VID_W].shape)} != the encoder's {tuple(enc.proj_w.shape)}")
        with torch.no_grad():
            enc.proj_w.copy_(state[VID_W].to(enc.proj_w.device))
            enc.proj_b.copy_(state[VID_B].to(enc.proj_b.device))


def synthetic_align_state_dict(seed: int, vid_dim: int, vocab: int, pad_id: int, txt_dim: int = 512,
                               txt_layers: int = 2, txt_nhead: int = 8, proj_dim: int = 256) -> Dict[str, np.ndarray]:
    """vid_proj.* and txt_* as ViTTextAlignModel.__init__ builds them (torch's default initialisers: nn.Linear,
    nn.Embedding with a zero pad row, nn.TransformerEncoderLayer with dim_feedforward = 4 txt_dim), seeded."""
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(int(seed))
        mods = {"vid_proj": nn.Linear(vid_dim, proj_dim), "txt_emb": nn.Embedding(vocab, txt_dim, padding_idx=pad_id)}
        if txt_layers > 0:
            layer = nn.TransformerEncoderLayer(d_model=txt_dim, nhead=txt_nhead, dim_feedforward=4 * txt_dim,
                                               dropout=0.1, batch_first=True)
            mods["txt_enc"] = nn.TransformerEncoder(layer, num_layers=txt_layers, enable_nested_tensor=False)
        mods["txt_proj"] = nn.Linear(txt_dim, proj_dim)
    return {f"{name}.{k}": v.detach().numpy().copy() for name, m in mods.items() for k, v in m.state_dict().items()}


def clip_features(encoder, video: torch.Tensor) -> torch.Tensor:
    """[B, vid_dim] f32: the frame mean of the frozen ViT's CLS output, before vid_proj - HipViTEncoder built
    with an identity encoder.proj (video_dim = the ViT width).  Run once per clip, without gradients."""
    with torch.no_grad():
        enc = encoder.encode(video)
        enc = enc[0] if isinstance(enc, tuple) else enc
        return enc.reshape(video.shape[0], -1).float()
