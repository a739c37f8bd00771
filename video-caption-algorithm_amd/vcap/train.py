"""Mapper fine-tuning on the device path: the reference's recipe (src/cli/train_caption_mapper.py - ViT
frozen, decoder.mapper trained with AdamW on the teacher-forced LM loss, GPT-2 frozen or, with
--unfreeze_gpt2_last N, its last N blocks trained in a second AdamW group at --lr_gpt2) with GPT-2 on the
HIP kernels.

With GPT-2 frozen the only gradient the recipe needs from it is that of the loss with respect to
inputs_embeds: HipGPT2Decoder.score_backward (vcap_gpt2_score_backward).  ScoreLogProbs wraps it as a
torch.autograd.Function, so the 0.79 M mapper parameters - an ordinary torch nn.Linear in front of it - get
their gradients from torch autograd.  The same Function serves soft-prompt / prefix tuning and embedding
saliency: anything that is a function of inputs_embeds.

With the tail unfrozen, ScoreLogProbsTail takes the 12 N block parameters as extra inputs and returns their
gradients from the one device call HipGPT2Decoder.score_backward_tail (vcap_gpt2_score_backward_tail); its
embedding gradient is score_backward's, bit for bit.  The parameters live as f32 torch nn.Parameters (the
masters AdamW updates); MapperTrainer.step() writes them back into the decoder's device weights with
HipGPT2Decoder.load_tail after every optimizer step (a bf16 decoder stores their RNE roundings), in place,
so captured decode graphs stay valid.  ln_f, wte and wpe stay frozen, as in the reference.

Differences from the reference, both deliberate:
  * The reference calls .train() on the whole model, so its GPT-2 applies dropout noise (attn / resid /
    embd pdrop 0.1), in the unfrozen blocks too.  The device GPT-2 is deterministic.  The mapper's own
    nn.Dropout stays, in torch.
  * cond_mode="bos" is not supported.
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence

import numpy as np
import torch
import torch.nn as nn

from .model import HipGPT2Decoder

MAPPER_W, MAPPER_B = "decoder.mapper.0.weight", "decoder.mapper.0.bias"


class ScoreLogProbs(torch.autograd.Function):
    """logprobs [B, S] = HipGPT2Decoder.score(embeds, key_mask, targets).logprobs, differentiable with
    respect to `embeds` ONLY: backward calls score_backward with the incoming grad_output as the per-position
    weights.  The decoder's weights are frozen, the logits are not an output of this path (no gradient
    reaches or leaves them), and key_mask / targets are not differentiable.  The forward runs once more
    inside the backward call (the residual stream is not kept between the two)."""

    @staticmethod
    def forward(ctx, embeds: torch.Tensor, hip: HipGPT2Decoder, key_mask: Optional[torch.Tensor],
                targets: torch.Tensor, check_mask: bool = True) -> torch.Tensor:
        x = embeds.detach().to(hip.device, torch.float32).contiguous()
        ctx.hip, ctx.key_mask, ctx.targets = hip, key_mask, targets
        ctx.save_for_backward(x)
        return hip.score(x, key_mask, targets, check_mask=check_mask).logprobs

    @staticmethod
    def backward(ctx, grad_output: torch.Tensor):
        (x,) = ctx.saved_tensors
        _, grad = ctx.hip.score_backward(x, ctx.key_mask, ctx.targets, grad_output, check_mask=False)
        return grad, None, None, None, None


class ScoreLogProbsTail(torch.autograd.Function):
    """ScoreLogProbs, also differentiable with respect to every parameter of the last n_tail blocks:
    `tail_params` are the f32 tensors of HipGPT2Decoder.tail_names(n_tail), in that order and in HF's layouts.
    The device computes with its own copies of them (HipGPT2Decoder.load_tail keeps those current); the
    inputs exist so that autograd routes the gradients.  backward is one score_backward_tail call."""

    @staticmethod
    def forward(ctx, embeds: torch.Tensor, hip: HipGPT2Decoder, key_mask: Optional[torch.Tensor],
                targets: torch.Tensor, check_mask: bool, n_tail: int, *tail_params: torch.Tensor) -> torch.Tensor:
        names = hip.tail_names(n_tail)
        if len(tail_params) != len(names):
            raise ValueError(f"{len(tail_params)} tail parameters given, n_tail = {n_tail} has {len(names)}")
        x = embeds.detach().to(hip.device, torch.float32).contiguous()
        ctx.hip, ctx.key_mask, ctx.targets, ctx.n_tail, ctx.names = hip, key_mask, targets, int(n_tail), names
        ctx.save_for_backward(x)
        return hip.score(x, key_mask, targets, check_mask=check_mask).logprobs

    @staticmethod
    def backward(ctx, grad_output: torch.Tensor):
        (x,) = ctx.saved_tensors
        _, grad, pg = ctx.hip.score_backward_tail(x, ctx.key_mask, ctx.targets, grad_output, ctx.n_tail,
                                                  check_mask=False)
        return (grad, None, None, None, None, None, *[pg[k] for k in ctx.names])


def lm_loss(decoder, prefix: torch.Tensor, input_ids: torch.Tensor,
            attention_mask: Optional[torch.Tensor] = None, labels: Optional[torch.Tensor] = None,
            tail: Optional[Dict[str, torch.Tensor]] = None) -> torch.Tensor:
    """GPT2TextDecoder.forward's loss as a differentiable scalar: nll_sum / count over the shifted labels,
    with HipTextDecoder.forward_from_prefix's inputs (the same shift and mask construction:
    HipTextDecoder.score_inputs).  `decoder` is a vcap.caption.HipTextDecoder after enable_grad;
    prefix [B, P, E] carries the graph.  labels default to input_ids, as in HF.  tail: {state-dict name:
    parameter} of the last N blocks (tail_parameters), which then receive gradients too."""
    if labels is None:
        labels = input_ids
    x, km, targets = decoder.score_inputs(prefix, input_ids, attention_mask, labels)
    if tail:
        n_tail = len(tail) // len(decoder.hip.TAIL_PARAMS)
        params = [tail[k] for k in decoder.hip.tail_names(n_tail)]
        lp = ScoreLogProbsTail.apply(x, decoder.hip, km, targets, prefix.shape[1] == 0, n_tail, *params)
    else:
        lp = ScoreLogProbs.apply(x, decoder.hip, km, targets, prefix.shape[1] == 0)
    count = ((targets >= 0) & (targets < decoder.arch.vocab)).sum()
    return -lp.sum() / count


def compute_loss(model, video_emb: torch.Tensor, caption_ids: torch.Tensor, pad_id: int,
                 mapper: nn.Module, tail: Optional[Dict[str, torch.Tensor]] = None) -> torch.Tensor:
    """The reference's training loss (train_caption_mapper.py compute_loss_local) on cached clip embeddings:
    video_emb [B, video_dim] = proj(encoder(video)) (proj is the identity), caption_ids [B, L] = <bos> ...
    <eos> right-padded with pad_id.  inputs = caption_ids[:, :-1], labels = caption_ids[:, 1:], key mask =
    inputs != pad_id with ones for the prefix, the prefix positions not counted.  `mapper` is a torch
    module video_dim -> P * E whose parameters receive the gradient; `model` is a HipVideoCaptionModel (or
    a HipTextDecoder); tail: lm_loss's."""
    dec = getattr(model, "decoder", model)
    dev = dec.hip.device
    emb = video_emb.to(dev, torch.float32)
    B = emb.shape[0]
    prefix = mapper(emb.reshape(B, -1)).reshape(B, dec.prefix_len, dec.arch.n_embd)
    ids = caption_ids.to(dev).long()
    inp, labels = ids[:, :-1], ids[:, 1:]
    return lm_loss(dec, prefix, inp, inp != pad_id, labels, tail)


def tail_parameters(hip: HipGPT2Decoder, sd: Dict[str, np.ndarray], n_tail: int) -> Dict[str, nn.Parameter]:
    """{state-dict name: f32 nn.Parameter on the decoder's device} for every parameter of the last n_tail
    blocks, from the state dict the decoder was built from, in HipGPT2Decoder.tail_names order."""
    return {k: nn.Parameter(torch.from_numpy(np.ascontiguousarray(sd[k], np.float32)).to(hip.device))
            for k in hip.tail_names(n_tail)}


class MapperTrainer:
    """decoder.mapper as a torch nn.Sequential(nn.Linear(video_dim, P * E), nn.Dropout) initialised from
    the checkpoint's decoder.mapper.0.*, trained with AdamW(lr 3e-4, weight_decay 0.01) as the reference
    trains it; GPT-2 runs on the device.  unfreeze_gpt2_last = N > 0: the last N blocks train too, as f32
    nn.Parameters in a second AdamW group at lr_gpt2 (the reference's --unfreeze_gpt2_last / --lr_gpt2); after
    every optimizer step they are written back into the decoder's device weights (load_tail).  N = 0 is the
    mapper-only trainer: the same calls, the same bits."""

    def __init__(self, model, sd: Dict[str, np.ndarray], pad_id: Optional[int] = None, lr: float = 3e-4,
                 weight_decay: float = 0.01, dropout: float = 0.1, unfreeze_gpt2_last: int = 0,
                 lr_gpt2: float = 1e-5):
        self.model = model
        self.decoder = getattr(model, "decoder", model)
        dev = self.decoder.hip.device
        self.decoder.hip.enable_grad(sd)
        w = torch.from_numpy(np.ascontiguousarray(sd[MAPPER_W], np.float32))
        b = torch.from_numpy(np.ascontiguousarray(sd[MAPPER_B], np.float32))
        lin = nn.Linear(w.shape[1], w.shape[0])
        with torch.no_grad():
            lin.weight.copy_(w)
            lin.bias.copy_(b)
        self.mapper = nn.Sequential(lin, nn.Dropout(dropout)).to(dev)
        self.pad_id = self.decoder.arch.eos_token_id if pad_id is None else int(pad_id)
        self.n_tail = int(unfreeze_gpt2_last)
        self.tail: Dict[str, nn.Parameter] = {}
        if self.n_tail > 0:
            self.tail = tail_parameters(self.decoder.hip, sd, self.n_tail)
            groups = [{"params": list(self.mapper.parameters()), "lr": lr},
                      {"params": list(self.tail.values()), "lr": lr_gpt2}]
            self.optimizer = torch.optim.AdamW(groups, weight_decay=weight_decay)
        else:
            self.optimizer = torch.optim.AdamW(self.mapper.parameters(), lr=lr, weight_decay=weight_decay)
        self.steps = 0

    def step(self, video_emb: torch.Tensor, caption_ids: torch.Tensor) -> float:
        """One optimiser step on a batch; returns the batch's loss before the step."""
        self.mapper.train()
        loss = compute_loss(self.model, video_emb, caption_ids, self.pad_id, self.mapper, self.tail or None)
        self.optimizer.zero_grad()
        loss.backward()
        self.optimizer.step()
        if self.tail:
            self.load_tail()
        self.steps += 1
        return float(loss)

    @torch.no_grad()
    def evaluate(self, video_emb: torch.Tensor, caption_ids: torch.Tensor) -> float:
        """The loss of a batch with the mapper in eval mode (dropout off), no gradient."""
        self.mapper.eval()
        return float(compute_loss(self.model, video_emb, caption_ids, self.pad_id, self.mapper))

    def state_dict(self) -> Dict[str, torch.Tensor]:
        """{decoder.mapper.0.weight, decoder.mapper.0.bias} and, with an unfrozen tail, its
        decoder.model.transformer.h.{i}.* tensors (f32 masters, HF's layouts), on the CPU: the checkpoint's
        names."""
        lin = self.mapper[0]
        out = {MAPPER_W: lin.weight.detach().cpu().clone(), MAPPER_B: lin.bias.detach().cpu().clone()}
        out.update({k: p.detach().cpu().clone() for k, p in self.tail.items()})
        return out

    def load_tail(self) -> None:
        """Write the tail's f32 masters into the decoder's device weights, in place."""
        self.decoder.hip.load_tail({k: p.detach() for k, p in self.tail.items()})

    def load_mapper(self) -> None:
        """Write the trained weights into the live device mappers (HipTextDecoder.mapper_op and, on a
        HipVideoCaptionModel, the engine prefix), so generate() uses them without a reload."""
        load_mapper(self.model, self.state_dict())


def load_mapper(model, state: Dict[str, torch.Tensor]) -> None:
    """Copy decoder.mapper.0.{weight, bias} from `state` into the model's live HipPrefix objects, in place
    (their descriptors keep pointing at the same device tensors)."""
    dec = getattr(model, "decoder", model)
    ops = [dec.mapper_op]
    if getattr(model, "_engine_prefix", None) is not None:
        ops.append(model._engine_prefix)
    w, b = torch.as_tensor(state[MAPPER_W]), torch.as_tensor(state[MAPPER_B])
    for op in ops:
        if tuple(w.shape) != tuple(op.mapper_w.shape):
            raise ValueError(f"mapper weight {tuple(w.shape)} != {tuple(op.mapper_w.shape)}")
        with torch.no_grad():
            op.mapper_w.copy_(w.to(op.mapper_w.device, torch.float32))
            op.mapper_b.copy_(b.to(op.mapper_b.device, torch.float32))
