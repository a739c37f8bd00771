"""Shared by test_cpu_score.py and test_gpu_score.py: the masked fp64 forward that is the oracle of the
teacher-forced scoring call (vcap_gpt2_score), the synthetic 2-layer decoders it is checked on, and the
inputs / masks / targets of the cases.

masked_forward is decoder_shapes.emulated_forward with attn_mask = causal & key_mask: query i of
sequence b sees the keys j <= i with key_mask[b, j] != 0; positions stay 0..S-1 whatever the mask
holds (HF's GPT2LMHeadModel(inputs_embeds=, attention_mask=) in a plain forward: test_cpu_score.py pins
this against the reference's own output, tests/golden/score_tiny.npz).  With rnd = bf16_rne and the
bf16-rounded weights it is the bf16 model of the kernels (decoder_shapes' docstring lists where they
round; the all-rows lm_head rounds ln_f's output at the same point as PRO_LN)."""
from __future__ import annotations

from functools import lru_cache
from typing import NamedTuple, Optional

import numpy as np
import torch
import torch.nn.functional as F

import decoder_shapes as DS
from oracle import vcap_oracle as O
from vcap import weights
from vcap.configs import GPT2Arch

P = DS.P
LNF_W, LNF_B = P + "ln_f.weight", P + "ln_f.bias"
PREFIX_LEN = DS.PREFIX_LEN
IGNORE = -100


def arch(E: int, V: int = DS.VOCAB, npos: int = DS.NPOS) -> GPT2Arch:
    return GPT2Arch(f"score_{E}_{V}", E, DS.NLAYER, E // 64, vocab=V, n_positions=npos,
                    bos_token_id=V - 1, eos_token_id=V - 1)


@lru_cache(maxsize=None)
def state_dict(E: int, V: int = DS.VOCAB, gain: float = 1.0):
    """Seeded weights; `gain` multiplies ln_f's weight and bias, so every logit scales by it exactly."""
    sd = dict(weights.synthetic_gpt2(DS.WEIGHT_SEED, arch(E, V)))
    if gain != 1.0:
        sd[LNF_W] = (sd[LNF_W].astype(np.float64) * gain).astype(np.float32)
        sd[LNF_B] = (sd[LNF_B].astype(np.float64) * gain).astype(np.float32)
    return sd


@lru_cache(maxsize=None)
def sd64(E: int, V: int = DS.VOCAB, gain: float = 1.0, rounded: bool = False):
    out = {}
    for k, v in state_dict(E, V, gain).items():
        t = torch.from_numpy(np.ascontiguousarray(v)).double()
        if rounded and (k.endswith(DS._MATS) or k in (DS.WTE, "decoder.model.lm_head.weight")):
            t = DS.bf16_rne(t)
        out[k] = t
    return out


def masked_forward(sd, ar, inputs_embeds, key_mask=None, rnd=DS._ident):
    """Logits [B, S, V] of one forward over inputs_embeds [B, S, E]; key_mask [B, S] (nonzero = visible)
    or None.  The operations of decoder_shapes.emulated_forward in its order, so a None mask gives its
    result bit for bit."""
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
        a = rnd(F.layer_norm(h, (e,), sd[b + "ln_1.weight"], sd[b + "ln_1.bias"], ar.ln_eps))
        qkv = rnd(a @ sd[b + "attn.c_attn.weight"] + sd[b + "attn.c_attn.bias"])
        q, k, v = (t.reshape(bsz, s, nh, hd).transpose(1, 2) for t in qkv.split(e, dim=2))
        att = rnd(F.scaled_dot_product_attention(q, k, v, attn_mask=mask))
        att = att.transpose(1, 2).reshape(bsz, s, e)
        h = h + (att @ sd[b + "attn.c_proj.weight"] + sd[b + "attn.c_proj.bias"])
        m = rnd(F.layer_norm(h, (e,), sd[b + "ln_2.weight"], sd[b + "ln_2.bias"], ar.ln_eps))
        m = rnd(O._gelu_new(m @ sd[b + "mlp.c_fc.weight"] + sd[b + "mlp.c_fc.bias"]))
        h = h + (m @ sd[b + "mlp.c_proj.weight"] + sd[b + "mlp.c_proj.bias"])
    h = rnd(F.layer_norm(h, (e,), sd[P + "ln_f.weight"], sd[P + "ln_f.bias"], ar.ln_eps))
    return h @ sd["decoder.model.lm_head.weight"].t()


def target_logprobs(logits: torch.Tensor, targets: torch.Tensor):
    """-> (logprob [B, S] float64, 0 where targets == -100; nll_sum; count)."""
    t = torch.as_tensor(targets).long()
    lp = F.log_softmax(logits.double(), dim=-1).gather(2, t.clamp(min=0)[..., None])[..., 0]
    live = t >= 0
    lp = torch.where(live, lp, torch.zeros_like(lp))
    return lp, float(-lp.sum()), int(live.sum())


def shift_labels(labels: torch.Tensor, prefix_len: int = PREFIX_LEN) -> torch.Tensor:
    """HF's in-model shift: labels [B, L] of the text -> targets [B, P + L] (the logits at position i
    are scored against label i + 1; the prefix and the last position score nothing)."""
    lab = torch.as_tensor(labels).long()
    ext = torch.cat([torch.full((lab.shape[0], prefix_len), IGNORE, dtype=torch.long), lab], dim=1)
    return torch.cat([ext[:, 1:], torch.full((lab.shape[0], 1), IGNORE, dtype=torch.long)], dim=1)


class Case(NamedTuple):
    name: str
    E: int
    V: int
    B: int
    S: int
    mask: str = "none"       # none | ones | right | interior
    targets: str = "mixed"   # mixed | edges | ignored
    gain: float = 1.0


def embeds(c: Case) -> torch.Tensor:
    """f32 [B, S, E]: 0.1 * randn prefix rows, then the model's own wte rows of seeded tokens."""
    g = torch.Generator().manual_seed(7 * c.E + 1000 * c.B + c.S + 31 * c.V)
    pre = 0.1 * torch.randn(c.B, min(PREFIX_LEN, c.S), c.E, generator=g, dtype=torch.float32)
    ids = torch.randint(0, c.V, (c.B, c.S - pre.shape[1]), generator=g)
    wte = torch.from_numpy(np.ascontiguousarray(state_dict(c.E, c.V, c.gain)[DS.WTE]))
    return torch.cat([pre, wte[ids]], dim=1)


def key_mask(c: Case) -> Optional[torch.Tensor]:
    if c.mask == "none":
        return None
    m = torch.ones(c.B, c.S, dtype=torch.uint8)
    if c.mask == "right":        # lengths S, S - 3, 5, ...
        for b, n in enumerate([c.S, c.S - 3, 5] * c.B):
            if b < c.B:
                m[b, n:] = 0
    elif c.mask == "interior":   # position 4 (the BOS slot after a 4-token prefix), the key right before
        m[:, 4] = 0              # the last query, and scattered ones
        m[:, c.S - 2] = 0
        m[0, 2] = 0
        m[c.B - 1, 7:9] = 0
    return m


def targets(c: Case) -> torch.Tensor:
    g = torch.Generator().manual_seed(13 * c.E + c.B + 100 * c.S + c.V)
    t = torch.randint(0, c.V, (c.B, c.S), generator=g)
    if c.targets == "ignored":
        return torch.full((c.B, c.S), IGNORE, dtype=torch.long)
    # the vocabulary's first and last column, the last column of a full 128-column tile and of its
    # first 64-column half, and ignored rows
    t[0, 0], t[0, 1], t[0, 2], t[0, 3] = 0, c.V - 1, 127, 63
    t[c.B - 1, c.S - 1] = c.V - 1
    t[c.B - 1, 0] = 128 * ((c.V - 1) // 128) - 1
    t[0, 4] = IGNORE
    t[c.B - 1, c.S // 2] = IGNORE
    if c.targets == "edges":
        t[:, c.S - 2] = IGNORE
    return t


@lru_cache(maxsize=None)
def reference(c: Case, mode: str = "fp64") -> torch.Tensor:
    """Oracle logits [B, S, V] float64 of the case: "fp64", or "bf16" (the kernels' roundings)."""
    ar = arch(c.E, c.V)
    with torch.no_grad():
        if mode == "fp64":
            return masked_forward(sd64(c.E, c.V, c.gain), ar, embeds(c).double(), key_mask(c))
        return masked_forward(sd64(c.E, c.V, c.gain, rounded=True), ar, embeds(c).double(), key_mask(c), DS.bf16_rne)
