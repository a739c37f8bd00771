"""CPU oracle for the ViT-frame-encoder -> GPT-2 caption hot path.

TEST INFRASTRUCTURE ONLY.  This module is the checker: only `tests/`,
`__graft_entry__.smoke()` and `bench.py`'s `cpu_baseline` leg may import it.
The product path (video-caption-algorithm_amd/vcap, core/, src/) never does,
and has no CPU fallback.

A plain fp32 restatement (torch CPU tensors used as an array library) of:
  * timm VisionTransformer.forward_features as patched by the reference
    (src/models/video_encoder.py:112-174: fused SDPA attention, tanh-GELU MLP,
    in-place residual blocks; LayerNorm eps 1e-6), called at :192-197;
  * CLS pooling + temporal mean (video_encoder.py:234-260, pool="cls" from
    src/models/caption_model.py:45), encoder.proj Linear (video_encoder.py:316),
    fp32 cast (:323-324), l2norm off (caption_model.py:46);
  * the engine's prefix normalisation (core/engine.py:44-50, same op as
    core/operators/normalization.py:6-13);
  * GPT2TextDecoder._build_inputs (src/models/text_decoder.py:60-74);
  * HF GPT-2 forward with KV cache (transformers GPT2Model: wpe positions
    past_len+i, pre-LN blocks eps 1e-5, Conv1D x@W+b, gelu_new, tied lm_head);
  * HF `generate` greedy with the reference's kwargs (text_decoder.py:131-144):
    RepetitionPenalty -> NoRepeatNGram -> MinNewTokens(=MinLength) -> argmax,
    EOS padding, stop when all finished (transformers 5.15.0 in this image,
    generation/utils.py:1174-1237 and logits_process.py);
  * the benchmark's raw greedy loop (core/scripts/benchmark_baseline.py:160-240);
  * HF `generate`'s sampling warpers (Temperature -> TopK -> TopP, logits_process.py) and the
    device's documented draw (Philox4x32-10 uniform, inverse CDF over the kept tokens).

Parity pin: tests/golden/make_goldens.py runs the reference's own code
(ViTFrameEncoder, InferenceEngine._generate_once, GPT2TextDecoder.generate)
in the build container and records its outputs; tests/test_cpu_oracle.py
checks this restatement against those fixtures.
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch
import torch.nn.functional as F

Tensor = torch.Tensor


def _t(sd: Dict[str, np.ndarray], key: str) -> Tensor:
    v = sd[key]
    return v if isinstance(v, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(v))


# --------------------------------------------------------------------------- ViT

def vit_forward_features(sd, arch, frames: Tensor) -> Tensor:
    """frames [BT,3,H,W] fp32 -> tokens [BT, N+1, D] after the final norm."""
    p = "encoder.backbone."
    d, heads = arch.dim, arch.heads
    x = F.conv2d(frames, _t(sd, p + "patch_embed.proj.weight"), _t(sd, p + "patch_embed.proj.bias"),
                 stride=arch.patch)
    x = x.flatten(2).transpose(1, 2)  # [BT, P, D]
    cls = _t(sd, p + "cls_token").expand(x.shape[0], -1, -1)
    x = torch.cat([cls, x], dim=1) + _t(sd, p + "pos_embed")
    bt, n, _ = x.shape
    for i in range(arch.depth):
        b = f"{p}blocks.{i}."
        h = F.layer_norm(x, (d,), _t(sd, b + "norm1.weight"), _t(sd, b + "norm1.bias"), arch.ln_eps)
        qkv = F.linear(h, _t(sd, b + "attn.qkv.weight"), _t(sd, b + "attn.qkv.bias"))
        qkv = qkv.reshape(bt, n, 3, heads, d // heads).permute(2, 0, 3, 1, 4)
        q, k, v = qkv.unbind(0)
        a = F.scaled_dot_product_attention(q, k, v)  # scale head_dim^-0.5, no mask
        a = a.transpose(1, 2).reshape(bt, n, d)
        x = x + F.linear(a, _t(sd, b + "attn.proj.weight"), _t(sd, b + "attn.proj.bias"))
        h = F.layer_norm(x, (d,), _t(sd, b + "norm2.weight"), _t(sd, b + "norm2.bias"), arch.ln_eps)
        h = F.gelu(F.linear(h, _t(sd, b + "mlp.fc1.weight"), _t(sd, b + "mlp.fc1.bias")), approximate="tanh")
        x = x + F.linear(h, _t(sd, b + "mlp.fc2.weight"), _t(sd, b + "mlp.fc2.bias"))
    return F.layer_norm(x, (d,), _t(sd, p + "norm.weight"), _t(sd, p + "norm.bias"), arch.ln_eps)


def cls_temporal_pool(feat: Tensor, bsz: int, timesteps: int) -> Tensor:
    """video_encoder.py:256-258: feat.reshape(B,T,N,C)[:, :, 0, :].mean(1)."""
    bt, n, c = feat.shape
    return feat.reshape(bsz, timesteps, n, c)[:, :, 0, :].mean(dim=1)


def encoder(sd, arch, video: Tensor) -> Tensor:
    """ViTFrameEncoder.forward (video_encoder.py:288-326): [B,T,3,H,W] -> [B,256] fp32."""
    if video.ndim == 4:
        video = video.unsqueeze(1)
    bsz, t = video.shape[:2]
    feat = vit_forward_features(sd, arch, video.reshape(bsz * t, *video.shape[2:]))
    pooled = cls_temporal_pool(feat, bsz, t)
    return F.linear(pooled, _t(sd, "encoder.proj.weight"), _t(sd, "encoder.proj.bias")).float()


def prefix_norm(emb: Tensor, ln_scale: Optional[float], in_weight: Optional[float]) -> Tensor:
    """core/engine.py:44-50."""
    if emb.dim() == 2:
        emb = emb.unsqueeze(1)
    if ln_scale is not None and ln_scale > 0:
        emb = F.layer_norm(emb, emb.shape[-1:]) * ln_scale
    if in_weight is not None and in_weight > 0:
        emb = emb * in_weight
    return emb


def mapper(sd, emb: Tensor, n_embd: int, prefix_len: int) -> Tensor:
    """text_decoder.py:249: mapper(video_emb).view(B, P, H) (Dropout is eval-identity).

    `emb` may be [B,256] (VideoCaptionModel.generate) or [B,1,256] (engine path);
    .view(B,P,H) flattens either the same way."""
    y = F.linear(emb, _t(sd, "decoder.mapper.0.weight"), _t(sd, "decoder.mapper.0.bias"))
    return y.reshape(emb.shape[0], prefix_len, n_embd)


# --------------------------------------------------------------------------- GPT-2

class KVCache:
    def __init__(self, n_layer: int):
        self.k: List[Optional[Tensor]] = [None] * n_layer
        self.v: List[Optional[Tensor]] = [None] * n_layer

    @property
    def length(self) -> int:
        return 0 if self.k[0] is None else self.k[0].shape[2]

    def reorder(self, idx: Tensor) -> None:
        for i in range(len(self.k)):
            self.k[i] = self.k[i].index_select(0, idx)
            self.v[i] = self.v[i].index_select(0, idx)


def _gelu_new(x: Tensor) -> Tensor:
    return 0.5 * x * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * torch.pow(x, 3.0))))


def gpt2_forward(sd, arch, inputs_embeds: Tensor, cache: KVCache) -> Tensor:
    """One GPT2LMHeadModel forward over S new positions; returns logits [B,S,V]."""
    p = "decoder.model.transformer."
    e, nh = arch.n_embd, arch.n_head
    hd = e // nh
    bsz, s, _ = inputs_embeds.shape
    past = cache.length
    pos = torch.arange(past, past + s)
    h = inputs_embeds + _t(sd, p + "wpe.weight")[pos].unsqueeze(0)
    causal = None
    if s > 1:
        causal = torch.ones(s, past + s, dtype=torch.bool).tril(diagonal=past)
    for i in range(arch.n_layer):
        b = f"{p}h.{i}."
        a = F.layer_norm(h, (e,), _t(sd, b + "ln_1.weight"), _t(sd, b + "ln_1.bias"), arch.ln_eps)
        qkv = a @ _t(sd, b + "attn.c_attn.weight") + _t(sd, b + "attn.c_attn.bias")
        q, k, v = qkv.split(e, dim=2)
        q = q.reshape(bsz, s, nh, hd).transpose(1, 2)
        k = k.reshape(bsz, s, nh, hd).transpose(1, 2)
        v = v.reshape(bsz, s, nh, hd).transpose(1, 2)
        if cache.k[i] is not None:
            k = torch.cat([cache.k[i], k], dim=2)
            v = torch.cat([cache.v[i], v], dim=2)
        cache.k[i], cache.v[i] = k, v
        att = F.scaled_dot_product_attention(q, k, v, attn_mask=causal)
        att = att.transpose(1, 2).reshape(bsz, s, e)
        h = h + (att @ _t(sd, b + "attn.c_proj.weight") + _t(sd, b + "attn.c_proj.bias"))
        m = F.layer_norm(h, (e,), _t(sd, b + "ln_2.weight"), _t(sd, b + "ln_2.bias"), arch.ln_eps)
        m = _gelu_new(m @ _t(sd, b + "mlp.c_fc.weight") + _t(sd, b + "mlp.c_fc.bias"))
        h = h + (m @ _t(sd, b + "mlp.c_proj.weight") + _t(sd, b + "mlp.c_proj.bias"))
    h = F.layer_norm(h, (e,), _t(sd, p + "ln_f.weight"), _t(sd, p + "ln_f.bias"), arch.ln_eps)
    return h @ _t(sd, "decoder.model.lm_head.weight").t()


def build_inputs(sd, arch, prefix: Tensor, prompt_ids: Sequence[int]) -> Tensor:
    """text_decoder.py:60-74: cat([prefix, wte(ids) broadcast to B], dim=1)."""
    ids = torch.tensor(list(prompt_ids), dtype=torch.long)
    base = _t(sd, "decoder.model.transformer.wte.weight")[ids].unsqueeze(0).expand(prefix.shape[0], -1, -1)
    return torch.cat([prefix, base], dim=1)


# --------------------------------------------------------------------------- logits processors

def apply_repetition_penalty(scores: Tensor, gen: Tensor, penalty: float) -> Tensor:
    """RepetitionPenaltyLogitsProcessor: gather, <0 ? *p : /p, scatter (duplicates idempotent)."""
    if penalty == 1.0 or gen.shape[1] == 0:
        return scores
    sc = torch.gather(scores, 1, gen)
    sc = torch.where(sc < 0, sc * penalty, sc / penalty)
    return scores.scatter(1, gen, sc)


def banned_ngram_tokens(seq: Sequence[int], n: int) -> List[int]:
    """NoRepeatNGramLogitsProcessor: tokens that would complete an n-gram already present."""
    L = len(seq)
    if n <= 0 or L + 1 < n:
        return []
    tail = tuple(seq[L - n + 1:]) if n > 1 else ()
    out = []
    for i in range(L - n + 1):
        if tuple(seq[i:i + n - 1]) == tail:
            out.append(seq[i + n - 1])
    return out


def process_logits(scores: Tensor, gen: Tensor, *, repetition_penalty: float, no_repeat_ngram_size: int,
                   min_new_tokens: int, eos_token_id: int) -> Tensor:
    scores = apply_repetition_penalty(scores, gen, repetition_penalty)
    if no_repeat_ngram_size and no_repeat_ngram_size > 0:
        scores = scores.clone()
        for r in range(scores.shape[0]):
            for tok in banned_ngram_tokens(gen[r].tolist(), no_repeat_ngram_size):
                scores[r, tok] = -float("inf")
    if gen.shape[1] < min_new_tokens:
        scores = scores.clone()
        scores[:, eos_token_id] = -float("inf")
    return scores


# --------------------------------------------------------------------------- decode loops

def generate_greedy(sd, arch, inputs_embeds: Tensor, *, max_new_tokens: int = 24, min_new_tokens: int = 8,
                    repetition_penalty: float = 1.1, no_repeat_ngram_size: int = 3,
                    eos_token_id: Optional[int] = None, pad_token_id: Optional[int] = None,
                    return_logits: bool = False) -> Tuple[Tensor, List[Tensor]]:
    """HF generate(num_beams=1, do_sample=False) from inputs_embeds; returns only new tokens."""
    eos = arch.eos_token_id if eos_token_id is None else eos_token_id
    pad = eos if pad_token_id is None else pad_token_id
    bsz = inputs_embeds.shape[0]
    cache = KVCache(arch.n_layer)
    gen = torch.zeros(bsz, 0, dtype=torch.long)
    unfinished = torch.ones(bsz, dtype=torch.bool)
    wte = _t(sd, "decoder.model.transformer.wte.weight")
    x = inputs_embeds
    raw_logits = []
    for _ in range(max_new_tokens):
        logits = gpt2_forward(sd, arch, x, cache)[:, -1, :].float()
        if return_logits:
            raw_logits.append(logits.clone())
        scores = process_logits(logits, gen, repetition_penalty=repetition_penalty,
                                no_repeat_ngram_size=no_repeat_ngram_size,
                                min_new_tokens=min_new_tokens, eos_token_id=eos)
        nxt = torch.argmax(scores, dim=-1)
        nxt = torch.where(unfinished, nxt, torch.full_like(nxt, pad))
        gen = torch.cat([gen, nxt[:, None]], dim=1)
        unfinished = unfinished & (nxt != eos)
        if not bool(unfinished.any()):
            break
        x = wte[nxt].unsqueeze(1)
    return gen, raw_logits


def generate_raw_greedy(sd, arch, inputs_embeds: Tensor, *, max_new_tokens: int = 24,
                        eos_token_id: Optional[int] = None) -> List[List[int]]:
    """benchmark_baseline.run_decoder_steps (:160-240): argmax, no processors, tokens up to and
    including EOS per row, break when all finished."""
    eos = arch.eos_token_id if eos_token_id is None else eos_token_id
    bsz = inputs_embeds.shape[0]
    cache = KVCache(arch.n_layer)
    wte = _t(sd, "decoder.model.transformer.wte.weight")
    out: List[List[int]] = [[] for _ in range(bsz)]
    finished = torch.zeros(bsz, dtype=torch.bool)
    x = inputs_embeds
    for _ in range(max_new_tokens):
        logits = gpt2_forward(sd, arch, x, cache)[:, -1, :]
        nxt = torch.argmax(logits, dim=-1)
        nxt = torch.where(finished, torch.full_like(nxt, eos), nxt)
        for i, tok in enumerate(nxt.tolist()):
            if not finished[i]:
                out[i].append(tok)
                if tok == eos:
                    finished[i] = True
        if bool(finished.all()):
            break
        x = wte[nxt].unsqueeze(1)
    return out


def generate_beam(sd, arch, inputs_embeds: Tensor, *, num_beams: int, max_new_tokens: int, min_new_tokens: int = 8,
                  repetition_penalty: float = 1.1, no_repeat_ngram_size: int = 3, length_penalty: float = 1.0,
                  eos_token_id: Optional[int] = None, trace: Optional[dict] = None) -> List[List[int]]:
    """HF GenerationMixin._beam_search (transformers 5.15.0 generation/utils.py, as
    text_decoder.py:131-144 reaches it with inputs_embeds: prompt length 0, early_stopping False)
    restated on the CPU: log_softmax -> processors -> + running beam scores -> top-2k over
    beams x vocab -> running / finished updates -> cache reorder; stop when no batch can improve
    or every candidate hit EOS / max length.  Returns each sequence's best finished hypothesis
    (the first max(length) tokens, EOS-padded) - pinned to the reference's beam3 / beam4 goldens
    and to transformers' own EOS-rich searches (tests/golden/beam_eos, tests/test_cpu_oracle.py).

    `trace`, when given, is a dict this fills (the ids returned do not change):
      lengths [B]            generated length of each best hypothesis
      steps                  number of select steps executed; stopped_early = steps < max_new_tokens
      sat_step [B]           step at which the sequence stopped being able to improve (None: never)
      events [B]             counters over the steps the sequence was still improvable: `did` (EOS in
                             the first nb of the top-2nb), `late` (EOS in ranks nb..2nb-1), `evict`
                             (a finished hypothesis pushed out of the best nb by a better one),
                             `best_replaced` (a newer hypothesis took the best place from an older)
      margins [B][step]      the smallest gap behind any decision of that step, taken while the
                             sequence is improvable, entries at or below -1e8 ignored: consecutive
                             gaps of the top 2nb+1 of lp + running score (the last is the membership
                             gap), consecutive gaps of the top nb+1 merged finished scores, and
                             |best running - worst finished| where a finished hypothesis exists."""
    eos = arch.eos_token_id if eos_token_id is None else eos_token_id
    B, nb = inputs_embeds.shape[0], num_beams
    V, L, K = arch.vocab, max_new_tokens, 2 * num_beams
    cache = KVCache(arch.n_layer)
    wte = _t(sd, "decoder.model.transformer.wte.weight")
    logits = gpt2_forward(sd, arch, inputs_embeds, cache)[:, -1, :].float().repeat_interleave(nb, dim=0)
    cache.reorder(torch.arange(B * nb) // nb)
    run_seq = torch.full((B, nb, L), eos, dtype=torch.long)
    run_score = torch.zeros(B, nb)
    run_score[:, 1:] = -1e9
    run_bidx = torch.full((B, nb, L), -1, dtype=torch.long)
    seqs, beam_idx = run_seq.clone(), run_bidx.clone()
    beam_score = torch.full((B, nb), -1e9)
    fin = torch.zeros(B, nb, dtype=torch.bool)
    unsat = torch.ones(B, dtype=torch.bool)
    take = lambda t, i: torch.stack([t[b][i[b]] for b in range(B)])  # noqa: E731
    if trace is not None:
        trace.update(sat_step=[None] * B, margins=[[] for _ in range(B)], steps=0,
                     events=[dict(did=0, late=0, evict=0, best_replaced=0) for _ in range(B)])

    def gaps(v):   # consecutive gaps of a descending list, pairs touching a masked entry dropped
        return [float(a - b) for a, b in zip(v[:-1], v[1:]) if b > -1.0e8]
    for cur in range(L):
        lp = torch.log_softmax(logits, dim=-1)
        lp = process_logits(lp, run_seq[:, :, :cur].reshape(B * nb, cur), repetition_penalty=repetition_penalty,
                            no_repeat_ngram_size=no_repeat_ngram_size, min_new_tokens=min_new_tokens,
                            eos_token_id=eos)
        lp = (lp.view(B, nb, V) + run_score[:, :, None]).reshape(B, nb * V)
        top_lp, top_i = torch.topk(lp, K)
        src, tok = top_i // V, top_i % V
        t_seq, t_bidx = take(run_seq, src), take(run_bidx, src)
        t_seq[:, :, cur] = tok
        t_bidx[:, :, cur] = src + torch.arange(B)[:, None] * nb
        hits = (tok == eos) | (cur + 1 >= L)
        run_lp = top_lp + hits.float() * -1.0e9
        nxt = torch.topk(run_lp, nb)[1]
        run_seq, run_score, run_bidx = take(t_seq, nxt), take(run_lp, nxt), take(t_bidx, nxt)
        did = hits & (torch.arange(K) < nb)[None, :]
        sc = top_lp / ((cur + 1) ** length_penalty)
        sc = sc + (~unsat)[:, None].float() * -1.0e9 + (~did).float() * -1.0e9
        m_sc, sel = torch.topk(torch.cat([beam_score, sc], 1), nb)
        if trace is not None:
            was, old_fin = unsat.clone(), fin.clone()
            mg = [gaps(torch.topk(lp[b], K + 1)[0].tolist()) +
                  gaps(torch.topk(torch.cat([beam_score[b], sc[b]]), nb + 1)[0].tolist()) for b in range(B)]
        seqs, beam_idx = take(torch.cat([seqs, t_seq], 1), sel), take(torch.cat([beam_idx, t_bidx], 1), sel)
        fin, beam_score = take(torch.cat([fin, did], 1), sel), m_sc
        cache.reorder(run_bidx[:, :, cur].reshape(-1))
        best_running = run_score[:, 0] / ((cur + 1) ** length_penalty)
        worst = torch.where(fin, beam_score.min(dim=1, keepdim=True)[0], torch.full_like(beam_score, -1.0e9))
        unsat = unsat & (best_running[:, None] > worst).any(dim=1)
        if trace is not None:
            trace["steps"] = cur + 1
            for b in range(B):
                if not bool(was[b]):
                    continue
                ev = trace["events"][b]
                ev["did"] += int(did[b].sum())
                ev["late"] += int(((tok[b] == eos) & (torch.arange(K) >= nb)).sum())
                ev["evict"] += int(old_fin[b].sum()) - int((fin[b] & (sel[b] < nb)).sum())
                ev["best_replaced"] += int(bool(old_fin[b].any()) and int(sel[b, 0]) >= nb)
                if bool(fin[b].any()) and float(beam_score[b].min()) > -1.0e8:
                    mg[b].append(abs(float(best_running[b]) - float(beam_score[b].min())))
                trace["margins"][b].append(min(mg[b]) if mg[b] else float("inf"))
                if not bool(unsat[b]):
                    trace["sat_step"][b] = cur
        if not bool(unsat.any()) or bool(hits.all()):
            break
        logits = gpt2_forward(sd, arch, wte[run_seq[:, :, cur].reshape(-1)].unsqueeze(1), cache)[:, -1, :].float()
    lens = (beam_idx[:, 0, :] != -1).sum(dim=1)
    n = int(lens.max())
    if trace is not None:
        trace.update(lengths=lens.tolist(), stopped_early=trace["steps"] < L)
    return seqs[:, 0, :n].tolist()


def hypothesis_scores(sd, arch, inputs_embeds: Tensor, seqs: Sequence[Sequence[int]], *, min_new_tokens: int = 8,
                      repetition_penalty: float = 1.1, no_repeat_ngram_size: int = 3, length_penalty: float = 1.0,
                      eos_token_id: Optional[int] = None) -> List[float]:
    """The score HF _beam_search gives a finished hypothesis (transformers 5.15.0
    generation/utils.py:3182 `_update_finished_beams`: the running sum of processed log-probs /
    generated length ** length_penalty; generate_beam above accumulates exactly that), computed
    for given token sequences teacher-forced from inputs_embeds (row i continues row i)."""
    eos = arch.eos_token_id if eos_token_id is None else eos_token_id
    seqs = [list(map(int, r)) for r in seqs]
    lens = [r.index(eos) + 1 if eos in r else len(r) for r in seqs]
    L = max(lens)
    tok = torch.full((len(seqs), L), eos, dtype=torch.long)
    for i, r in enumerate(seqs):
        tok[i, :lens[i]] = torch.tensor(r[:lens[i]])
    cache = KVCache(arch.n_layer)
    wte = _t(sd, "decoder.model.transformer.wte.weight")
    x = inputs_embeds
    total = torch.zeros(len(seqs), dtype=torch.float64)
    for s in range(L):
        lp = torch.log_softmax(gpt2_forward(sd, arch, x, cache)[:, -1, :].float(), dim=-1)
        lp = process_logits(lp, tok[:, :s], repetition_penalty=repetition_penalty,
                            no_repeat_ngram_size=no_repeat_ngram_size, min_new_tokens=min_new_tokens,
                            eos_token_id=eos)
        live = torch.tensor([s < n for n in lens])
        total += torch.where(live, lp.gather(1, tok[:, s:s + 1])[:, 0].double(), torch.zeros_like(total))
        x = wte[tok[:, s]].unsqueeze(1)
    return (total / torch.tensor(lens, dtype=torch.float64) ** length_penalty).tolist()


def caption_ids(sd, vit_arch, gpt_arch, video: Tensor, prompt_ids: Sequence[int], *, ln_scale: float = 0.6,
                in_weight: float = 0.4, prefix_len: int = 4, mode: str = "hf_greedy", **gen_kw):
    """Engine path A1 (core/engine.py:39-64) up to token ids (before detokenize/clean_text)."""
    emb = encoder(sd, vit_arch, video)
    emb = prefix_norm(emb, ln_scale, in_weight)
    pre = mapper(sd, emb, gpt_arch.n_embd, prefix_len)
    x = build_inputs(sd, gpt_arch, pre, prompt_ids)
    if mode == "raw_greedy":
        return generate_raw_greedy(sd, gpt_arch, x, **gen_kw)
    if gen_kw.get("num_beams", 1) > 1:
        return torch.tensor(generate_beam(sd, gpt_arch, x, **gen_kw))
    gen_kw.pop("num_beams", None)
    ids, _ = generate_greedy(sd, gpt_arch, x, **gen_kw)
    return ids


# ----------------------------------------------------------------------------- sampling (HF _sample)
# HF generate with do_sample: the processors above, then TemperatureLogitsWarper -> TopKLogitsWarper ->
# TopPLogitsWarper (transformers generation/logits_process.py), then one multinomial draw per row.
# The warpers are restated here (tests/test_cpu_sampling_cases.py pins them bit for bit to HF's own
# classes); the draw is the device's documented one (csrc/sample.hip): a Philox4x32-10 uniform and an
# inverse CDF over the kept tokens in ascending order.

def warp_scores(scores: Tensor, temperature: float, top_k: int, top_p: float) -> Tensor:
    """scores [B, V] f32 (processed) -> warped scores [B, V] f32, -inf where removed.  The top-p warper
    is left out at top_p == 1.0, as HF's generate leaves it out; min_tokens_to_keep is 1.
    Where the top-p cut falls inside a group of equal scores, which of them go is the choice of
    torch.sort (HF's call, not a stable sort); the device drops those of lowest vocabulary index."""
    s = scores / temperature
    k = min(int(top_k), s.shape[-1])
    s = s.masked_fill(s < torch.topk(s, k)[0][..., -1, None], -float("inf"))   # ties at the k-th value stay
    if top_p < 1.0:
        srt, idx = torch.sort(s, descending=False)
        remove = srt.softmax(dim=-1).cumsum(dim=-1) <= (1 - top_p)
        remove[..., -1:] = False                                    # the largest is always kept
        s = s.masked_fill(remove.scatter(-1, idx, remove), -float("inf"))
    return s


_PHILOX_M0, _PHILOX_M1, _PHILOX_W0, _PHILOX_W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
_M32 = 0xFFFFFFFF


def philox4x32_10(counter4: Sequence[int], key2: Sequence[int]) -> Tuple[int, int, int, int]:
    """Philox4x32 with 10 rounds (Salmon et al., Random123) on 32-bit words."""
    c0, c1, c2, c3 = (int(c) & _M32 for c in counter4)
    k0, k1 = (int(k) & _M32 for k in key2)
    for _ in range(10):
        p0, p1 = _PHILOX_M0 * c0, _PHILOX_M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & _M32, (p0 >> 32) ^ c3 ^ k1, p0 & _M32
        k0, k1 = (k0 + _PHILOX_W0) & _M32, (k1 + _PHILOX_W1) & _M32
    return c0, c1, c2, c3


def sample_uniform(seed: int, row: int, step: int) -> float:
    """The uniform of (seed, row, step): counter (step, row, 0, 0), key (seed low word, seed high
    word), the top 24 bits of the first output word -> u in [0, 1), a multiple of 2^-24."""
    w0 = philox4x32_10((step, row, 0, 0), (seed & _M32, (seed >> 32) & _M32))[0]
    return (w0 >> 8) / float(1 << 24)


def _ascending_mass(row: Tensor) -> Tuple[Tensor, Tensor]:
    """The finite entries of a row in ascending order (ties by vocabulary index) -> (their indices,
    cumulative exp(s - max) / total in float64)."""
    row = row.double()
    kept = torch.nonzero(torch.isfinite(row)).flatten()
    vals, order = torch.sort(row[kept], stable=True)
    cum = torch.exp(vals - vals[-1]).cumsum(0)
    return kept[order], cum / cum[-1]


def draw(warped_row: Tensor, u: float) -> Tuple[int, float]:
    """Inverse-CDF draw from softmax(warped_row): the kept (finite) tokens are walked ascending by
    value, ties by vocabulary index, and the token is the first whose cumulative mass exceeds
    u * total.  -> (token, margin); margin = min_j |u - C_j / total|, how far u is from a different draw."""
    idx, cdf = _ascending_mass(warped_row)
    j = min(int(torch.searchsorted(cdf, torch.tensor(u, dtype=torch.float64), right=True)), len(idx) - 1)
    return int(idx[j]), float((cdf - u).abs().min())


def top_p_margin(processed_row: Tensor, temperature: float, top_k: int, top_p: float) -> float:
    """How far the top-p cut of one processed f32 row is from keeping a different set: the smallest
    |cumsum_j - (1 - top_p)| of the ascending cumulative softmax (float64) over the top-k survivors.
    The last cumsum (1.0, the largest token) is left out: that token is kept whatever it compares to,
    and counting it would put every row of a tiny top_p within top_p of a cut that cannot happen.
    inf at top_p == 1 (no top-p warper runs) and where one score survives top-k."""
    if top_p >= 1.0:
        return float("inf")
    s = warp_scores(processed_row.float()[None], temperature, top_k, 1.0)[0]
    _, cdf = _ascending_mass(s)
    return float((cdf[:-1] - (1.0 - top_p)).abs().min()) if len(cdf) > 1 else float("inf")


# ----------------------------------------------------------------------------- MXFP8 (configs[4])
# The reference has no fp8 path; BASELINE.json configs[4] asks for an fp8 MFMA path for the ViT
# GEMMs.  The format restated here is the one libvcap_hip.so computes in (include/vcap.h
# VCAP_DT_MXFP8): OCP MX (Microscaling Formats v1.0) MXFP8-E4M3 - blocks of 32 consecutive
# K elements sharing one E8M0 scale - with the shared exponent floor(log2(amax)) - 7 (the spec's
# recipe with emax 7 instead of 8, so no element saturates), elements rounded to nearest-even.

def mx_scale_index(rows: int, K: int) -> np.ndarray:
    """Byte offset of scale (row, 32-block) in the GEMM staging layout -> int64 [rows, K/32]."""
    r = np.arange(rows)[:, None]
    k = (np.arange(K // 32) * 32)[None, :]
    groups = (rows + 255) // 256
    return (((k // 128) * groups + r // 256) * 4 + (k % 128) // 32) * 256 + (r % 16) * 16 + (r % 256) // 16


def mx_scale_bytes(rows: int, K: int) -> int:
    return (K // 128) * ((rows + 255) // 256) * 1024


def mx_quantize(x: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """f32 [rows, K] -> (e4m3 bytes [rows, K] uint8, E8M0 scales [rows, K/32] uint8).
    Non-finite input follows include/vcap.h: a NaN takes no part in the block max (np.fmax, the kernels'
    fmaxf) and is stored as an e4m3 NaN; a block holding +-inf has scale byte 248.  The byte of an inf
    element is the one place this function and the device may differ (here 0x7F / 0xFF, torch's cast; the
    header leaves it open between that and +-448)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    rows, K = x.shape
    blk = x.reshape(rows, K // 32, 32)
    amax = np.fmax.reduce(np.abs(blk), axis=-1).astype(np.float32)
    sb = np.maximum(((amax.view(np.uint32) >> 23) & 0xFF).astype(np.int32) - 7, 0)
    inv = ((254 - sb).astype(np.uint32) << 23).view(np.float32)
    q = torch.from_numpy(blk * inv[..., None]).to(torch.float8_e4m3fn).view(torch.uint8).numpy()
    return q.reshape(rows, K), sb.astype(np.uint8)


def mx_dequantize(q: np.ndarray, sb: np.ndarray) -> np.ndarray:
    rows, K = q.shape
    v = torch.from_numpy(np.ascontiguousarray(q)).view(torch.float8_e4m3fn).float().numpy().reshape(rows, K // 32, 32)
    return (v * np.exp2(sb.astype(np.float32) - 127.0)[..., None]).reshape(rows, K)


def mx_pack_scales(sb: np.ndarray) -> np.ndarray:
    """[rows, K/32] scales -> the flat staging-layout array (vcap_mx_scale_bytes long)."""
    rows, nb = sb.shape
    out = np.zeros(mx_scale_bytes(rows, nb * 32), np.uint8)
    out[mx_scale_index(rows, nb * 32)] = sb
    return out


def mx_unpack_scales(flat: np.ndarray, rows: int, K: int) -> np.ndarray:
    return np.asarray(flat)[mx_scale_index(rows, K)]


# ----------------------------------------------------------------------------- frame preprocessing
# Reference: core/preprocessing/frame_loader.py:34-45 - torchvision Resize((S, S)) on a PIL image
# (= PIL Image.resize(BILINEAR), Pillow 12.2 in this image) -> ToTensor (/255 in f32) ->
# Normalize(mean, std) (f32 sub, div).  Restated here from Pillow's Resample.c algorithm
# (precompute_coeffs / normalize_coeffs_8bpc / ImagingResample{Horizontal,Vertical}_8bpc): separable
# triangle filter widened by the downscale factor, double-precision weights normalised per output
# pixel, converted to 22-bit fixed point, int32 accumulation from a 2^21 rounding bias, clamp to
# [0, 255] after each pass (horizontal pass first, over the source rows the vertical pass uses).

_PREC = 22


def _pil_coeffs(in_size: int, out_size: int):
    scale = in_size / out_size
    fscale = max(scale, 1.0)
    support = 1.0 * fscale
    ksize = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((out_size, 2), np.int64)
    kk = np.zeros((out_size, ksize), np.int64)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        ss = 1.0 / fscale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = []
        for x in range(xmax):
            t = abs((x + xmin - center + 0.5) * ss)
            w.append(1.0 - t if t < 1.0 else 0.0)
        ww = sum(w) if w else 0.0  # left-to-right double sum, as the C loop
        acc = 0.0
        for v in w:
            acc += v
        ww = acc
        for x in range(xmax):
            v = w[x] / ww if ww != 0.0 else w[x]
            kk[xx, x] = int(-0.5 + v * (1 << _PREC)) if v < 0 else int(0.5 + v * (1 << _PREC))
        bounds[xx] = (xmin, xmax)
    return bounds, kk


def _pil_pass(img: np.ndarray, bounds, kk, axis: int) -> np.ndarray:
    """One 8-bpc resample pass along `axis` (0 rows, 1 columns) of an [H, W, C] uint8 image."""
    src = np.moveaxis(img.astype(np.int64), axis, 0)
    out = np.empty((len(bounds),) + src.shape[1:], np.uint8)
    for i, (lo, n) in enumerate(bounds):
        acc = np.full(src.shape[1:], 1 << (_PREC - 1), np.int64)
        for t in range(n):
            acc += src[lo + t] * kk[i, t]
        out[i] = np.clip(acc >> _PREC, 0, 255)
    return np.moveaxis(out, 0, axis)


def pil_resize_bilinear(img: np.ndarray, out_w: int, out_h: int) -> np.ndarray:
    """[H, W, 3] uint8 -> [out_h, out_w, 3] uint8, bit-identical to PIL Image.resize(BILINEAR)."""
    h, w = img.shape[:2]
    if (h, w) == (out_h, out_w):
        return img.copy()
    bh, kh = _pil_coeffs(w, out_w)
    bv, kv = _pil_coeffs(h, out_h)
    if w != out_w:
        y0, y1 = int(bv[0, 0]), int(bv[-1, 0] + bv[-1, 1])
        img = _pil_pass(img[y0:y1], bh, kh, axis=1)
        bv = bv.copy()
        bv[:, 0] -= y0
    if h != out_h:
        img = _pil_pass(img, bv, kv, axis=0)
    return img


def frames_to_tensor(imgs_u8: np.ndarray, size: int) -> np.ndarray:
    """[T, H, W, 3] uint8 frames -> [T, 3, size, size] f32 (Resize -> ToTensor -> Normalize)."""
    mean = np.array([0.485, 0.456, 0.406], np.float32)[:, None, None]
    std = np.array([0.229, 0.224, 0.225], np.float32)[:, None, None]
    out = []
    for im in imgs_u8:
        r = pil_resize_bilinear(im, size, size).transpose(2, 0, 1).astype(np.float32) / np.float32(255.0)
        out.append((r - mean) / std)
    return np.stack(out)
