"""Shared by test_cpu_sampling_cases.py and test_gpu_sampling_sweep.py: the cases of the sampling sweep
(vocab axis, warper-parameter axis, ties at the k-th value, a row with no finite score), their
synthetic models and prefixes, and the fp64 oracle's own free-running sampled path.

The models are decoder_shapes' n_embd 128 decoder at other vocab sizes (bos = eos = V - 1), prefix 4,
prompt [bos].  Every case decodes 8 tokens with EOS banned for the first two, no-repeat 2-grams and
repetition penalty 1.3, so that bans and penalties occur within the 8 steps.

What a GPU run is compared with is computed from its own raw logits and its own ids (oracle
process_logits -> warp_scores -> sample_uniform -> draw), so no GEMM error enters; a (row, step) pair
binds unless the oracle's own margin says a rounding difference could change the result:
  * top_p_margin < MARGIN: the ascending cumulative softmax passes within MARGIN of 1 - top_p, so a
    different summation order may cut the support elsewhere;
  * draw margin < MARGIN: u lies within MARGIN of a boundary of the inverse CDF.
MARGIN = 1e-5 is a few hundred f32 ulps of a cumulative sum of at most 256 terms of size <= 1: it
covers expf and summation-order differences with room to spare.  It is argued, not measured."""
from __future__ import annotations

from dataclasses import dataclass
from functools import lru_cache

import numpy as np
import torch

import decoder_shapes as S
from oracle import vcap_oracle as O

E = 128
MAX_NEW, MIN_NEW, NGRAM, REP = 8, 2, 2, 1.3
SEEDS = (7, (3 << 32) + 11)      # the second keeps the high key word live
MARGIN = 1e-5
SKIP_CAP = 0.05                  # share of a case's live (row, step) pairs the margins may skip
KCAND = 256                      # csrc/sample.hip kCand: survivors the kernel can hold
WARPED_RTOL, WARPED_ATOL = 1e-5, 1e-4   # test_gpu_surface.py's bar on the warped values


@dataclass(frozen=True)
class Case:
    V: int
    T: float
    k: int
    p: float
    B: int
    prec: str = "fp32"

    @property
    def id(self) -> str:
        return f"V{self.V}-T{self.T:g}-k{self.k}-p{self.p:g}-B{self.B}-{self.prec}"


# vocab axis: <1> partial, <1> full, <8> nearly all padding, <8> full, <16>, <32>, <50>, <50> full (the
# ABI's bound); V = 8193 and 51200 again in bf16.  The raw logits of these cases are checked too.
VOCABS = (1000, 1024, 1025, 8192, 8193, 16385, 32769, 51200)
INSTANCE = {1000: 1, 1024: 1, 1025: 8, 8192: 8, 8193: 16, 16385: 32, 32769: 50, 51200: 50, 64: 1}
VOCAB_CASES = [Case(v, 0.9, 50, 0.9, 5) for v in VOCABS] + [Case(v, 0.9, 50, 0.9, 5, "bf16") for v in (8193, 51200)]
# parameter axis at V = 8193 (<16>); its first row is the vocab axis' V = 8193 case and runs at B = 1 too
PARAMS = [(0.9, 50, 0.9), (0.7, 50, 1.0), (0.7, 1, 1.0), (0.05, 50, 0.9), (5.0, 128, 0.999999), (1.3, 128, 1e-6),
          (0.8, 20, 0.5)]
PARAM_CASES = [Case(8193, t, k, p, 5) for t, k, p in PARAMS[1:]] + [Case(8193, *PARAMS[0], 1)]
FULL_SUPPORT = Case(64, 0.9, 128, 1.0, 3)       # top_k >= V: the whole unbanned vocabulary is the support
CASES = VOCAB_CASES + PARAM_CASES + [FULL_SUPPORT]

TIE_V, TIE_B, TIE_T, TIE_K = 1025, 2, 0.9, 50
TIES_INSIDE = Case(TIE_V, TIE_T, TIE_K, 1.0, TIE_B)
# 16 (row, step) pairs: one skipped pair is over the cap, so each tie test runs the seed whose oracle
# path skips none (test_cpu_sampling_cases.py::test_tie_paths_skip_nothing)
TIE_SEEDS = {"inside": SEEDS[0], "over": SEEDS[0]}
N_TIES_INSIDE, N_TIES_OVER = 12, 300
NAN_CASE = Case(1000, 0.9, 50, 0.9, 3)


def arch(c: Case):
    return S.arch(E, c.V)


def prefix(c: Case) -> torch.Tensor:
    """0.1 * randn [B, 4, E] f32 from a fixed CPU generator.  With these seeds the oracle's own sampled
    path skips at most one (row, step) pair of a case (test_cpu_sampling_cases.py prints every case's
    share and asserts it is at most SKIP_CAP / 2)."""
    g = torch.Generator().manual_seed(7919 * c.V + c.B)
    return 0.1 * torch.randn(c.B, S.PREFIX_LEN, E, generator=g, dtype=torch.float32)


def prompt(c: Case):
    return [c.V - 1]


def process(c: Case, raw: torch.Tensor, hist: torch.Tensor) -> torch.Tensor:
    """oracle.process_logits under the sweep's settings: raw [B, V] f32, hist [B, step] int64."""
    return O.process_logits(raw, hist, repetition_penalty=REP, no_repeat_ngram_size=NGRAM, min_new_tokens=MIN_NEW,
                            eos_token_id=c.V - 1)


def kcand_support(ref_row: torch.Tensor) -> torch.Tensor:
    """The device's documented support for one warped reference row (top_p == 1): HF's own when it has
    at most KCAND tokens; otherwise every score strictly above the tied threshold value and then the
    tied tokens of lowest vocabulary index, KCAND in all (include/vcap.h, vcap_gpt2_sample)."""
    fin = torch.isfinite(ref_row)
    if int(fin.sum()) <= KCAND:
        return fin
    thr = ref_row[fin].min()
    above = fin & (ref_row > thr)
    tied = torch.nonzero(fin & (ref_row == thr)).flatten()
    keep = above.clone()
    keep[tied[:KCAND - int(above.sum())]] = True
    return keep


def with_duplicates(sd, src: int, dst) -> dict:
    """The state dict with wte row `src` copied over the rows `dst`: the lm_head is tied, so those
    columns' logits are one dot product."""
    w = np.array(sd[S.WTE], copy=True)
    w[np.asarray(dst)] = w[src]
    out = dict(sd)
    out[S.WTE] = w
    out["decoder.model.lm_head.weight"] = w
    return out


@lru_cache(maxsize=None)
def _step0_order(c: Case):
    """Vocabulary indices of row 0 by descending step-0 logit of the untouched model (fp64 oracle), EOS
    left out.  Step 0 reads wte only at the prompt's token V - 1, so duplicating other rows leaves the
    step-0 hidden state and every untouched column's logit as they are."""
    ar, sd = arch(c), S.sd64(E, vocab=c.V)
    with torch.no_grad():
        lg = O.gpt2_forward(sd, ar, O.build_inputs(sd, ar, prefix(c).double(), prompt(c)), O.KVCache(ar.n_layer))
    order = torch.argsort(lg[0, -1], descending=True).tolist()
    return [i for i in order if i != c.V - 1]


def ties_inside_rows():
    """(src, dst): the token of rank 45 at row 0's step 0 and 11 low-ranked tokens that take its row.
    44 scores stay strictly above the 12 equal ones, which then hold ranks 45 .. 56: across k = 50.
    (The row is copied unscaled: a row picked at the rank that is wanted needs no scale.)"""
    order = _step0_order(TIES_INSIDE)
    return order[TIE_K - 6], sorted(order[600:600 + N_TIES_INSIDE - 1])


def ties_over_rows():
    """(src, dst): row 0's step-0 argmax and 299 rows spread over the vocabulary (every third index) that
    take its row: 300 scores tie at the top, more than KCAND."""
    src = _step0_order(TIES_INSIDE)[0]
    dst = [i for i in range(1, TIE_V - 1, 3) if i != src][:N_TIES_OVER - 1]
    return src, dst


def tied_rows(ties: str):
    return ties_inside_rows() if ties == "inside" else ties_over_rows()


@lru_cache(maxsize=None)
def oracle_path(c: Case, seed: int, ties: str = ""):
    """The fp64 oracle's own free-running sampled path of a case (forward in float64, processors and
    warpers on the f32 cast, the device's uniforms) -> dict of ids [B, steps], live [B, steps] (the row
    had not finished before the step), top-p and draw margins [B, steps], the number of n-gram bans.
    `ties` "inside" / "over": the model with the duplicated wte rows of that tie test, drawing from the
    device's documented support (kcand_support)."""
    ar, sd = arch(c), S.sd64(E, vocab=c.V)
    if ties:
        src, dst = tied_rows(ties)
        w = sd[S.WTE].clone()
        w[dst] = w[src].clone()
        sd = {**sd, S.WTE: w, "decoder.model.lm_head.weight": w}
    eos, B = c.V - 1, c.B
    cache = O.KVCache(ar.n_layer)
    x = O.build_inputs(sd, ar, prefix(c).double(), prompt(c))
    gen = torch.zeros(B, 0, dtype=torch.long)
    finished = torch.zeros(B, dtype=torch.bool)
    live = np.zeros((B, MAX_NEW), bool)
    tpm, drm = np.full((B, MAX_NEW), np.inf), np.full((B, MAX_NEW), np.inf)
    bans = 0
    with torch.no_grad():
        for step in range(MAX_NEW):
            proc = process(c, O.gpt2_forward(sd, ar, x, cache)[:, -1, :].float(), gen)
            warped = O.warp_scores(proc, c.T, c.k, c.p)
            if ties:
                warped = torch.stack([w.masked_fill(~kcand_support(w), -float("inf")) for w in warped])
            nxt = torch.full((B,), eos, dtype=torch.long)
            for r in range(B):
                if finished[r]:
                    continue
                live[r, step] = True
                bans += len(O.banned_ngram_tokens(gen[r].tolist(), NGRAM))
                tpm[r, step] = O.top_p_margin(proc[r], c.T, c.k, c.p)
                nxt[r], drm[r, step] = O.draw(warped[r], O.sample_uniform(seed, r, step))
            gen = torch.cat([gen, nxt[:, None]], dim=1)
            finished = finished | (nxt == eos)
            x = sd[S.WTE][nxt].unsqueeze(1)
    return {"ids": gen.numpy(), "live": live, "top_p_margin": tpm, "draw_margin": drm, "bans": bans}


def skipped_share(live, top_p_margin, draw_margin) -> float:
    """The share of live (row, step) pairs that either margin leaves unchecked."""
    skip = live & ((top_p_margin < MARGIN) | (draw_margin < MARGIN))
    return float(skip.sum()) / max(int(live.sum()), 1)
