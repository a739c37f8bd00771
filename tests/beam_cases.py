"""Shared by test_cpu_beam_cases.py, test_cpu_oracle.py and test_gpu_beam_sweep.py: the EOS-rich beam
searches (every beam width 2..8, three length penalties, processors on and off, a two-chunk vocabulary,
a context that crosses 64), their fp64-forward oracle runs, and the rule that says on which rows a
device search must reproduce the oracle token for token.

The decoders are the synthetic sweep decoders of decoder_shapes.py (2 layers, 128 positions, vocab 1000)
and the same weights at vocab 2053 (two candidate chunks, the last 5 columns wide).  EOS is a parameter
of the search, not of the weights: each case names as EOS a token the EOS-free beam path of its rows
emits early, so hypotheses finish, get evicted and satisfy sequences long before max_new_tokens.

A row is *certain* when every decision margin the oracle records for it (oracle.generate_beam's `trace`)
exceeds GAP(E, t) at its step t.  Rows are searched one seed at a time (sequences are independent in HF's
search) and stacked into batches; the few rows listed as uncertain only fill a batch to its size."""
from __future__ import annotations

from collections import namedtuple
from functools import lru_cache

import torch

import decoder_shapes as S
from oracle import vcap_oracle as O
from vcap import weights
from vcap.configs import GPT2Arch

# fp32 max |gpu - fp64| logit error of the decoder width sweep (greedy path, 24 steps, all B; DESIGN.md
# "Decoder widths")
E_LOGIT = {128: 3.4e-7, 256: 6.6e-7, 384: 1.0e-6}
# 2 scores compared x 2.2 (a log-prob is a logit minus a normaliser, each within e_logit, times at most
# the 1.1 repetition penalty) x 3 (the safety factor decoder_shapes.bf16_tolerance uses); the (t + 1)
# summed tokens of a running score enter GAP separately.  Dividing by (t + 1) ** length_penalty only
# shrinks an error for penalties >= 0, so the same bound serves the merged finished scores.
GAP_FACTOR = 2 * 2.2 * 3


def gap(E: int, t: int) -> float:
    return GAP_FACTOR * (t + 1) * E_LOGIT[E]


Case = namedtuple("Case", "name E V nb L min_new ngram rep lpen prompt_len eos seeds uncertain")

# Row seeds come from a scan of seeds 0..80 (0..300 at nb = 8, 0..150 for the long prompt), one sequence
# per search, keeping rows whose margins clear GAP and whose events differ; eos is the most common token
# of steps 2..L/2 of the first 8 seeds' EOS-free beam paths (2052 where the case is about the 5-column
# chunk).  One row each of nb3_b5 (15), nb5_lp0 (21), nb7 (14), v2053_early (14), long_s64 (23) and
# e256_nb4 (66) was picked because its result would change if an EOS in ranks nb..2nb-1 were admitted as
# finished (a copy of the oracle with that one line changed returns a shorter hypothesis for it).
# test_cpu_beam_cases.py enforces every condition on this table from the oracle alone.
CASES = [
    #    name           E    V     nb  L   min ngram rep  lpen prompt eos   seeds                 uncertain
    Case("nb2_b1",      128, 1000, 2,  16, 0,  0,    1.0, 1.0, 1,     784,  (34,),                ()),
    Case("nb3_b5",      128, 1000, 3,  24, 2,  3,    1.1, 1.0, 1,     765,  (73, 35, 15, 5, 1),   (1,)),
    Case("nb4_lp2",     128, 1000, 4,  12, 2,  2,    1.1, 2.0, 1,     765,  (58, 10),             ()),
    Case("nb5_lp0",     128, 1000, 5,  16, 4,  3,    1.1, 0.0, 1,     843,  (77, 30, 21),         ()),
    Case("nb6_plain",   128, 1000, 6,  16, 0,  2,    1.0, 1.0, 1,     765,  (67, 19),             ()),
    Case("nb7",         128, 1000, 7,  16, 3,  3,    1.1, 1.0, 1,     97,   (34, 14),             ()),
    Case("nb8_b8",      128, 1000, 8,  12, 2,  3,    1.1, 1.0, 1,     843,  (11, 298, 156, 98, 168, 193, 79, 147), ()),
    Case("v2053_nb8",   128, 2053, 8,  12, 0,  3,    1.1, 1.0, 1,     2052, (50, 55),             ()),
    Case("v2053_early", 128, 2053, 3,  16, 2,  3,    1.1, 1.0, 1,     1997, (7, 17, 14),          ()),
    Case("long_s64",    128, 1000, 3,  64, 4,  3,    1.1, 1.0, 60,    450,  (147, 23),            ()),
    Case("e256_nb4",    256, 1000, 4,  16, 2,  3,    1.1, 1.0, 1,     375,  (57, 34, 66),         ()),
]
BY_NAME = {c.name: c for c in CASES}
# the cases transformers' own generate() pins (tests/golden/beam_eos, written by make_goldens.py)
GOLDEN_CASES = ("nb2_b1", "nb3_b5", "nb4_lp2", "nb5_lp0", "nb6_plain", "nb7", "nb8_b8", "v2053_early",
                "long_s64", "e256_nb4")
BF16_CASES = ("nb3_b5", "nb6_plain", "e256_nb4")


def arch(E: int, V: int = S.VOCAB) -> GPT2Arch:
    if V == S.VOCAB:
        return S.arch(E)
    return GPT2Arch(f"beam_{E}_{V}", E, S.NLAYER, E // 64, vocab=V, n_positions=S.NPOS,
                    bos_token_id=V - 1, eos_token_id=V - 1)


@lru_cache(maxsize=None)
def state_dict(E: int, V: int = S.VOCAB):
    return S.state_dict(E) if V == S.VOCAB else weights.synthetic_gpt2(S.WEIGHT_SEED, arch(E, V))


@lru_cache(maxsize=None)
def sd64(E: int, V: int = S.VOCAB):
    return {k: torch.from_numpy(v.copy()).double() for k, v in state_dict(E, V).items()}


def prefix_rows(E: int, seeds) -> torch.Tensor:
    """0.1 * randn [len(seeds), 4, E] f32, one fixed CPU generator per row seed."""
    return torch.cat([0.1 * torch.randn(1, S.PREFIX_LEN, E, generator=torch.Generator().manual_seed(7919 * E + s),
                                        dtype=torch.float32) for s in seeds])


def prefix(c: Case) -> torch.Tensor:
    return prefix_rows(c.E, c.seeds)


def prompt(c: Case):
    return [c.V - 1] + [(37 * i + 11) % (c.V - 1) for i in range(c.prompt_len - 1)]


def search_kwargs(c: Case) -> dict:
    """The keyword arguments vcap.search's three searches share."""
    return dict(num_beams=c.nb, max_new_tokens=c.L, min_new_tokens=c.min_new, no_repeat_ngram_size=c.ngram,
                repetition_penalty=c.rep, eos=c.eos, length_penalty=c.lpen)


def run_oracle(c: Case, seeds=None, f32: bool = False):
    """oracle.generate_beam on the rows `seeds` (default: the case's batch) -> (ids rows, trace).
    The forward runs on float64 weights (f32: on the float32 state dict, as transformers runs it)."""
    ar = arch(c.E, c.V)
    sd = state_dict(c.E, c.V) if f32 else sd64(c.E, c.V)
    pre = prefix_rows(c.E, c.seeds if seeds is None else seeds)
    trace = {}
    with torch.no_grad():
        x = O.build_inputs(sd, ar, pre if f32 else pre.double(), prompt(c))
        rows = O.generate_beam(sd, ar, x, num_beams=c.nb, max_new_tokens=c.L, min_new_tokens=c.min_new,
                               repetition_penalty=c.rep, no_repeat_ngram_size=c.ngram, length_penalty=c.lpen,
                               eos_token_id=c.eos, trace=trace)
    return rows, trace


@lru_cache(maxsize=None)
def oracle(name: str):
    """The case's batch through the fp64-forward oracle, computed once and shared: (ids, trace)."""
    return run_oracle(BY_NAME[name])


def margin_over_bound(c: Case, trace: dict, b: int) -> float:
    """min over the row's steps of margin / GAP(E, step): the row is certain when this exceeds 1."""
    return min((m / gap(c.E, t) for t, m in enumerate(trace["margins"][b])), default=float("inf"))


def certain(c: Case, trace: dict, b: int) -> bool:
    return all(m > gap(c.E, t) for t, m in enumerate(trace["margins"][b]))


def listed_certain(c: Case):
    return [s not in c.uncertain for s in c.seeds]


def padded(rows, width: int, eos: int):
    return [list(r) + [eos] * (width - len(r)) for r in rows]
