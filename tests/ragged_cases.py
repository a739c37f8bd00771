"""Shared by test_cpu_ragged.py and test_gpu_ragged.py: the ragged-prompt cases on the 2-layer sweep
decoders of tests/decoder_shapes.py (imported as it is).

LENS with the sweep's 4 prefix rows gives S0 = 4, 5, 15, 16, 17, 54: three rows straddle the 16-position
page edge, and the last row's context crosses 64 at step 10 while the others stay short (so one launch
holds rows on both sides of the <= 64 attention form).  Row b's prompt depends on b, so no two rows
share ids.  n_embd 256 is the width where the f32 mlp c_proj takes the unsplit K = 1024 kernel."""
from __future__ import annotations

from functools import lru_cache

import torch

import decoder_shapes as S

LENS = (0, 1, 11, 12, 13, 50)
WIDTHS = (128, 256)
PRECS = ("bf16", "fp32")
BEAM_CASES = (((0, 1, 13), 16), ((0, 12, 50), 24))   # (lens, max_new): ancestry <= 64 form / general form
BEAM_WIDTHS = (2, 3, 4)


def prompts(E: int, lens=LENS):
    """Row b: ([bos] + [(37 i + 11 + 5 b) % (VOCAB - 1) ...])[:len_b]; length 0 is the empty prompt."""
    bos = S.arch(E).bos_token_id
    return [([bos] + [(37 * i + 11 + 5 * b) % (S.VOCAB - 1) for i in range(n - 1)])[:n] for b, n in enumerate(lens)]


def prefix(E: int) -> torch.Tensor:
    """0.1 * randn [6, 4, E] f32 from a fixed CPU generator; a case of n rows takes the first n."""
    k = {128: 0, 256: 1}[E]
    g = torch.Generator().manual_seed(7000 * E + 6 + 100000 * k)
    return 0.1 * torch.randn(len(LENS), S.PREFIX_LEN, E, generator=g, dtype=torch.float32)


@lru_cache(maxsize=None)
def near_tie_shares(E: int):
    """Per row of the LENS case, along the fp64 oracle's own greedy path at B = 1 with the row's prompt:
    (share of steps the fp32 rule skips, share the bf16 rule skips) - gap 2 x FP32_TOL and
    decoder_shapes.bf16_token_gap, the rules test_gpu_decoder_shapes._check_logits_and_tokens applies."""
    pre, out = prefix(E), []
    for b, pr in enumerate(prompts(E)):
        row = pre[b:b + 1]
        ids = S.oracle_greedy(E, row, pr)
        ref = S.teacher_forced(E, row, pr, ids, "fp64")
        emu = S.teacher_forced(E, row, pr, ids, "bf16")
        _, bound32 = S.token_check(E, ref, ids, 2.0 * S.FP32_TOL)
        _, bound16 = S.token_check(E, ref, ids, S.bf16_token_gap(ref, emu))
        out.append((1.0 - float(bound32.mean()), 1.0 - float(bound16.mean())))
    return out
