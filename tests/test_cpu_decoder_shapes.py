"""CPU side of the decoder width sweep (test_gpu_decoder_shapes.py): everything that sweep's bounds
rest on is derived here from the fp64 oracle alone, with no GPU in the loop.

  * the emulated-bf16 forward with its rounding switched off IS oracle.gpt2_forward (1e-12);
  * along the oracle's own greedy path, at most 15 % of the (row, step) pairs of every case are
    near-ties (fp64 processed top-2 gap <= 2 x tolerance) under either precision's tolerance - so
    the GPU token check binds on >= 85 % of the pairs and its skip cap is reachable;
  * the bf16 tolerance (3 x max |emulated - fp64|) is printed per case (pytest -s shows the table).
"""
import numpy as np
import pytest
import torch

import decoder_shapes as S


def test_emulation_without_rounding_is_the_oracle():
    E, B = 256, 3
    pre = S.prefix(E, B)
    ids = S.oracle_greedy(E, pre, S.prompt(E), steps=6)
    ref = S.teacher_forced(E, pre, S.prompt(E), ids, "fp64")
    emu = S.teacher_forced(E, pre, S.prompt(E), ids, "ident")
    assert ref.dtype == torch.float64 and ref.shape == (B, 6, S.VOCAB)
    assert float((ref - emu).abs().max()) < 1e-12


def test_teacher_forcing_reproduces_the_free_running_path():
    """One forward over [inputs, wte[ids[:, :-1]]] gives the logits the step-by-step loop saw: its
    processed argmax is the path itself."""
    E, B = 128, 2
    pre = S.prefix(E, B)
    ids = S.oracle_greedy(E, pre, S.prompt(E))
    ref = S.teacher_forced(E, pre, S.prompt(E), ids, "fp64")
    arg, _ = S.token_check(E, ref, ids, 0.0)
    assert np.array_equal(arg, ids)


def test_bf16_rne_rounds_to_nearest_even():
    x = torch.tensor([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -20, -3.0], dtype=torch.float64)
    assert S.bf16_rne(x).tolist() == [1.0, 1.0 + 2.0 ** -6, 1.0 + 2.0 ** -7, -3.0]


def _case_figures(E, B, long=False):
    pre, pr = S.prefix(E, B), S.prompt(E, long)
    ids = S.oracle_greedy(E, pre, pr)
    ref = S.teacher_forced(E, pre, pr, ids, "fp64")
    emu = S.teacher_forced(E, pre, pr, ids, "bf16")
    tol, gap16 = S.bf16_tolerance(ref, emu), S.bf16_token_gap(ref, emu)
    assert gap16 <= 2.0 * tol
    out = {"tol_bf16": tol, "gap_bf16": gap16, "share_2tol": 1.0 - float(S.token_check(E, ref, ids, 2.0 * tol)[1].mean())}
    for prec, t in (("fp32", 2.0 * S.FP32_TOL), ("bf16", gap16)):
        arg, bound = S.token_check(E, ref, ids, t)
        assert np.array_equal(arg[bound], ids[bound])      # the oracle's path is its own argmax
        out[prec] = 1.0 - float(bound.mean())
    return out


@pytest.mark.parametrize("E,B", S.CASES + [(S.LONG_E, S.LONG_B)])
def test_near_tie_share_within_cap(E, B):
    long = (E, B) == (S.LONG_E, S.LONG_B)
    f = _case_figures(E, B, long)
    print(f"\nsweep-cpu n_embd={E:4d} B={B:2d}{' long' if long else '     '} tol_bf16={f['tol_bf16']:.3e} "
          f"bf16 token gap={f['gap_bf16']:.3e} near-tie share fp32={f['fp32']:.3f} bf16={f['bf16']:.3f} "
          f"(cap {S.SKIP_CAP}; under gap > 2 tol_bf16 it would be {f['share_2tol']:.3f})")
    assert np.isfinite(f["tol_bf16"]) and f["tol_bf16"] > 0
    assert f["fp32"] <= S.SKIP_CAP, f
    assert f["bf16"] <= S.SKIP_CAP, f
