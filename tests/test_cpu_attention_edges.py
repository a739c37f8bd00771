"""CPU self-check of the attention edge inputs (tests/attention_edge_cases.py, test_gpu_attention_edges.py): the
inputs are what the docstring says, and the faults the end-to-end encoder checks cannot see in half precision
are far outside the tolerance here.  pytest -s prints the tolerance per pattern.

  * q / k are exact in every element type and the scores are +8 / -8 (patterns 1, 2) or 16 on the match with
    the rest spread at std about 2 (pattern 3);
  * pattern 1 gives v_j to within exp(-16) N max |v|, pattern 2 the mean of v;
  * the fused kernel's xn / W reproduce the same q / k exactly;
  * the last key dropped (pattern 1 with j = N - 1) and a padding key admitted (pattern 2) move the output by
    more than 100 x the tolerance; the output shifted by one row moves pattern 3 by more than the tolerance;
  * MXFP8 output (heads = 4): the same three faults, and a row tile left unwritten, each push at least one
    element past the per-element MXFP8 bound (half an e4m3 step of its block + the bf16 tolerance) at every
    token count of the MXFP8 runs, and the bf16 emulation itself stays inside that bound."""
import math

import numpy as np

import pytest
import torch

import attention_edge_cases as A
import mx_cases as MX
from encoder_shapes import generic_attention
from oracle import vcap_oracle as O

RUNS = [(p, n) for p in ("bf16", "fp16", "fp32") for n in A.TOKENS[p]]


def test_token_counts_sit_on_every_dispatch_edge():
    assert A.TOKENS["bf16"] == A.TOKENS["fp32"] == (1, 2, 17, 32, 193, 197, 208, 209, 224, 257, 272, 273, 288)
    assert set(A.TOKENS["fp16"]) - set(A.WINDOW_EDGES) == {33, 64, 65, 128, 129, 192, 225, 256}
    assert A.dominant_keys(197) == [0, 1, 15, 16, 31, 32, 180, 181, 195, 196]
    assert A.dominant_keys(17) == [0, 1, 15, 16] and A.dominant_keys(1) == [0] and A.dominant_keys(2) == [0, 1]
    # fp16 outside the windows: the generic kernel at each of its paddings 64 / 128 / 192 / 256
    assert [n for n in A.TOKENS["fp16"] if generic_attention("fp16", n)] == [33, 64, 65, 128, 129, 192, 225, 256]


@pytest.mark.parametrize("prec,n", RUNS, ids=[f"{p}-{n}" for p, n in RUNS])
def test_inputs_reference_and_faults(prec, n):
    tols = {}
    for pattern, j in A.variants(n):
        x = A.qkv(pattern, prec, n, j=j)
        assert x.shape == (2, n, 3, 2, 64)
        assert torch.equal(x, x.to(A.TORCH[prec]).double())                      # exact in the element type
        assert set(x[:, :, :2].abs().unique().tolist()) <= {0.0, 1.0, 2.0}
        q, k, v = x.permute(2, 0, 3, 1, 4).unbind(0)
        s = q @ k.transpose(-1, -2) / 8.0
        ref = A.attend(x)
        vmax = float(v.abs().max())
        tol = A.tolerance(x, prec, ref)
        tols[pattern] = max(tol, tols.get(pattern, 0.0))
        vt = v.transpose(1, 2).reshape(2, n, 128)                                 # [frames, n, heads * 64]
        if pattern == "dominant":
            want = torch.full_like(s, -8.0)
            want[..., j] = 8.0
            assert torch.equal(s, want)
            assert float((ref - vt[:, j:j + 1]).abs().max()) <= 2 * math.exp(-16) * n * vmax
            if j == n - 1 and n > 1:
                move = float((A.attend(x, fault="drop_key") - ref).abs().max())
                assert move > 100 * tol, (prec, n, move, tol)
        elif pattern == "uniform":
            assert torch.equal(s, torch.full_like(s, -8.0))
            assert float((ref - vt.mean(1, keepdim=True)).abs().max()) < 1e-12
            move = float((A.attend(x, fault="pad_key") - ref).abs().max())
            share = 1.0 / (1.0 + n * math.exp(-8))
            assert abs(move - share * float(vt.mean(1).abs().max())) < 1e-9
            assert move > 100 * tol, (prec, n, move, tol)
        else:
            pi = (7 * torch.arange(n) + 3) % n
            match = s[..., torch.arange(n), pi]
            assert torch.equal(match, torch.full_like(match, 16.0))
            if n >= 64:
                rest = s.clone()
                rest[..., torch.arange(n), pi] = float("nan")
                rest = rest[~rest.isnan()]
                assert 1.8 < float(rest.std()) < 2.2 and float(rest.max()) < 16.0
            if n > 1:
                move = float((torch.roll(ref, 1, dims=1) - ref).abs().max())
                assert move > tol and move > 0.5, (prec, n, move, tol)
    print(f"\nattention-cpu {prec} N={n}: tol " + " ".join(f"{p}={t:.3e}" for p, t in tols.items()), end="")


@pytest.mark.parametrize("n", A.FUSED_TOKENS)
@pytest.mark.parametrize("prec", ["bf16", "fp16"])
def test_fused_inputs_give_the_same_q_and_k(prec, n):
    for pattern, j in A.variants(n):
        xn, w, b, qk = A.fused_inputs(pattern, prec, n, j=j)
        for t in (xn, w):
            assert torch.equal(t, t.to(A.TORCH[prec]).double())
        assert set(w[:256].abs().unique().tolist()) <= {0.0, 1.0, 2.0} and not bool(b[:256].any())
        got = (xn @ w.t() + b).reshape(2, n, 3, 2, 64)
        assert torch.equal(got[:, :, :2], qk)
        assert torch.equal(qk, A.qkv(pattern, prec, n, j=j)[:, :, :2])
        assert 0.2 < float(got[:, :, 2].std()) < 2.0                             # a random v of ordinary size


@pytest.mark.parametrize("n", A.MX_TOKENS)
def test_faults_exceed_the_mxfp8_bound(n):
    frames, heads = 2, A.MX_HEADS
    M, D = frames * n, heads * 64
    assert A.MX_TOKENS == MX.ATTN_TOKENS and (heads * 64) % 256 == 0

    def over(x, moved, ref, term):
        return bool((np.abs(moved.reshape(M, D).numpy() - ref.reshape(M, D).numpy()) > MX.attention_mx_bound(ref.reshape(M, D).numpy(), term)).any())

    seen = set()
    for pattern, j in A.variants(n):
        x = A.qkv(pattern, "bf16", n, frames, heads, j)
        ref = A.attend(x)
        term = A.tolerance(x, "bf16", ref)
        # the emulated kernel output, quantised, passes its own check
        q, s = O.mx_quantize(A.attend(x, "bf16").reshape(M, D).float().numpy())
        assert not MX.attention_mx_check(ref.reshape(M, D).numpy(), term, q, s), (pattern, j)
        if pattern == "dominant" and j == n - 1:
            assert over(x, A.attend(x, fault="drop_key"), ref, term)
            seen.add("drop_key")
        if pattern == "uniform":
            assert over(x, A.attend(x, fault="pad_key"), ref, term)
            seen.add("pad_key")
        if pattern == "permutation":
            assert over(x, torch.roll(ref, 1, dims=1), ref, term)
            tile = ref.clone()
            tile[:, n - (n % 16 or 16):] = 0.0            # the last row tile never stored (a zeroed buffer)
            assert over(x, tile, ref, term)
            seen.add("row_tile")
    assert seen == {"drop_key", "pad_key", "row_tile"}
