"""Decoder width sweep against the fp64 oracle: n_embd 256 / 384 / 512 / 640 / 896 (accepted by the
ABI, pinned by no golden) plus the anchors 128 and 768, bf16 and fp32, 1 / 5 / 16 / 20 rows (prefill
of 5 / 25 / 80 / 100 rows: the one-tile and two-tile row chunks and several blockIdx.y chunks; decode
steps on both sides of the 16-row limits), vocab 1000 (a partial last 16-column tile and a partial
last 4-tile workgroup), and one 54-position prompt whose context crosses 64 (c64 -> paged attention).
DESIGN.md "Decoder widths" lists the kernel each width reaches.

Per case, along the GPU's own ids (teacher-forced fp64 forward, tests/decoder_shapes.py):
  1. raw logits: fp32 max |gpu - fp64| < 1e-3 (the project's bar).  bf16: max |gpu - fp64| < tol_bf16
     = 3 x max |emulated - fp64|, and max |gpu - emulated| <= tol_bf16 / 3 + 1e-3, where `emulated`
     is the fp64 oracle with bf16 rounding exactly where the kernels round - both bounds come from
     the two CPU forwards, never from a GPU run.  Largest tol_bf16 on the CPU (oracle's own path):
     5.0e-2 at n_embd 896, 1.0e-2 at 128 (test_cpu_decoder_shapes.py prints every case's);
  2. tokens: the GPU id is the processed fp64 argmax wherever the fp64 top-2 gap exceeds 2e-3 (fp32)
     or decoder_shapes.bf16_token_gap (bf16: at most 2 x tol_bf16; why it is tighter is argued
     there); at most 15 % of the (row, step) pairs may be near-ties;
  3. every logit is finite;
  4. rows 16 / 20: the last row decoded alone (B = 1) gives the same ids, bit-identical fp32 logits
     (the arithmetic may not depend on the launch's M), bf16 logits within the same tolerance.
The captured-graph run and the grid-capped run (max_blocks 40: 2- and 4-tile workgroups) give the
eager ids exactly.

The fp32 n_embd 256 shape (K = 1024 mlp c_proj: vcap_rows_gemv_kernel<float, .., 16>) first ran
after vcap_rows_gemm_dispatch stopped passing it the K-split buffers it cannot honour."""
import numpy as np
import pytest
import torch

import decoder_shapes as S
from vcap.model import GenConfig, HipGPT2Decoder

pytestmark = pytest.mark.gpu
PRECS = ("bf16", "fp32")


@pytest.fixture(scope="module")
def decoder(device):
    made = {}

    def get(E, prec):
        if (E, prec) not in made:
            made[(E, prec)] = HipGPT2Decoder(S.state_dict(E), S.arch(E), prec, device)
        return made[(E, prec)]
    return get


def _cfg(ga, use_graph, cap=0):
    cfg = GenConfig(S.STEPS, S.STEPS, S.NGRAM, S.REP, ga.eos_token_id, ga.eos_token_id, use_graph)
    cfg.max_blocks = cap
    return cfg


def _run(dec, pre, prompt, cfg, logits=False):
    """-> (ids [B, steps], raw logits [B, steps, V] or None)."""
    ga = dec.arch
    lg = torch.empty(cfg.max_new_tokens, pre.shape[0], ga.vocab, dtype=torch.float32, device=pre.device) if logits else None
    ids = dec.generate_ids(pre, prompt, cfg, logits_out=lg)
    torch.cuda.synchronize()
    return ids.cpu().numpy(), (lg.permute(1, 0, 2).contiguous().cpu().numpy() if logits else None)


def _check_logits_and_tokens(E, prec, pre_cpu, prompt, ids, lg, tag):
    """Assertions 1 - 3 for one run; returns the logits tolerance it used."""
    assert np.isfinite(lg).all(), tag
    ref = S.teacher_forced(E, pre_cpu, prompt, ids, "fp64")
    err64 = float(np.abs(lg - ref.numpy()).max())
    if prec == "fp32":
        tol, gap_min = S.FP32_TOL, 2.0 * S.FP32_TOL
        print(f"\nsweep-gpu {tag} max|gpu-fp64|={err64:.3e} (bar {tol:.0e})", end="")
        assert err64 < tol, (tag, err64)
    else:
        emu = S.teacher_forced(E, pre_cpu, prompt, ids, "bf16")
        tol, gap_min = S.bf16_tolerance(ref, emu), S.bf16_token_gap(ref, emu)
        erre = float(np.abs(lg - emu.numpy()).max())
        print(f"\nsweep-gpu {tag} max|gpu-fp64|={err64:.3e} (tol_bf16 {tol:.3e}) "
              f"max|gpu-emulated|={erre:.3e} (bound {tol / 3 + 1e-3:.3e})", end="")
        assert err64 < tol, (tag, err64, tol)
        assert erre <= tol / 3 + 1e-3, (tag, erre, tol / 3 + 1e-3)
    arg, bound = S.token_check(E, ref, ids, gap_min)
    skipped = 1.0 - float(bound.mean())
    print(f" near-ties skipped {skipped:.3f}", end="")
    assert skipped <= S.SKIP_CAP, (tag, skipped)
    assert np.array_equal(ids[bound], arg[bound]), (tag, np.argwhere(bound & (ids != arg)).tolist())
    return tol


def _sweep(decoder, device, E, B, prec, long=False):
    dec, ga = decoder(E, prec), S.arch(E)
    pre_cpu, prompt = S.prefix(E, B), S.prompt(E, long)
    pre = pre_cpu.to(device)
    tag = f"n_embd={E} B={B} {prec}{' long' if long else ''}"
    ids, lg = _run(dec, pre, prompt, _cfg(ga, False), logits=True)
    tol = _check_logits_and_tokens(E, prec, pre_cpu, prompt, ids, lg, tag)
    gids, _ = _run(dec, pre, prompt, _cfg(ga, True))
    assert np.array_equal(gids, ids), (tag, "captured graph")
    if not long:
        cids, _ = _run(dec, pre, prompt, _cfg(ga, False, cap=40))
        assert np.array_equal(cids, ids), (tag, "max_blocks 40")
    if B >= 16:
        r = B - 1
        ids1, lg1 = _run(dec, pre[r:r + 1].contiguous(), prompt, _cfg(ga, False), logits=True)
        assert np.array_equal(ids1[0], ids[r]), (tag, "row alone", ids1[0], ids[r])
        d = float(np.abs(lg1[0] - lg[r]).max())
        print(f" row-alone max|diff|={d:.3e}", end="")
        if prec == "fp32":
            assert np.array_equal(lg1[0].view(np.int32), lg[r].view(np.int32)), (tag, d)
        else:
            assert d <= tol, (tag, d, tol)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("E,B", S.CASES)
def test_width_sweep(decoder, device, E, B, prec):
    _sweep(decoder, device, E, B, prec)


@pytest.mark.parametrize("prec", PRECS)
def test_context_crosses_64(decoder, device, prec):
    _sweep(decoder, device, S.LONG_E, S.LONG_B, prec, long=True)


@pytest.mark.parametrize("prec", PRECS)
def test_workspace_bytes_nonzero_at_every_width(decoder, prec):
    for E in (256, 384, 512, 640, 896):
        assert decoder(E, prec).workspace_bytes(20, 1, S.STEPS) > 0, E
