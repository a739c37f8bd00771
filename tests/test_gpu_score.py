"""Teacher-forced scoring on the GPU: vcap_gpt2_score (masked attention, the all-rows lm_head + fused
cross-entropy of csrc/score.hip) and its Python surface (HipGPT2Decoder.score, HipTextDecoder.forward,
HipVideoCaptionModel.forward / compute_loss / score_ids) against the masked fp64 oracle of
tests/score_cases.py and the reference's own outputs (tests/golden/score_*.npz).

Tolerances (none comes from a measured result):
  f32   logits within decoder_shapes.FP32_TOL (1e-3, the project's bar); log-probs and loss within 2e-3 (a
        log-prob's error is the target logit's plus the log-sum-exp's, each at most the max logit error)
  bf16  logits within decoder_shapes.bf16_tolerance(fp64, bf16-emulated CPU forward of the same case);
        log-probs and loss within twice that
Shapes are the smallest that reach each path: a vocabulary of 1009 (prime: the last 128-column tile
holds 113 columns, its second 64-column part 49), 5 / 21 / 135 rows (less than a tile, one tile, two
tiles with 7 rows in the last), 512 rows (four row tiles), contexts of 12 (one-wave attention) and 80
(page-table attention)."""
import ctypes as C
from functools import lru_cache

import numpy as np
import pytest
import torch

import decoder_shapes as DS
import score_cases as SC
from helpers import golden
from vcap import _native as N
from vcap import configs, fidelity, prng, weights
from vcap.caption import HipTextDecoder, HipVideoCaptionModel
from vcap.model import HipGPT2Decoder

pytestmark = pytest.mark.gpu
PRECS = ["fp32", "bf16"]


@lru_cache(maxsize=None)
def decoder(E, V, prec, gain=1.0):
    return HipGPT2Decoder(SC.state_dict(E, V, gain), SC.arch(E, V), prec, "cuda", screen=False)


def abi_score(dec, x, km=None, tg=None, want_logits=False):
    """One raw vcap_gpt2_score call -> (rc, logits, logprobs, loss[2]); outputs pre-filled with NaN."""
    dev = dec.device
    B, S, _ = x.shape
    x = x.to(dev, torch.float32).contiguous()
    km = None if km is None else km.to(dev, torch.uint8).contiguous()
    tg = None if tg is None else tg.to(dev, torch.int32).contiguous()
    nan = float("nan")
    logits = torch.full((B, S, dec.arch.vocab), nan, device=dev) if want_logits else None
    lp = torch.full((B, S), nan, device=dev) if tg is not None else None
    loss = torch.full((2,), nan, device=dev) if tg is not None else None
    ws = torch.empty(max(int(N.lib().vcap_gpt2_score_workspace_bytes(C.byref(dec.desc), B, S)), 1), dtype=torch.uint8,
                     device=dev)
    rc = N.lib().vcap_gpt2_score(C.byref(dec.desc), x.data_ptr(), B, S, N.ptr(km), N.ptr(tg), N.ptr(logits),
                                 N.ptr(lp), N.ptr(loss), ws.data_ptr(), ws.numel(),
                                 torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize(dev)
    return rc, logits, lp, loss


def tolerances(c, prec):
    """(logit tolerance, log-prob / loss tolerance) of the case, from the CPU forwards alone."""
    if prec == "fp32":
        return DS.FP32_TOL * c.gain, 2e-3 * c.gain
    t = DS.bf16_tolerance(SC.reference(c), SC.reference(c, "bf16"))
    return t, 2.0 * t


def check(c, prec, res, rows=slice(None)):
    """A ScoreResult-like (logits, logprobs, nll_sum, count) against the fp64 oracle of case c."""
    ref = SC.reference(c)[rows]
    tg = SC.targets(c)[rows]
    ltol, ptol = tolerances(c, prec)
    lp_ref, nll_ref, cnt_ref = SC.target_logprobs(ref, tg)
    if res.logits is not None:
        err = float((res.logits.double().cpu() - ref).abs().max())
        print(f"{c.name} {prec}: max |logit err| {err:.3e} (tol {ltol:.3e})")
        assert torch.isfinite(res.logits).all()
        assert err <= ltol
    lp = res.logprobs.double().cpu()
    perr = float((lp - lp_ref).abs().max())
    loss, loss_ref = float(res.nll_sum) / float(res.count), nll_ref / cnt_ref
    print(f"{c.name} {prec}: max |logprob err| {perr:.3e}, loss {loss:.6f} vs {loss_ref:.6f} (tol {ptol:.3e})")
    assert torch.isfinite(lp).all()
    assert bool((lp[tg < 0] == 0).all())
    assert perr <= ptol
    assert int(res.count) == cnt_ref
    assert abs(loss - loss_ref) <= ptol


# ---------------------------------------------------------------------------- 1. ragged rows / columns

@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("B,S", [(1, 5), (3, 7), (5, 27)])
def test_ragged_rows_and_columns(device, prec, B, S):
    c = SC.Case(f"ragged_{B}x{S}", 128, 1009, B, S, targets="edges")
    dec = decoder(c.E, c.V, prec)
    check(c, prec, dec.score(SC.embeds(c), None, SC.targets(c), want_logits=True))


@pytest.mark.parametrize("prec", PRECS)
def test_all_targets_ignored(device, prec):
    c = SC.Case("ignored", 128, 1009, 3, 7, targets="ignored")
    res = decoder(c.E, c.V, prec).score(SC.embeds(c), None, SC.targets(c))
    assert float(res.count) == 0.0 and float(res.nll_sum) == 0.0
    assert bool((res.logprobs == 0).all())
    assert torch.isnan(res.loss)


# ---------------------------------------------------------------------------- 2. max rows, 7. 8.

MAXC = SC.Case("max_rows", 256, 1000, 9, 64)   # 576 rows: the first 8 sequences fill one call


@pytest.mark.parametrize("prec", PRECS)
def test_max_rows_and_chunking(device, prec):
    dec = decoder(MAXC.E, MAXC.V, prec)
    x, tg = SC.embeds(MAXC), SC.targets(MAXC)
    assert N.lib().vcap_gpt2_max_rows() == 512
    rc, _, _, _ = abi_score(dec, x, None, tg)
    assert rc == N.E_UNSUPPORTED
    rc, logits, lp, loss = abi_score(dec, x[:8], None, tg[:8], want_logits=True)
    assert rc == 0
    from vcap.model import ScoreResult
    check(MAXC, prec, ScoreResult(logits, lp, loss[0], loss[1]), rows=slice(0, 8))
    # the Python layer chunks 9 sequences into 8 + 1 and adds the pairs in chunk order
    res = dec.score(x, None, tg, want_logits=True)
    check(MAXC, prec, res)
    rc, _, _, loss9 = abi_score(dec, x[8:], None, tg[8:])
    assert rc == 0
    want = (float(loss[0]) + float(loss9[0])) / (float(loss[1]) + float(loss9[1]))
    assert abs(float(res.loss) - want) <= 1e-6 * abs(want)
    assert torch.equal(res.logprobs[:8], lp)


def test_deterministic_and_optional_outputs(device):
    dec = decoder(MAXC.E, MAXC.V, "bf16")
    x, tg = SC.embeds(MAXC)[:8], SC.targets(MAXC)[:8]
    a = abi_score(dec, x, None, tg, want_logits=True)
    b = abi_score(dec, x, None, tg, want_logits=True)
    c = abi_score(dec, x, None, tg, want_logits=False)
    assert a[0] == b[0] == c[0] == 0
    for u, v in zip(a[1:], b[1:]):
        assert torch.equal(u.view(torch.int32), v.view(torch.int32))
    assert torch.equal(a[2].view(torch.int32), c[2].view(torch.int32))
    assert torch.equal(a[3].view(torch.int32), c[3].view(torch.int32))
    # logits only (no targets): the same logits
    rc, lg, _, _ = abi_score(dec, x, None, None, want_logits=True)
    assert rc == 0 and torch.equal(lg.view(torch.int32), a[1].view(torch.int32))


# ---------------------------------------------------------------------------- 3. widths

@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("E", [128, 384, 768, 1024])
def test_widths(device, prec, E):
    c = SC.Case(f"width_{E}", E, 1000, 3, 12)
    check(c, prec, decoder(E, c.V, prec).score(SC.embeds(c), None, SC.targets(c), want_logits=True))


# ---------------------------------------------------------------------------- 4. masks

@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("mask,B,S", [("right", 3, 12), ("interior", 3, 12), ("interior", 2, 80)])
def test_masks(device, prec, mask, B, S):
    c = SC.Case(f"mask_{mask}_{S}", 128, 1009, B, S, mask=mask)
    km = SC.key_mask(c)
    assert int((km == 0).sum()) > 0
    check(c, prec, decoder(c.E, c.V, prec).score(SC.embeds(c), km, SC.targets(c), want_logits=True))


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("S", [12, 80])
def test_null_mask_is_all_ones_mask(device, prec, S):
    c = SC.Case("null_vs_ones", 128, 1009, 2, S)
    dec = decoder(c.E, c.V, prec)
    a = abi_score(dec, SC.embeds(c), None, SC.targets(c), want_logits=True)
    b = abi_score(dec, SC.embeds(c), torch.ones(c.B, c.S, dtype=torch.uint8), SC.targets(c), want_logits=True)
    assert a[0] == b[0] == 0
    for u, v in zip(a[1:], b[1:]):
        assert torch.equal(u.view(torch.int32), v.view(torch.int32))


def test_hidden_first_key_is_an_argument_error(device):
    c = SC.Case("first_key", 128, 1009, 3, 7)
    dec = decoder(c.E, c.V, "fp32")
    km = torch.ones(c.B, c.S, dtype=torch.uint8)
    km[1, 0] = 0
    with pytest.raises(N.VcapError) as ei:
        dec.score(SC.embeds(c), km, SC.targets(c))
    assert ei.value.rc == N.E_ARG
    # the raw call checks on the device: the offending sequence's log-probs and the loss sum are NaN
    rc, _, lp, loss = abi_score(dec, SC.embeds(c), km, SC.targets(c))
    assert rc == 0
    assert torch.isnan(lp[1]).all() and torch.isfinite(lp[0]).all() and torch.isfinite(lp[2]).all()
    assert torch.isnan(loss[0])
    # bad arguments the host can see
    assert abi_score(dec, SC.embeds(c), None, None, want_logits=False)[0] == N.E_ARG


# ---------------------------------------------------------------------------- 5. log-sum-exp stability

def test_large_logits(device):
    base = SC.Case("gain_probe", 128, 1009, 3, 7)
    peak = float(SC.reference(base).abs().max())
    gain = float(2 ** int(np.ceil(np.log2(120.0 / peak))))    # a power of two: every logit scales exactly
    c = base._replace(name="large_logits", gain=gain)
    assert float(SC.reference(c).abs().max()) > 100.0          # exp() of it overflows f32 (88.7)
    check(c, "fp32", decoder(c.E, c.V, "fp32", gain).score(SC.embeds(c), None, SC.targets(c), want_logits=True))


# ---------------------------------------------------------------------------- 6. the step-wise path

@pytest.mark.parametrize("prec", PRECS)
def test_matches_stepwise_teacher_forcing(device, prec):
    E, B, steps = 768, 4, 8
    dec = HipGPT2Decoder(DS.state_dict(E), DS.arch(E), prec, device, screen=False)
    pre, prompt = DS.prefix(E, B), DS.prompt(E)
    g = torch.Generator().manual_seed(99)
    toks = torch.randint(0, DS.VOCAB - 1, (B, steps), generator=g)
    tf = fidelity.teacher_forced_logits(dec, pre.to(device), prompt, toks, steps)       # [steps, B, V]
    ids = torch.cat([torch.tensor([prompt] * B), toks[:, :-1]], dim=1).to(device)
    x = torch.cat([pre.to(device), dec.wte[ids].float()], dim=1)                      # S = 4 + 1 + 7
    s0 = pre.shape[1] + len(prompt)
    got = dec.score(x, want_logits=True).logits[:, s0 - 1:].transpose(0, 1)
    tol = DS.FP32_TOL
    if prec == "bf16":
        tol = DS.bf16_tolerance(DS.teacher_forced(E, pre, prompt, toks.numpy(), "fp64"),
                                DS.teacher_forced(E, pre, prompt, toks.numpy(), "bf16"))
    err = float((got - tf).abs().max())
    print(f"score vs step-wise {prec}: max |diff| {err:.3e} (tol {tol:.3e})")
    assert err <= tol


# ---------------------------------------------------------------------------- 9. reference goldens

@lru_cache(maxsize=None)
def tiny_model():
    meta, _ = golden("score_tiny")
    va, ga = configs.vit_arch(meta["vit"]), configs.gpt2_arch(meta["gpt2"])
    sd = weights.synthetic_state_dict(meta["weights_seed"], va, ga)
    return HipVideoCaptionModel(sd, meta["vit"], meta["gpt2"], precision="fp32", device="cuda",
                                decoder_precision="fp32")


def test_reference_forward_tiny(device):
    meta, arr = golden("score_tiny")
    dec = tiny_model().decoder
    out = dec(torch.from_numpy(arr["video_emb"]), torch.from_numpy(arr["input_ids"]).long(),
              torch.from_numpy(arr["attention_mask"]).long(), torch.from_numpy(arr["labels"]).long())
    err = float((out["logits"].cpu() - torch.from_numpy(arr["logits"])).abs().max())
    print(f"forward tiny: max |logit err| {err:.3e}, loss {float(out['loss']):.6f} vs {meta['loss']:.6f}")
    assert out["logits"].shape == arr["logits"].shape and out["loss"].dim() == 0
    assert err <= 1e-3
    assert abs(float(out["loss"]) - meta["loss"]) <= 2e-3
    # attention_mask = None -> input_ids != pad; labels = None -> no loss
    out_d = dec(torch.from_numpy(arr["video_emb"]), torch.from_numpy(arr["input_ids"]).long(), None,
                torch.from_numpy(arr["labels"]).long())
    assert abs(float(out_d["loss"]) - meta["loss_default_mask"]) <= 2e-3
    assert dec(torch.from_numpy(arr["video_emb"]), torch.from_numpy(arr["input_ids"]).long())["loss"] is None


def test_reference_compute_loss_and_model_forward(device):
    meta, arr = golden("score_tiny")
    model = tiny_model()
    va = configs.vit_arch(meta["vit"])
    video = torch.from_numpy(prng.imagenet_frames(meta["frames_seed"], (meta["B"], meta["T"], 3, va.image, va.image)))
    loss = model.compute_loss(video, torch.from_numpy(arr["caption_ids"]).long(), meta["pad_id"])
    print(f"compute_loss {float(loss):.6f} vs {meta['compute_loss']:.6f}")
    assert loss.dim() == 0 and abs(float(loss) - meta["compute_loss"]) <= 2e-3
    out = model(video, torch.from_numpy(arr["input_ids"]).long(), torch.from_numpy(arr["attention_mask"]).long(),
                torch.from_numpy(arr["labels"]).long())
    assert float((out["logits"].cpu() - torch.from_numpy(arr["logits"])).abs().max()) <= 1e-3
    assert abs(float(out["loss"]) - meta["loss"]) <= 2e-3


def test_score_ids_sums(device):
    """score_ids (engine prefix path, no logits) against the forward's log-probs along the same tokens."""
    meta, arr = golden("score_tiny")
    model = tiny_model()
    va, ga = configs.vit_arch(meta["vit"]), configs.gpt2_arch(meta["gpt2"])
    video = torch.from_numpy(prng.imagenet_frames(meta["frames_seed"], (meta["B"], meta["T"], 3, va.image, va.image)))
    ids = [[5, 900, 17, 1000, 3, 44, ga.eos_token_id], [7, 8, 9], [1022, 0, 511, 64, 128]]
    lp, lens, sums = model.score_ids(video, ids)
    assert lens.tolist() == [7, 3, 5] and lp.shape == (3, 7)
    _, prefix = model.encode_prefix(video, 0.6, 0.4)
    L = 7
    inp = torch.full((3, 1 + L), ga.eos_token_id, dtype=torch.long)
    lab = torch.full((3, 1 + L), -100, dtype=torch.long)
    for b, r in enumerate(ids):
        inp[b, 1:1 + len(r)] = torch.tensor(r)
        lab[b, 1:1 + len(r)] = torch.tensor(r)
    res = model.decoder.forward_from_prefix(prefix, inp, torch.ones_like(inp), lab)
    want = res.logprobs.sum(dim=1)
    print("score_ids sums", sums.tolist(), "forward", want.tolist())
    assert float((sums - want).abs().max()) <= 1e-4
    assert bool((lp[1, 3:] == 0).all())
    # and against the fp64 oracle of the same inputs
    sd = {k: torch.from_numpy(np.ascontiguousarray(v)).double()
          for k, v in weights.synthetic_state_dict(meta["weights_seed"], va, ga).items()}
    x = torch.cat([prefix.double().cpu(), sd[DS.WTE][inp]], dim=1)
    with torch.no_grad():
        ref = SC.masked_forward(sd, ga, x)
    lp_ref, _, _ = SC.target_logprobs(ref, SC.shift_labels(lab))
    assert float((res.logprobs.double().cpu() - lp_ref).abs().max()) <= 2e-3


def test_reference_forward_gpt2(device):
    meta, arr = golden("score_gpt2")
    ga = configs.gpt2_arch(meta["gpt2"])
    dec = HipTextDecoder(weights.synthetic_gpt2(meta["weights_seed"], ga), ga, "fp32", device)
    res = dec.forward_from_prefix(dec.prefix_embeds(torch.from_numpy(arr["video_emb"]).to(device)),
                                  torch.from_numpy(arr["input_ids"]).long(),
                                  torch.from_numpy(arr["attention_mask"]).long(),
                                  torch.from_numpy(arr["labels"]).long())
    top = res.logits.cpu().gather(2, torch.from_numpy(arr["logits_top_i"]).long())
    err = float((top - torch.from_numpy(arr["logits_top_v"])).abs().max())
    perr = float((res.logprobs.double().cpu() - torch.from_numpy(arr["target_logprob"])).abs().max())
    print(f"forward gpt2: top-64 |err| {err:.3e}, |logprob err| {perr:.3e}, loss {float(res.loss):.6f} vs {meta['loss']:.6f}")
    assert err <= 1e-3
    assert perr <= 2e-3
    assert abs(float(res.loss) - meta["loss"]) <= 2e-3


# ---------------------------------------------------------------------------- 10. unmasked attention

def _attn_ref(q, kc, vc, pt, maxp, H, S_new, past):
    M = q.shape[0]
    out = torch.empty(M, H * 64, dtype=torch.float64)
    q, kc, vc = q.double().cpu(), kc.double().cpu(), vc.double().cpu()
    for m in range(M):
        seq, qpos = m // S_new, past + m % S_new
        pos = torch.arange(qpos + 1)
        pages = pt.cpu()[seq, pos // 16].long() if pt is not None else seq * maxp + pos // 16
        kk, vv = kc[pages, :, pos % 16], vc[pages, :, pos % 16]
        att = torch.einsum("hd,chd->hc", q[m].reshape(H, 64), kk) / 8.0
        out[m] = torch.einsum("hc,chd->hd", att.softmax(-1), vv).reshape(-1)
    return out


@pytest.mark.parametrize("prec,S_new,past,paged", [("bf16", 1, 28, False), ("bf16", 5, 0, False), ("bf16", 3, 70, True),
                                                   ("fp32", 1, 28, True), ("fp32", 7, 60, True)])
def test_unmasked_attention_unchanged(device, prec, S_new, past, paged):
    """vcap_decode_attention (no mask: the kernels every decode step runs) against an fp64 reference, and
    bit-identical before and after masked calls of the same kernels' masked instantiations."""
    tdt, dt = (torch.bfloat16, N.DT_BF16) if prec == "bf16" else (torch.float32, N.DT_F32)
    seqs, H = 3, 2
    maxp = (past + S_new + 15) // 16 + 1
    M = seqs * S_new
    g = torch.Generator().manual_seed(1000 * S_new + past)
    q = torch.randn(M, H * 64, generator=g).to(device, tdt)
    kc = torch.randn(seqs * maxp, H, 16, 64, generator=g).to(device, tdt)
    vc = torch.randn(seqs * maxp, H, 16, 64, generator=g).to(device, tdt)
    pt = torch.randperm(seqs * maxp, generator=g).int().reshape(seqs, maxp).to(device) if paged else None

    def run():
        out = torch.full((M, H * 64), float("nan"), dtype=tdt, device=device)
        N.check(N.lib().vcap_decode_attention(dt, q.data_ptr(), kc.data_ptr(), vc.data_ptr(), N.ptr(pt), maxp,
                                              out.data_ptr(), M, H, S_new, past,
                                              torch.cuda.current_stream(device).cuda_stream), "decode attention")
        torch.cuda.synchronize(device)
        return out

    before = run()
    for S in (12, 80):   # masked one-wave and page-table attention in between
        c = SC.Case("between", 128, 1009, 2, S, mask="interior")
        assert abi_score(decoder(c.E, c.V, prec), SC.embeds(c), SC.key_mask(c), SC.targets(c))[0] == 0
    after = run()
    assert torch.equal(before.view(torch.int16 if prec == "bf16" else torch.int32),
                       after.view(torch.int16 if prec == "bf16" else torch.int32))
    tol = 1e-2 if prec == "bf16" else 1e-5   # test_gpu_bf16.py::test_decode_attention's bars
    torch.testing.assert_close(before.double().cpu(), _attn_ref(q, kc, vc, pt, maxp, H, S_new, past), rtol=tol, atol=tol)
