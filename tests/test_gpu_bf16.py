"""Parity of the BENCHMARKED kernel set (bf16: gemm256<bf16>, the bf16 ViT attention, the CLS-tail
split-K, the bf16 rows GEMVs, decode_attention_c64, the lm_head processor epilogue) against the
reference's recorded outputs (tests/golden/b16_b8 = BASELINE configs[1], produced by running the
reference's own generate(): tests/golden/make_goldens.py) and against fp32 torch references at
the bench shapes.

Tolerances (bf16 operands, fp32 accumulation): teacher-forced step logits within BF16_LOGIT_TOL of
the reference's fp32 logits at every one of the 24 steps; greedy tokens identical wherever the
reference's processed top-2 gap exceeds that tolerance; free-running token agreement above a
stated floor (bf16 rounding flips near-ties, after which a greedy continuation legitimately
diverges - the fp32 mode is the token-exact one, tests/test_gpu_parity.py)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from helpers import case
from vcap import _native as N
from vcap import search
from vcap.caption import HipGPT2LMHead, _WTE
from vcap.model import GenConfig, HipGPT2Decoder, HipPrefix, HipViTEncoder, trim_generated

pytestmark = pytest.mark.gpu

BF16_LOGIT_TOL = 0.02          # |bf16 HIP - fp32 reference| on every raw logit the golden records (measured max 0.013)
BF16_E2E_TOL = 0.03            # the same bound for bf16 encoder + decoder (tests/test_gpu_fidelity.py, measured 0.019)
_CACHE = {}


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _models(prec, device, name="b16_b8"):
    meta, g, va, ga, sd, frames = case(name)
    key = (name, prec)
    if key not in _CACHE:
        _CACHE.clear()
        _CACHE[key] = (HipViTEncoder(sd, va, prec, device), HipPrefix(sd, ga.n_embd, device=device),
                       HipGPT2Decoder(sd, ga, prec, device))
    return (meta, g, va, ga, sd, frames) + _CACHE[key]


def _hf_cfg(ga, graph=True, max_blocks=0):
    c = GenConfig(24, 8, 3, 1.1, ga.eos_token_id, ga.eos_token_id, graph)
    c.max_blocks = max_blocks
    return c


def _golden_step(g, s):
    return g[f"hf_greedy_logits_s{s}_top_i"].astype(np.int64), g[f"hf_greedy_logits_s{s}_top_v"]


def _processed_top2_gap(ti, tv, hist, V, eos, step):
    """Processed (rep 1.1, ngram 3, min_new 8) top-2 gap of the golden raw logits, computed on the
    golden top-64 (every other logit set far below): rows whose gap is certain."""
    row = torch.full((ti.shape[0], V), -1e30, dtype=torch.float64)
    row.scatter_(1, torch.from_numpy(ti), torch.from_numpy(tv.astype(np.float64)))
    sc = search._processors(row, torch.from_numpy(hist.astype(np.int64)), 1.1, 3, 8, eos)
    top = torch.topk(sc, 2, dim=-1).values
    return (top[:, 0] - top[:, 1]).numpy(), sc.argmax(-1).numpy()


def test_bf16_teacher_forced_all_steps(device):
    """bf16 decoder fed the reference's fp32 prefix and, at each step, the reference's own greedy
    token (fp32 wte rows): every step's raw logits within BF16_LOGIT_TOL of the reference's, and
    the processed argmax identical wherever the reference's processed top-2 gap > the tolerance."""
    meta, g, va, ga, sd, frames, enc, pre, dec = _models("bf16", device)
    B, V, eos = meta["B"], ga.vocab, ga.eos_token_id
    steps = meta["hf_greedy_logit_steps"]
    assert steps == 24
    ids = g["hf_greedy_ids"]
    wte32 = torch.from_numpy(sd["decoder.model.transformer.wte.weight"]).to(device)
    lm = HipGPT2LMHead(dec, ga, _WTE(dec.wte))
    x = torch.from_numpy(g["inputs_embeds"].copy()).to(device)    # [B, 5, E] fp32 (prefix + BOS)
    out = lm(inputs_embeds=x, use_cache=True)
    errs, checked, flips = [], 0, []
    for s in range(steps):
        lg = out.logits[:, -1, :].double()
        ti, tv = _golden_step(g, s)
        got = torch.gather(lg, 1, torch.from_numpy(ti).to(device)).cpu().numpy()
        errs.append(float(np.abs(got - tv).max()))
        gap, gold_arg = _processed_top2_gap(ti, tv, ids[:, :s], V, eos, s)
        assert np.array_equal(gold_arg, ids[:, s]), "golden top-64 does not reproduce the golden token"
        mine = search._processors(lg, torch.from_numpy(ids[:, :s].astype(np.int64)).to(device), 1.1, 3, 8, eos)
        mine = mine.argmax(-1).cpu().numpy()
        sure = gap > BF16_LOGIT_TOL
        checked += int(sure.sum())
        flips += [(s, int(b)) for b in np.nonzero(sure & (mine != ids[:, s]))[0]]
        if s + 1 < steps:
            emb = wte32[torch.from_numpy(ids[:, s].astype(np.int64)).to(device)].unsqueeze(1)
            out = lm(inputs_embeds=emb, past_key_values=out.past_key_values, use_cache=True)
    print(f"bf16 teacher-forced: max |dlogit| per step {np.round(errs, 4).tolist()}; "
          f"{checked} of {B * steps} tokens certain, flips {flips}")
    assert max(errs) < BF16_LOGIT_TOL, errs
    assert not flips, flips
    assert checked >= 0.75 * B * steps


def _free_running(device):
    meta, g, va, ga, sd, frames, enc, pre, dec = _models("bf16", device)
    _, prefix = enc.encode(torch.from_numpy(frames).to(device), pre)
    ids = dec.generate_ids(prefix, [ga.bos_token_id], _hf_cfg(ga)).cpu().numpy()
    return ids, g["hf_greedy_ids"]


def token_agreement(got, ref):
    """(mean leading-token agreement per caption, position-wise agreement) of [B, L] id arrays."""
    lead = []
    for a, b in zip(got, ref):
        n = 0
        while n < len(b) and n < len(a) and a[n] == b[n]:
            n += 1
        lead.append(n / len(b))
    return float(np.mean(lead)), float((got[:, :ref.shape[1]] == ref).mean())


def test_bf16_free_running_agreement(device):
    """The benchmark's bf16 path end to end (encode + fused greedy decode graph) against the
    reference's HF-greedy captions of the same 8 videos.  The floor is argued, not measured: with
    every processed score within BF16_E2E_TOL of the reference's, no token can differ before the
    first step whose reference processed top-2 gap is <= 2 x BF16_E2E_TOL (gaps from the golden
    all-step logits); each caption's leading agreement must reach that step, and every divergence
    must start at such a near-tie."""
    meta, g, va, ga, sd, frames, enc, pre, dec = _models("bf16", device)
    got, ref = _free_running(device)
    B, L, eos = ref.shape[0], ref.shape[1], ga.eos_token_id
    gaps = np.stack([_processed_top2_gap(*_golden_step(g, s), ref[:, :s], ga.vocab, eos, s)[0] for s in range(L)], 1)
    lead, pos = token_agreement(got, ref)
    for b in range(B):
        first_div = next((s for s in range(L) if got[b, s] != ref[b, s]), L)
        guard = next((s for s in range(L) if gaps[b, s] <= 2 * BF16_E2E_TOL), L)
        assert first_div >= guard, (b, first_div, guard, gaps[b, :first_div + 1])
        if first_div < L:
            assert gaps[b, first_div] <= 2 * BF16_E2E_TOL, (b, first_div, gaps[b, first_div])
    print(f"bf16 free-running: leading-token agreement {lead:.3f}, position-wise {pos:.3f}")


@pytest.mark.parametrize("prec", ["bf16", "fp32"])
def test_lm_head_processor_epilogue_every_step(device, prec):
    """The lm_head epilogue (RepetitionPenalty -> NoRepeatNGram -> MinNewTokens -> argmax partials)
    + finalize, all 24 steps: the token each step emits equals torch's processors + argmax
    applied to the raw logits the same kernel wrote (integer-exact)."""
    meta, g, va, ga, sd, frames, enc, pre, dec = _models(prec, device)
    B, eos = meta["B"], ga.eos_token_id
    prefix = torch.from_numpy(g["inputs_embeds"][:, :4].copy()).to(device)
    logits = torch.empty(24, B, ga.vocab, device=device)
    ids = dec.generate_ids(prefix, [ga.bos_token_id], _hf_cfg(ga, graph=False), logits_out=logits)
    ids64 = ids.long()
    fin = torch.zeros(B, dtype=torch.bool, device=device)
    for s in range(24):
        sc = search._processors(logits[s], ids64[:, :s], 1.1, 3, 8, eos)
        exp = torch.where(fin, torch.full_like(ids64[:, s], eos), sc.argmax(-1))
        assert torch.equal(exp, ids64[:, s]), (s, exp, ids64[:, s])
        fin |= ids64[:, s] == eos


@pytest.mark.parametrize("lanes,group,egroup,dcus", [(2, 1, 1, 0), (1, 2, 1, 0), (2, 2, 1, 0), (1, 4, 1, 0),
                                                     (2, 2, 2, 0), (1, 4, 2, 0), (2, 2, 2, 96)])
def test_bf16_pipeline_bit_identical_to_serial(device, lanes, group, egroup, dcus):
    """The bench schedule (vcap/pipeline.py: CU-masked encode stream, decode lanes with capped
    grids, own workspaces / graphs, optionally `group` batches decoded as one decode of group*8
    rows and `egroup` batches encoded as one encode of egroup*8 videos, and the decode lanes masked
    to the first `dcus` CUs as the headline runs them) gives bit-identical bf16 encodes and ids to a
    serial bf16 encode + generate_ids of one batch on the default stream (deterministic,
    M-independent split-K; mask-independent plans; row-independent kernels)."""
    from vcap.pipeline import CaptionPipeline
    meta, g, va, ga, sd, frames, enc, pre, dec = _models("bf16", device)
    video = torch.from_numpy(frames).to(device)
    emb_serial, pre_serial = enc.encode(video, pre)
    ids_serial = dec.generate_ids(pre_serial, [ga.bos_token_id], _hf_cfg(ga)).clone()
    cfg = _hf_cfg(ga, max_blocks=128)
    pipe = CaptionPipeline(enc, pre, dec, cfg, video.shape[0], [ga.bos_token_id], device, reserve_cus=32,
                           dec_lanes=lanes, dec_group=group, enc_group=egroup, confine_decode=dcus)
    try:
        slots = [pipe.submit(video) for _ in range(5)]
        pipe.synchronize()
        for slot in slots[-3:]:
            assert torch.equal(pipe.result(slot), ids_serial)
            assert torch.equal(pipe.prefix_bufs[slot], pre_serial)
    finally:
        pipe.close()


@pytest.mark.parametrize("group,egroup,dcus", [(2, 2, 0), (4, 2, 0), (2, 2, 160)])
def test_token_exact_pipeline_bit_identical_to_serial(device, group, egroup, dcus):
    """The token-exact leg's schedule - bf16 ViT, fp32 GPT-2 decoder (its mlp c_proj K-split over
    workgroup pairs, the bf16 lm_head screen) - decodes 16- and 32-row groups on two lanes with capped
    grids beside the CU-masked encode, and every batch's ids equal a serial fp32 decode of that batch's
    bf16 prefix: the pair hand-off and the screen are deterministic whatever the grid, lane, group or
    decode CU mask (160 CUs: the token-exact leg's)."""
    from vcap.pipeline import CaptionPipeline
    meta, g, va, ga, sd, frames, enc, pre, _ = _models("bf16", device)
    dec32 = HipGPT2Decoder(sd, ga, "fp32", device)
    video = torch.from_numpy(frames).to(device)
    _, pre_serial = enc.encode(video, pre)
    ids_serial = dec32.generate_ids(pre_serial, [ga.bos_token_id], _hf_cfg(ga)).clone()
    pipe = CaptionPipeline(enc, pre, dec32, _hf_cfg(ga, max_blocks=96), video.shape[0], [ga.bos_token_id], device,
                           reserve_cus=32, dec_lanes=2, dec_group=group, enc_group=egroup, confine_decode=dcus)
    try:
        slots = [pipe.submit(video) for _ in range(2 * group + 1)]
        pipe.synchronize()
        for slot in slots[-group:]:
            assert torch.equal(pipe.result(slot), ids_serial)
    finally:
        pipe.close()


def test_pipelines_reuse_one_stream_set_per_schedule(device):
    """Pipelines with the same schedule reuse one set of streams for the process (vcap/pipeline.py
    _stream_set: fresh streams per pipeline measured serialised, profiles/r04_stream_reuse.txt);
    a second pipeline after the first is closed still gives the serial ids."""
    from vcap.pipeline import CaptionPipeline
    meta, g, va, ga, sd, frames, enc, pre, dec = _models("bf16", device)
    video = torch.from_numpy(frames).to(device)
    _, pre_serial = enc.encode(video, pre)
    ids_serial = dec.generate_ids(pre_serial, [ga.bos_token_id], _hf_cfg(ga)).clone()
    cfg = _hf_cfg(ga, max_blocks=96)
    mk = lambda r: CaptionPipeline(enc, pre, dec, cfg, video.shape[0], [ga.bos_token_id], device,  # noqa: E731
                                   reserve_cus=r, dec_lanes=2, dec_group=1, enc_group=1)
    a = mk(32)
    streams = (a.s_enc, list(a.s_decs))
    a.close()
    b, c = mk(32), mk(0)
    try:
        assert b.s_enc is streams[0] and b.s_decs == streams[1]
        assert c.s_enc is not b.s_enc
        slots = [b.submit(video) for _ in range(3)]
        b.synchronize()
        assert all(torch.equal(b.result(s), ids_serial) for s in slots)
    finally:
        b.close()
        c.close()


# ------------------------------------------------------------------ per-kernel tests at bench shapes

def _rand(shape, seed, scale=1.0, device="cuda"):
    gen = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=gen) * scale).to(device)


M_BENCH = 8 * 16 * 197   # configs[1]: 8 videos x 16 frames x 197 tokens = 25216 rows


@pytest.mark.parametrize("role,N_,K,act", [("qkv", 2304, 768, 0), ("fc1", 3072, 768, 1)])
def test_gemm_bench_shape_bf16_out(device, role, N_, K, act):
    """QKV (bias) and fc1 (bias + tanh-GELU) at M = 25216 under the auto policy (256x256 rounds +
    128x128 remainder), bf16 out, against fp32 torch on the same bf16 operands."""
    N.check(N.lib().vcap_set_gemm_policy(0), "policy")
    A = _rand((M_BENCH, K), 31).to(torch.bfloat16)
    W = _rand((N_, K), 32, 0.03).to(torch.bfloat16)
    b = _rand((N_,), 33, 0.1)
    out = torch.empty(M_BENCH, N_, dtype=torch.bfloat16, device=device)
    N.check(N.lib().vcap_gemm(N.DT_BF16, N.DT_BF16, A.data_ptr(), K, W.data_ptr(), K, out.data_ptr(), N_, M_BENCH, N_,
                              K, b.data_ptr(), act, None, 0, 0, 0, 0, 0, 0, _stream()), role)
    ref = A.float() @ W.float().t() + b
    if act:
        ref = F.gelu(ref, approximate="tanh")
    # one bf16 rounding of an fp32-accumulated value: <= 2^-8 relative (+ summation order)
    torch.testing.assert_close(out.float(), ref, rtol=8e-3, atol=2e-3)


@pytest.mark.parametrize("N_,K", [(2304, 768), (768, 3072)])
def test_gemm_tile128_and_tile256_bitwise_equal(device, N_, K):
    """The 128x128 and 256x256 kernels issue the same MFMA chain per output (K ascending, weight
    fragment as operand A): the dispatcher's whole-round / remainder split, which depends on the
    stream's CU mask, therefore cannot change a single bit of the encode."""
    M = 4096
    A = _rand((M, K), 34).to(torch.bfloat16)
    W = _rand((N_, K), 35, 0.03).to(torch.bfloat16)
    b = _rand((N_,), 36, 0.1)
    outs = []
    for pol in (1, 2):
        N.check(N.lib().vcap_set_gemm_policy(pol), "policy")
        x = _rand((M, N_), 37)
        N.check(N.lib().vcap_gemm(N.DT_BF16, N.DT_F32, A.data_ptr(), K, W.data_ptr(), K, x.data_ptr(), N_, M, N_, K,
                                  b.data_ptr(), 0, x.data_ptr(), N_, 1, 0, 0, 0, 0, _stream()), "gemm")
        outs.append(x)
    N.check(N.lib().vcap_set_gemm_policy(0), "policy")
    assert torch.equal(outs[0], outs[1])


def test_vit_attention_bench_shape_bf16(device):
    """128 frames x 12 heads x 197 tokens (configs[1]) against fp32 SDPA on the same bf16 q/k/v."""
    BT, Ntok, H = 128, 197, 12
    D = H * 64
    qkv = _rand((BT * Ntok, 3 * D), 38, 1.5).to(torch.bfloat16)
    out = torch.empty(BT * Ntok, D, dtype=torch.bfloat16, device=device)
    N.check(N.lib().vcap_vit_attention(N.DT_BF16, qkv.data_ptr(), out.data_ptr(), BT, Ntok, H, _stream()), "attn")
    q, k, v = qkv.float().reshape(BT, Ntok, 3, H, 64).permute(2, 0, 3, 1, 4).unbind(0)
    ref = F.scaled_dot_product_attention(q, k, v).transpose(1, 2).reshape(BT * Ntok, D)
    torch.testing.assert_close(out.float(), ref, rtol=2e-2, atol=2e-2)


def _decode_attn_ref(q, kc, vc, pt, maxp, H, S_new, past):
    M = q.shape[0]
    out = torch.empty(M, H * 64, device=q.device)
    for m in range(M):
        seq, qpos = m // S_new, past + m % S_new
        pos = torch.arange(qpos + 1, device=q.device)
        pages = pt[seq, pos // 16].long() if pt is not None else seq * maxp + pos // 16
        kk = kc.float()[pages, :, pos % 16]   # [ctx, H, 64]
        vv = vc.float()[pages, :, pos % 16]
        qq = q.float()[m].reshape(H, 64)
        att = torch.einsum("hd,chd->hc", qq, kk) / 8.0
        out[m] = torch.einsum("hc,chd->hd", att.softmax(-1), vv).reshape(-1)
    return out


@pytest.mark.parametrize("prec,S_new,past,paged", [("bf16", 1, 28, False), ("bf16", 5, 0, False),
                                                   ("bf16", 1, 63, False), ("bf16", 1, 70, True),
                                                   ("fp32", 1, 28, True), ("fp32", 5, 0, True)])
def test_decode_attention(device, prec, S_new, past, paged):
    """vcap_decode_attention: the bf16 contiguous-page fast path (decode_attention_c64, context
    <= 64: every configs[1] step) and the page-table kernel, against an fp32 torch reference."""
    tdt = torch.bfloat16 if prec == "bf16" else torch.float32
    dt = N.DT_BF16 if prec == "bf16" else N.DT_F32
    seqs, H = 8, 12
    ctx = past + S_new
    maxp = (ctx + 15) // 16 + 1
    M = seqs * S_new
    q = _rand((M, H * 64), 40).to(tdt)
    kc = _rand((seqs * maxp, H, 16, 64), 41).to(tdt)
    vc = _rand((seqs * maxp, H, 16, 64), 42).to(tdt)
    pt = None
    if paged:   # a shuffled page table
        perm = torch.randperm(seqs * maxp, generator=torch.Generator().manual_seed(43)).int()
        pt = perm.reshape(seqs, maxp).to(device)
    out = torch.empty(M, H * 64, dtype=tdt, device=device)
    N.check(N.lib().vcap_decode_attention(dt, q.data_ptr(), kc.data_ptr(), vc.data_ptr(), N.ptr(pt), maxp,
                                          out.data_ptr(), M, H, S_new, past, _stream()), "decode attention")
    ref = _decode_attn_ref(q, kc, vc, pt, maxp, H, S_new, past)
    tol = 1e-2 if prec == "bf16" else 1e-5
    torch.testing.assert_close(out.float(), ref, rtol=tol, atol=tol)


@pytest.mark.parametrize("S_new,past", [(1, 0), (1, 28), (1, 63), (5, 59)])
def test_decode_attention_kernels_agree(device, S_new, past):
    """The two decode attention kernel templates compute the same bits: bf16 with an identity page table
    (the general kernel) against the NULL table (the <= 64 kernel) on the same pools."""
    seqs, H = 3, 2
    maxp = (past + S_new + 15) // 16 + 1
    M = seqs * S_new
    q = _rand((M, H * 64), 50).to(torch.bfloat16)
    kc = _rand((seqs * maxp, H, 16, 64), 51).to(torch.bfloat16)
    vc = _rand((seqs * maxp, H, 16, 64), 52).to(torch.bfloat16)
    outs = []
    for pt in (torch.arange(seqs * maxp, dtype=torch.int32, device=device), None):
        out = torch.zeros(M, H * 64, dtype=torch.bfloat16, device=device)
        N.check(N.lib().vcap_decode_attention(N.DT_BF16, q.data_ptr(), kc.data_ptr(), vc.data_ptr(), N.ptr(pt), maxp,
                                              out.data_ptr(), M, H, S_new, past, _stream()), "decode attention")
        outs.append(out.view(torch.int16))
    assert torch.equal(outs[0], outs[1])
