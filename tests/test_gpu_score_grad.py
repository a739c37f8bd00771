"""vcap_gpt2_score_backward on the GPU: the gradient of the teacher-forced target log-probs with respect
to inputs_embeds (csrc/runtime_gpt2_grad.hip, csrc/score_backward.hip), HipGPT2Decoder.score_backward and
the autograd surface of vcap/train.py, against the fp64 autograd oracle of tests/score_grad_cases.py.

Tolerances come from CPU runs alone (score_grad_cases.tolerance), never from the device's output:
  fp32  err <= 10 * err(torch CPU float32 autograd of the same case)
  bf16  err <= 3 * err(the bf16-emulated CPU run of the same case)
with err(g) = max |g - g64| / max |g64| over the whole [B, S, E] gradient.  Each accuracy test prints its
measured figure and the device / CPU-f32 ratio before it asserts.

Models: the 2-layer sweep models (n_positions 128).  Shapes: one position; 13 positions under no / right /
interior masks; contexts 64 and 65; 70 with a right mask; V = 1024 (whole tiles), 1009 and 50257 (ragged
last tile); every width class; 512 rows = the row limit with S = n_positions."""
import ctypes as C
from functools import lru_cache

import pytest
import torch

import score_cases as SC
import score_grad_cases as G
from vcap import _native as N
from vcap.model import HipGPT2Decoder

pytestmark = pytest.mark.gpu
PRECS = ["fp32", "bf16"]


@lru_cache(maxsize=None)
def decoder(E, V, prec):
    d = HipGPT2Decoder(SC.state_dict(E, V), SC.arch(E, V), prec, "cuda", screen=False)
    d.enable_grad(SC.state_dict(E, V))
    return d


def last_error() -> str:
    return (N.lib().vcap_last_error() or b"").decode()


def abi_backward(dec, x, km=None, tg=None, w=None, ws_bytes=None):
    """One raw vcap_gpt2_score_backward call -> (rc, grad, logprobs, loss[2]); outputs pre-filled with a
    sentinel so that a refused call is seen to have written nothing."""
    dev = dec.device
    B, S, _ = x.shape
    x = x.to(dev, torch.float32).contiguous()
    km = None if km is None else km.to(dev, torch.uint8).contiguous()
    tg = None if tg is None else tg.to(dev, torch.int32).contiguous()
    w = None if w is None else w.to(dev, torch.float32).contiguous()
    grad = torch.full_like(x, 777.0)
    lp = torch.full((B, S), 777.0, device=dev)
    loss = torch.full((2,), 777.0, device=dev)
    need = int(N.lib().vcap_gpt2_score_backward_workspace_bytes(C.byref(dec.desc), C.byref(dec.grad_desc), B, S))
    ws = torch.empty(max(need if ws_bytes is None else ws_bytes, 1), dtype=torch.uint8, device=dev)
    rc = N.lib().vcap_gpt2_score_backward(C.byref(dec.desc), C.byref(dec.grad_desc), x.data_ptr(), B, S, N.ptr(km),
                                          N.ptr(tg), N.ptr(w), grad.data_ptr(), lp.data_ptr(), loss.data_ptr(),
                                          ws.data_ptr(), ws.numel() if ws_bytes is None else ws_bytes,
                                          torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize(dev)
    return rc, grad, lp, loss


def case_inputs(c, wmode="rand"):
    return SC.embeds(c), SC.key_mask(c), G.targets(c), G.weights_w(c, wmode)


def run_case(c, prec, wmode="rand"):
    x, km, tg, w = case_inputs(c, wmode)
    rc, grad, lp, loss = abi_backward(decoder(c.E, c.V, prec), x, km, tg, w)
    assert rc == 0, last_error()
    return grad.cpu(), lp.cpu(), loss.cpu()


# ------------------------------------------------------------------------------------------ 1. accuracy
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("wmode", ["rand", "null"])
@pytest.mark.parametrize("c", G.CASES, ids=lambda c: c.name)
def test_gradient_matches_fp64_autograd(c, wmode, prec):
    grad, _, _ = run_case(c, prec, wmode)
    g64 = G.oracle_grad(c, wmode)
    tol = G.tolerance(c, wmode, prec)
    e = G.err(grad, g64)
    ref = tol / (G.F32_FACTOR if prec == "fp32" else G.BF16_FACTOR)   # the CPU f32 run's / the bf16 emulation's error
    print(f"score_grad {c.name} w={wmode} {prec}: err {e:.3e} tol {tol:.3e} cpu_ref_err {ref:.3e} "
          f"ratio {e / ref:.3f}")
    assert torch.isfinite(grad).all()
    assert 0.0 < tol < 1.0
    assert e <= tol


# ------------------------------------------------------------------------------------ 2. exact contracts
EXACT = [G.MASKS[1], G.MASKS[2], G.SHAPES[3]]   # right, interior, 70 right / edges


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("c", EXACT, ids=lambda c: c.name)
def test_forward_outputs_are_score_bits(c, prec):
    dec = decoder(c.E, c.V, prec)
    x, km, tg, w = case_inputs(c)
    _, lp, loss = run_case(c, prec)
    ref = dec.score(x, km, tg)
    assert torch.equal(lp, ref.logprobs.cpu())
    assert torch.equal(loss, torch.stack([ref.nll_sum, ref.count]).cpu())


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("c", EXACT, ids=lambda c: c.name)
def test_two_calls_same_bits_and_batch_independent(c, prec):
    dec = decoder(c.E, c.V, prec)
    x, km, tg, w = case_inputs(c)
    g1, _, _ = run_case(c, prec)
    g2, _, _ = run_case(c, prec)
    assert torch.equal(g1, g2)
    for b in range(c.B):
        rc, gb, _, _ = abi_backward(dec, x[b:b + 1], None if km is None else km[b:b + 1], tg[b:b + 1], w[b:b + 1])
        assert rc == 0
        assert torch.equal(gb.cpu()[0], g1[b]), f"sequence {b} differs from its own B = 1 call"


@pytest.mark.parametrize("prec", PRECS)
def test_python_chunking_equals_single_sequence_calls(prec):
    c = SC.Case("chunk_9x64", 128, 1009, 9, 64, "interior")   # 576 rows: two chunks (8 + 1 sequences)
    dec = decoder(c.E, c.V, prec)
    x, km, tg, w = case_inputs(c)
    res, grad = dec.score_backward(x, km, tg, w)
    ref = dec.score(x, km, tg)
    assert torch.equal(res.logprobs, ref.logprobs)
    assert torch.equal(res.nll_sum, ref.nll_sum) and torch.equal(res.count, ref.count)
    for b in range(c.B):
        rc, gb, _, _ = abi_backward(dec, x[b:b + 1], km[b:b + 1], tg[b:b + 1], w[b:b + 1])
        assert rc == 0
        assert torch.equal(gb[0], grad[b])


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("c", EXACT, ids=lambda c: c.name)
def test_doubling_the_weights_doubles_every_bit(c, prec):
    dec = decoder(c.E, c.V, prec)
    x, km, tg, w = case_inputs(c)
    _, g1, _, _ = abi_backward(dec, x, km, tg, w)
    _, g2, _, _ = abi_backward(dec, x, km, tg, 2.0 * w)
    assert torch.equal(g2, 2.0 * g1)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("wmode", ["rand", "null"])
@pytest.mark.parametrize("c", EXACT, ids=lambda c: c.name)
def test_exact_zero_positions(c, wmode, prec):
    grad, _, _ = run_case(c, prec, wmode)
    z = G.zero_positions(c)
    assert bool(z.any())
    assert bool(G.is_plus_zero(grad[z]).all())
    assert torch.isfinite(grad).all()


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("c", G.IGNORED, ids=lambda c: c.name)
def test_all_targets_ignored(c, prec):
    grad, lp, loss = run_case(c, prec)
    assert bool(G.is_plus_zero(grad).all())
    assert bool((lp == 0).all())
    assert loss.tolist() == [0.0, 0.0]


# ------------------------------------------------------------------------------------------ 3. refusals
def test_device_refusals_launch_nothing():
    dec = decoder(128, 1009, "fp32")
    E = 128
    tg = torch.zeros(1, 513, dtype=torch.long)
    rc, g, lp, loss = abi_backward(dec, torch.zeros(1, 513, E), None, tg)     # 513 rows
    assert rc == N.E_UNSUPPORTED and "vcap_gpt2_max_rows" in last_error()
    assert bool((g == 777.0).all()) and bool((lp == 777.0).all()) and bool((loss == 777.0).all())
    tg = torch.zeros(1, 129, dtype=torch.long)
    rc, g, lp, loss = abi_backward(dec, torch.zeros(1, 129, E), None, tg)     # S > n_positions = 128
    assert rc == N.E_UNSUPPORTED and "n_positions" in last_error()
    assert bool((g == 777.0).all()) and bool((lp == 777.0).all())
    c = G.MASKS[0]
    x, km, tg, w = case_inputs(c)
    need = int(N.lib().vcap_gpt2_score_backward_workspace_bytes(C.byref(dec.desc), C.byref(dec.grad_desc), c.B, c.S))
    rc, g, lp, loss = abi_backward(dec, x, km, tg, w, ws_bytes=need - 1)
    assert rc == N.E_WORKSPACE and "workspace too small" in last_error()
    assert bool((g == 777.0).all()) and bool((lp == 777.0).all()) and bool((loss == 777.0).all())


@pytest.mark.parametrize("prec", PRECS)
def test_hidden_first_key_poisons_its_sequence_only(prec):
    c = G.MASKS[2]
    dec = decoder(c.E, c.V, prec)
    x, km, tg, w = case_inputs(c)
    _, good, _, _ = abi_backward(dec, x, km, tg, w)
    bad = km.clone()
    bad[1, 0] = 0
    rc, g, lp, _ = abi_backward(dec, x, bad, tg, w)
    assert rc == 0
    assert bool(torch.isnan(g[1]).all()) and bool(torch.isnan(lp[1]).all())
    assert torch.equal(g[0], good[0]) and torch.equal(g[2], good[2])


# -------------------------------------------------------------------------------- 4. existing behaviour
@pytest.mark.parametrize("prec", PRECS)
def test_score_and_generate_unchanged_after_a_backward(prec):
    from vcap.model import GenConfig
    c = G.MASKS[2]
    sd, ar = SC.state_dict(c.E, c.V), SC.arch(c.E, c.V)
    dec = HipGPT2Decoder(sd, ar, prec, "cuda", screen=False)
    x, km, tg, w = case_inputs(c)
    cfg = GenConfig(12, 0, 3, 1.1, ar.eos_token_id, ar.eos_token_id, True)
    prefix = x[:, :4].cuda().contiguous()
    s0 = dec.score(x, km, tg, want_logits=True)
    ids0 = dec.generate_ids(prefix, [ar.bos_token_id], cfg).clone()
    dec.enable_grad(sd)
    dec.score_backward(x, km, tg, w)
    s1 = dec.score(x, km, tg, want_logits=True)
    ids1 = dec.generate_ids(prefix, [ar.bos_token_id], cfg)
    assert torch.equal(s0.logits, s1.logits) and torch.equal(s0.logprobs, s1.logprobs)
    assert torch.equal(s0.nll_sum, s1.nll_sum)
    assert torch.equal(ids0, ids1)


# ------------------------------------------------------------------------------------ 5. autograd wiring
WIRE = SC.Case("wiring", 128, 1009, 3, 12)   # 3 clips, prefix 4 + captions of 9 ids (8 inputs)
VIDEO_DIM = 256


def wiring_batch():
    """(video_emb [3, 256] f32, caption_ids [3, 9], pad_id): <bos> ... <eos>, bos = eos = pad = V - 1 (so the
    leading BOS is a hidden key, as with GPT-2), the last caption right-padded by two."""
    g = torch.Generator().manual_seed(2024)
    emb = torch.randn(WIRE.B, VIDEO_DIM, generator=g, dtype=torch.float32)
    pad = WIRE.V - 1
    ids = torch.randint(0, WIRE.V - 1, (WIRE.B, 9), generator=g)
    ids[:, 0] = pad
    ids[:, -1] = pad
    ids[2, -3:] = pad
    return emb, ids, pad


def linear_from(sd, dtype):
    w = torch.from_numpy(sd["decoder.mapper.0.weight"].copy())
    lin = torch.nn.Linear(w.shape[1], w.shape[0]).to(dtype)
    with torch.no_grad():
        lin.weight.copy_(w)
        lin.bias.copy_(torch.from_numpy(sd["decoder.mapper.0.bias"].copy()))
    return lin


def replica_inputs(lin64, emb, ids, pad):
    """The fp64 replica's (inputs_embeds with the Linear's graph, key mask, shifted targets)."""
    sd = SC.sd64(WIRE.E, WIRE.V)
    inp, labels = ids[:, :-1], ids[:, 1:]
    prefix = lin64(emb.double()).reshape(WIRE.B, SC.PREFIX_LEN, WIRE.E)
    x = torch.cat([prefix, sd[SC.DS.WTE][inp]], dim=1)
    km = torch.cat([torch.ones(WIRE.B, SC.PREFIX_LEN, dtype=torch.uint8), (inp != pad).to(torch.uint8)], dim=1)
    return x, km, SC.shift_labels(labels)


def replica_loss(lin64, emb, ids, pad):
    x, km, tg = replica_inputs(lin64, emb, ids, pad)
    logits = SC.masked_forward(SC.sd64(WIRE.E, WIRE.V), SC.arch(WIRE.E, WIRE.V), x, km)
    return G._objective(logits, tg, None) / int((tg >= 0).sum())


@lru_cache(maxsize=None)
def text_decoder(prec):
    from vcap.caption import HipTextDecoder
    sd = SC.state_dict(WIRE.E, WIRE.V)
    dec = HipTextDecoder(sd, SC.arch(WIRE.E, WIRE.V), prec, "cuda")
    dec.hip.enable_grad(sd)
    return dec


@pytest.mark.parametrize("prec", PRECS)
def test_lm_loss_backward_reaches_the_mapper(prec):
    from vcap import train as T
    dec = text_decoder(prec)
    sd = SC.state_dict(WIRE.E, WIRE.V)
    emb, ids, pad = wiring_batch()
    lin = linear_from(sd, torch.float32).cuda()
    loss = T.compute_loss(dec, emb, ids, pad, lin)
    assert loss.requires_grad
    loss.backward()
    lin64 = linear_from(sd, torch.float64)
    loss64 = replica_loss(lin64, emb, ids, pad)
    loss64.backward()
    # the case's tolerance: the embedding-gradient bound of these very inputs, from the CPU runs
    x, km, tg = replica_inputs(lin64, emb, ids, pad)
    w = torch.full(tg.shape, -1.0 / int((tg >= 0).sum()))
    g64 = G.grad_of(WIRE, "", "fp64", x.detach(), km, tg, w)
    kind, factor = ("f32", G.F32_FACTOR) if prec == "fp32" else ("bf16", G.BF16_FACTOR)
    tol = factor * G.err(G.grad_of(WIRE, "", kind, x.detach(), km, tg, w), g64) * VIDEO_DIM
    e = G.err(lin.weight.grad.cpu(), lin64.weight.grad)
    eb = G.err(lin.bias.grad.cpu(), lin64.bias.grad)
    print(f"score_grad wiring {prec}: loss {float(loss):.6f} vs {float(loss64):.6f}, weight.grad err {e:.3e}, "
          f"bias.grad err {eb:.3e}, tol {tol:.3e}")
    assert tol > 0.0
    assert e <= tol and eb <= tol


@pytest.mark.parametrize("prec", PRECS)
def test_mapper_trainer_lowers_the_loss_and_loads_back(prec):
    from vcap import train as T
    dec = text_decoder(prec)
    sd = SC.state_dict(WIRE.E, WIRE.V)
    emb, ids, pad = wiring_batch()
    before = dec.prefix_embeds(emb.cuda()).clone()
    tr = T.MapperTrainer(dec, sd, pad_id=pad, dropout=0.0)
    first = tr.evaluate(emb, ids)
    for _ in range(30):
        tr.step(emb, ids)
    last = tr.evaluate(emb, ids)
    # the CPU fp64 replica of the same loop
    lin64 = linear_from(sd, torch.float64)
    opt = torch.optim.AdamW(lin64.parameters(), lr=3e-4, weight_decay=0.01)
    first64 = float(replica_loss(lin64, emb, ids, pad))
    for _ in range(30):
        opt.zero_grad()
        replica_loss(lin64, emb, ids, pad).backward()
        opt.step()
    last64 = float(replica_loss(lin64, emb, ids, pad))
    print(f"score_grad trainer {prec}: device {first:.4f} -> {last:.4f}, fp64 replica {first64:.4f} -> {last64:.4f}")
    assert first64 - last64 > 0
    assert first - last >= 0.5 * (first64 - last64)
    # the trained weights in the live device mapper: prefix_embeds is the trained Linear's output
    try:
        tr.load_mapper()
        got = dec.prefix_embeds(emb.cuda())
        tr.mapper.eval()
        with torch.no_grad():
            want = tr.mapper(emb.cuda()).reshape(got.shape)
            lin = tr.mapper[0]
            bound = VIDEO_DIM * 2.0 ** -23 * (emb.cuda().abs() @ lin.weight.abs().t() + lin.bias.abs())
        assert bool(((got - want).abs() <= bound.reshape(got.shape)).all())
        assert float((got - before).abs().max()) > 0
    finally:
        T.load_mapper(dec, {k: torch.from_numpy(sd[k].copy()) for k in (T.MAPPER_W, T.MAPPER_B)})
