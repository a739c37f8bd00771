"""CPU checks of the teacher-forced scoring oracle (tests/score_cases.py) against the reference's own
output (tests/golden/score_*.npz, written by tests/golden/make_score_goldens.py): they pin the mask and
position semantics of vcap_gpt2_score before any GPU code is judged.  Bars: 1e-4 on logits and losses,
as test_cpu_oracle.py."""
import json

import numpy as np
import torch

import decoder_shapes as DS
import score_cases as SC
from helpers import GOLDEN, golden
from oracle import vcap_oracle as O
from vcap import _native as N
from vcap import configs, prng, weights

TOL = 1e-4


def _sd64(sd):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).double() for k, v in sd.items()}


def _decoder_forward(sd, ga, video_emb, input_ids, attention_mask, labels):
    """GPT2TextDecoder.forward on the oracle: -> (logits [B, P + L, V], loss)."""
    ids = torch.as_tensor(input_ids).long()
    B = video_emb.shape[0]
    prefix = O.mapper(sd, video_emb.double(), ga.n_embd, SC.PREFIX_LEN)
    x = torch.cat([prefix, sd[DS.WTE][ids]], dim=1)
    km = torch.cat([torch.ones(B, SC.PREFIX_LEN, dtype=torch.uint8), torch.as_tensor(attention_mask).to(torch.uint8)], 1)
    with torch.no_grad():
        logits = SC.masked_forward(sd, ga, x, km)
    _, nll, cnt = SC.target_logprobs(logits, SC.shift_labels(torch.as_tensor(labels)))
    return logits, nll / cnt


def test_null_mask_is_emulated_forward():
    c = SC.Case("null", 128, 1009, 3, 7)
    ar, x = SC.arch(c.E, c.V), SC.embeds(c).double()
    for rounded, rnd in ((False, DS._ident), (True, DS.bf16_rne)):
        sd = SC.sd64(c.E, c.V, 1.0, rounded)
        with torch.no_grad():
            want = DS.emulated_forward(sd, ar, x, O.KVCache(ar.n_layer), rnd)
            assert torch.equal(SC.masked_forward(sd, ar, x, None, rnd), want)
            assert torch.equal(SC.masked_forward(sd, ar, x, torch.ones(c.B, c.S), rnd), want)


def test_mask_hides_keys_only_from_later_queries():
    """Hiding key j leaves every row before j unchanged and changes rows after it."""
    c = SC.Case("hide", 128, 1009, 2, 12)
    ar, sd, x = SC.arch(c.E, c.V), SC.sd64(c.E, c.V), SC.embeds(c).double()
    m = torch.ones(c.B, c.S)
    m[:, 5] = 0
    with torch.no_grad():
        a, b = SC.masked_forward(sd, ar, x, None), SC.masked_forward(sd, ar, x, m)
    assert torch.equal(a[:, :5], b[:, :5])
    assert bool(((a[:, 5:] - b[:, 5:]).abs().amax(dim=-1) > 0).all())


def test_reference_forward_tiny():
    meta, arr = golden("score_tiny")
    va, ga = configs.vit_arch(meta["vit"]), configs.gpt2_arch(meta["gpt2"])
    sd = _sd64(weights.synthetic_state_dict(meta["weights_seed"], va, ga))
    emb = torch.from_numpy(arr["video_emb"])
    logits, loss = _decoder_forward(sd, ga, emb, arr["input_ids"], arr["attention_mask"], arr["labels"])
    err = float((logits - torch.from_numpy(arr["logits"]).double()).abs().max())
    print(f"score_tiny: max |logit - reference| {err:.3e}, loss {loss:.6f} vs {meta['loss']:.6f}")
    assert err < TOL
    assert abs(loss - meta["loss"]) < TOL
    # attention_mask = None: input_ids != pad
    dmask = arr["input_ids"] != meta["pad_id"]
    _, loss_d = _decoder_forward(sd, ga, emb, arr["input_ids"], dmask, arr["labels"])
    assert abs(loss_d - meta["loss_default_mask"]) < TOL


def test_reference_compute_loss_tiny():
    """compute_loss' quirks: the mask caption_ids[:, :-1] != pad hides the leading BOS (bos = pad), and
    the labels at pad positions are scored."""
    meta, arr = golden("score_tiny")
    va, ga = configs.vit_arch(meta["vit"]), configs.gpt2_arch(meta["gpt2"])
    sd32 = weights.synthetic_state_dict(meta["weights_seed"], va, ga)
    video = torch.from_numpy(prng.imagenet_frames(meta["frames_seed"], (meta["B"], meta["T"], 3, va.image, va.image)))
    with torch.no_grad():
        emb = O.encoder(sd32, va, video)
    assert float((emb - torch.from_numpy(arr["video_emb"])).abs().max()) < TOL
    cap = torch.from_numpy(arr["caption_ids"]).long()
    inp, labels = cap[:, :-1], cap[:, 1:]
    assert bool((inp[:, 0] == meta["pad_id"]).all())       # the BOS the mask hides
    _, loss = _decoder_forward(_sd64(sd32), ga, emb, inp, inp != meta["pad_id"], labels)
    print(f"compute_loss {loss:.6f} vs {meta['compute_loss']:.6f}")
    assert abs(loss - meta["compute_loss"]) < TOL


def test_reference_forward_gpt2():
    meta, arr = golden("score_gpt2")
    va, ga = configs.vit_arch(meta["vit"]), configs.gpt2_arch(meta["gpt2"])
    sd = _sd64(weights.synthetic_gpt2(meta["weights_seed"], ga))
    logits, loss = _decoder_forward(sd, ga, torch.from_numpy(arr["video_emb"]), arr["input_ids"],
                                    arr["attention_mask"], arr["labels"])
    top = logits.gather(2, torch.from_numpy(arr["logits_top_i"]).long())
    assert float((top - torch.from_numpy(arr["logits_top_v"]).double()).abs().max()) < TOL
    assert float((logits.sum(-1) - torch.from_numpy(arr["logits_sum"])).abs().max()) < 50257 * TOL
    tgt = torch.from_numpy(arr["targets"])
    assert torch.equal(tgt.long(), SC.shift_labels(torch.from_numpy(arr["labels"])))
    lp, _, _ = SC.target_logprobs(logits, tgt)
    assert float((lp - torch.from_numpy(arr["target_logprob"])).abs().max()) < TOL
    assert abs(loss - meta["loss"]) < TOL


def test_goldens_are_small():
    for f in GOLDEN.glob("score_*"):
        assert f.stat().st_size <= 512 * 1024, f
    assert json.loads((GOLDEN / "score_tiny.json").read_text())["gpt2"] == "gpt2_tiny_test"


def test_binding_has_score_symbols():
    header = (GOLDEN.parents[1] / "include" / "vcap.h").read_text()
    for name in ("vcap_gpt2_score_workspace_bytes", "vcap_gpt2_score"):
        assert name in N.SIGNATURES and name + "(" in header
    assert "#define VCAP_ABI_VERSION 16" in header and N.ABI_VERSION == 16
