"""Ragged prompts on the device: one decode for rows with different prompts (vcap_gpt2_generate_ragged /
_sample_ragged / _beam_search_ragged).  The specification is per row - row b gives what the uniform entry
point gives at B = 1 with prefix row b and prompt b - so the checks are the sweep's fp64 oracle applied
row by row (A) and bit equality with the uniform path (B .. E), on the 2-layer sweep decoders and the case
table of tests/ragged_cases.py; F is the engine's merged S1 + S2 decode."""
import numpy as np
import pytest
import torch

import decoder_shapes as S
import ragged_cases as R
from test_gpu_decoder_shapes import _cfg, _check_logits_and_tokens, _run
from vcap import _native as N
from vcap import search
from vcap.model import GenConfig, HipGPT2Decoder

pytestmark = pytest.mark.gpu
CASES = [(E, prec) for E in R.WIDTHS for prec in R.PRECS]


@pytest.fixture(scope="module")
def decoder(device):
    made = {}

    def get(E, prec):
        if (E, prec) not in made:
            made[(E, prec)] = HipGPT2Decoder(S.state_dict(E), S.arch(E), prec, device)
        return made[(E, prec)]
    return get


@pytest.fixture(scope="module")
def lens_run(decoder, device):
    """The eager LENS run with logits, once per (E, prec): (ids [6, steps], logits [6, steps, V])."""
    done = {}

    def get(E, prec):
        if (E, prec) not in done:
            done[(E, prec)] = _run(decoder(E, prec), R.prefix(E).to(device), R.prompts(E), _cfg(S.arch(E), False),
                                   logits=True)
        return done[(E, prec)]
    return get


@pytest.fixture(scope="module")
def alone_run(decoder, device):
    """Row b of the LENS case through the uniform call at B = 1, once per (E, prec, b)."""
    done = {}

    def get(E, prec, b):
        if (E, prec, b) not in done:
            pre = R.prefix(E)[b:b + 1].contiguous().to(device)
            done[(E, prec, b)] = _run(decoder(E, prec), pre, R.prompts(E)[b], _cfg(S.arch(E), False), logits=True)
        return done[(E, prec, b)]
    return get


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


# ---- A: against the fp64 oracle ------------------------------------------------------------------
@pytest.mark.parametrize("E,prec", CASES)
def test_rows_against_fp64_oracle(decoder, device, lens_run, E, prec):
    ids, lg = lens_run(E, prec)
    pre_cpu, prompts = R.prefix(E), R.prompts(E)
    for b, pr in enumerate(prompts):
        _check_logits_and_tokens(E, prec, pre_cpu[b:b + 1], pr, ids[b:b + 1], lg[b:b + 1],
                                 f"ragged n_embd={E} {prec} row {b} (len {len(pr)})")
    dec, pre, ga = decoder(E, prec), pre_cpu.to(device), S.arch(E)
    gids, _ = _run(dec, pre, prompts, _cfg(ga, True))
    assert np.array_equal(gids, ids), "captured graph"
    cids, _ = _run(dec, pre, prompts, _cfg(ga, False, cap=40))
    assert np.array_equal(cids, ids), "max_blocks 40"


# ---- B: against the uniform path -----------------------------------------------------------------
@pytest.mark.parametrize("E,prec", CASES)
def test_equal_prompts_equal_uniform_call(decoder, device, E, prec):
    """(i) five equal prompts of length 12 through the ragged call == the uniform call at B = 5;
    (iv) B = 1 ragged == uniform."""
    dec, ga = decoder(E, prec), S.arch(E)
    pre, pr = R.prefix(E)[:5].contiguous().to(device), R.prompts(E)[3]
    assert len(pr) == 12
    for B in (5, 1):
        uni = _run(dec, pre[:B].contiguous(), pr, _cfg(ga, False), logits=True)
        dec.force_ragged = True
        try:
            rag = _run(dec, pre[:B].contiguous(), [pr] * B, _cfg(ga, False), logits=True)
        finally:
            dec.force_ragged = False
        assert np.array_equal(rag[0], uni[0]), (B, "ids")
        assert np.array_equal(_bits(rag[1]), _bits(uni[1])), (B, float(np.abs(rag[1] - uni[1]).max()))


@pytest.mark.parametrize("E,prec", CASES)
def test_rows_equal_batch1_uniform_calls(lens_run, alone_run, E, prec):
    """(ii) the LENS run, row by row, == the uniform call at B = 1: ids and raw logits, bit for bit."""
    ids, lg = lens_run(E, prec)
    for b in range(len(R.LENS)):
        ids1, lg1 = alone_run(E, prec, b)
        d = float(np.abs(lg1[0] - lg[b]).max())
        steps = np.flatnonzero((_bits(lg1[0]) != _bits(lg[b])).any(axis=1))
        print(f"\nragged-gpu n_embd={E} {prec} row {b}: max|ragged - batch1| = {d:.3e}"
              f"{'' if not len(steps) else f' first differing step {steps[0]}'}", end="")
        assert np.array_equal(ids1[0], ids[b]), (b, ids1[0], ids[b])
        assert np.array_equal(_bits(lg1[0]), _bits(lg[b])), (b, d)


@pytest.mark.parametrize("prec", R.PRECS)
def test_prefill_on_both_sides_of_64(decoder, device, prec):
    """S0 = 6 and 66 in one packed prefill: the short sequence's rows take the <= 64 attention form and the
    long one's the general form, as their B = 1 calls do (the two forms differ in f32 bits)."""
    E, lens = 128, (2, 62)
    dec, ga = decoder(E, prec), S.arch(E)
    pre, prompts = R.prefix(E)[:2].contiguous().to(device), R.prompts(E, lens)
    ids, lg = _run(dec, pre, prompts, _cfg(ga, False), logits=True)
    for b, pr in enumerate(prompts):
        ids1, lg1 = _run(dec, pre[b:b + 1].contiguous(), pr, _cfg(ga, False), logits=True)
        assert np.array_equal(ids1[0], ids[b]), b
        assert np.array_equal(_bits(lg1[0]), _bits(lg[b])), (b, float(np.abs(lg1[0] - lg[b]).max()))


@pytest.mark.parametrize("E,prec", CASES)
def test_row_permutation_permutes_results(decoder, device, lens_run, E, prec):
    """(iii) permuting the rows permutes ids and logits bitwise."""
    ids, lg = lens_run(E, prec)
    perm = [4, 0, 5, 2, 1, 3]
    pre, prompts = R.prefix(E)[perm].contiguous().to(device), R.prompts(E)
    pids, plg = _run(decoder(E, prec), pre, [prompts[p] for p in perm], _cfg(S.arch(E), False), logits=True)
    assert np.array_equal(pids, ids[perm])
    assert np.array_equal(_bits(plg), _bits(lg[perm]))


@pytest.mark.parametrize("E,prec", CASES)
def test_rows_finishing_at_different_steps(decoder, device, lens_run, E, prec):
    """(v) min_new_tokens = 8 and an EOS id that row 0 reaches first: row 0 finishes and pads while the
    others go on; ids == the B = 1 ids.  (The models' own EOS is never the argmax, so the EOS here is the
    first token row 0 emits at a step >= 8 that it has not emitted before: its path up to there is the
    LENS run's, and it ends there.)"""
    dec = decoder(E, prec)
    row0 = lens_run(E, prec)[0][0]
    t = next(t for t in range(8, S.STEPS - 1) if row0[t] not in row0[:t])
    eos = int(row0[t])
    cfg = GenConfig(S.STEPS, 8, S.NGRAM, S.REP, eos, eos, False)
    pre, prompts = R.prefix(E).to(device), R.prompts(E)
    ids, _ = _run(dec, pre, prompts, cfg)
    for b, pr in enumerate(prompts):
        ids1, _ = _run(dec, pre[b:b + 1].contiguous(), pr, cfg)
        assert np.array_equal(ids1[0], ids[b]), (b, ids1[0], ids[b])
    ends = [int(np.argmax(r == eos)) if (r == eos).any() else -1 for r in ids]
    print(f"\nragged-gpu n_embd={E} {prec}: eos {eos}, first EOS per row {ends}", end="")
    assert ends[0] == t and (ids[0][t:] == eos).all()          # row 0 ended at t and is padded from there
    assert any(e != t for e in ends[1:])                        # ... while another row went on


# ---- C: graph reuse ------------------------------------------------------------------------------
@pytest.mark.parametrize("E,prec", CASES)
def test_one_graph_serves_two_id_sets(decoder, device, lens_run, E, prec):
    """Two id sets with the same offsets through the captured graph, in the order A, B, A: each result
    equals its own eager result (stale ids in the workspace or in a replayed graph would show)."""
    dec, ga = decoder(E, prec), S.arch(E)
    pre, a = R.prefix(E).to(device), R.prompts(E)
    b = [[t if i == 0 else (t + 7) % (S.VOCAB - 1) for i, t in enumerate(p)] for p in a]
    assert [len(p) for p in a] == [len(p) for p in b] and a != b
    eager = {"a": lens_run(E, prec)[0], "b": _run(dec, pre, b, _cfg(ga, False))[0]}
    assert not np.array_equal(eager["a"], eager["b"])
    out = torch.empty(len(a), S.STEPS, dtype=torch.int32, device=device)   # one output address: one graph key
    for name, ids in (("a", a), ("b", b), ("a", a)):
        dec.generate_ids(pre, ids, _cfg(ga, True), out=out)
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy(), eager[name]), name


# ---- D: sampling ---------------------------------------------------------------------------------
SAMPLE_STEPS = 12   # the len-50 row's context crosses 64 at step 10


def _sample(dec, pre, prompts, seed, force=None):
    ga, B = dec.arch, pre.shape[0]
    cfg = GenConfig(SAMPLE_STEPS, 4, S.NGRAM, S.REP, ga.eos_token_id, ga.eos_token_id, False, temperature=0.7,
                    top_k=50, top_p=0.9, seed=seed)
    warped = torch.empty(SAMPLE_STEPS, B, ga.vocab, dtype=torch.float32, device=pre.device)
    ids = dec.generate_ids(pre, prompts, cfg, warped_out=warped, force_ids=force)
    torch.cuda.synchronize()
    return ids.cpu().numpy(), warped.permute(1, 0, 2).contiguous().cpu().numpy()


@pytest.mark.parametrize("E,prec", CASES)
def test_sampling_rows(decoder, device, E, prec):
    dec = decoder(E, prec)
    pre, prompts = R.prefix(E).to(device), R.prompts(E)
    B = len(prompts)
    force = torch.tensor([[(7 * b + 3 * t + 1) % (S.VOCAB - 1) for t in range(SAMPLE_STEPS)] for b in range(B)],
                         dtype=torch.int32, device=device)
    ids, warped = _sample(dec, pre, prompts, 11, force)
    assert np.array_equal(ids, force.cpu().numpy())
    for b, pr in enumerate(prompts):
        ids1, w1 = _sample(dec, pre[b:b + 1].contiguous(), pr, 11, force[b:b + 1].contiguous())
        assert np.array_equal(ids1[0], ids[b])
        assert np.array_equal(_bits(w1[0]), _bits(warped[b])), (b, "warped scores under forced ids")
    # row 0's free draw: the Philox counter is (step, row 0) in both calls
    free, _ = _sample(dec, pre, prompts, 23)
    free1, _ = _sample(dec, pre[:1].contiguous(), prompts[0], 23)
    assert np.array_equal(free1[0], free[0])


# ---- E: beam search ------------------------------------------------------------------------------
def _beam(dec, pre, prompts, nb, L, use_graph):
    kw = dict(num_beams=nb, max_new_tokens=L, min_new_tokens=2, no_repeat_ngram_size=S.NGRAM, repetition_penalty=S.REP,
              eos=dec.arch.eos_token_id, length_penalty=1.0)
    search.beam_search_device(dec, pre, prompts, use_graph=use_graph, **kw)
    _, out, lens = dec._beam_bufs[(pre.shape[0], nb, L)]
    torch.cuda.synchronize()
    return out.cpu().numpy().copy(), lens.cpu().numpy().copy()


@pytest.mark.parametrize("prec", R.PRECS)
@pytest.mark.parametrize("nb", R.BEAM_WIDTHS)
@pytest.mark.parametrize("lens,L", R.BEAM_CASES)
def test_beam_rows_equal_batch1_device_search(decoder, device, lens, L, nb, prec):
    E = 128
    dec = decoder(E, prec)
    prompts = R.prompts(E, lens)
    pre = R.prefix(E)[:len(lens)].contiguous().to(device)
    alone = [_beam(dec, pre[b:b + 1].contiguous(), pr, nb, L, True) for b, pr in enumerate(prompts)]
    for use_graph in (False, True):
        out, ln = _beam(dec, pre, prompts, nb, L, use_graph)
        for b in range(len(lens)):
            assert ln[b] == alone[b][1][0], (use_graph, b, ln, alone[b][1])
            assert np.array_equal(out[b], alone[b][0][0]), (use_graph, b, out[b], alone[b][0][0])


def test_beam_search_any_chunks_and_falls_back(decoder, device):
    """beam_search_any with a prompt per row: 9 rows (two device chunks) give each row's own result; a
    num_beams the device search refuses runs the host search one row at a time."""
    E, dec = 128, decoder(128, "fp32")
    lens = (0, 1, 13, 12, 5, 1, 0, 2, 7)
    prompts = R.prompts(E, lens)
    pre = torch.cat([R.prefix(E), R.prefix(E)[:3] * 0.5]).contiguous().to(device)
    kw = dict(num_beams=2, max_new_tokens=10, min_new_tokens=2, no_repeat_ngram_size=S.NGRAM, repetition_penalty=S.REP,
              eos=dec.arch.eos_token_id, length_penalty=1.0)
    rows = search.beam_search_any(dec, pre, prompts, **kw)
    alone = [search.beam_search_device(dec, pre[b:b + 1].contiguous(), pr, **kw)[0] for b, pr in enumerate(prompts)]
    width = max(len(r) for r in alone)
    assert rows == [r + [kw["eos"]] * (width - len(r)) for r in alone]
    kw9 = dict(kw, num_beams=9, max_new_tokens=6)
    host = [search.beam_search(dec, pre[b:b + 1].contiguous(), prompts[b], **kw9)[0] for b in range(3)]
    width = max(len(r) for r in host)
    assert search.beam_search_any(dec, pre[:3].contiguous(), prompts[:3], **kw9) == \
        [r + [kw["eos"]] * (width - len(r)) for r in host]


# ---- F: engine -----------------------------------------------------------------------------------
_ENG = {}


def _engine(name, device):
    from core.config import InferenceConfig
    from core.engine import InferenceEngine
    from helpers import case
    meta, g, va, ga, sd, frames = case(name)
    surf = meta["surface"]
    if name not in _ENG:
        _ENG.clear()
        cfg = InferenceConfig(vit_name=meta["vit"], gpt2_name=meta["gpt2"], num_frames=meta["T"], precision="fp32",
                              device=str(device), weights_seed=meta["weights_seed"], preset1="precise",
                              preset2="precise", preset3="natural", prompt1="", prompt2=surf["prompt_text"],
                              prompt3=surf["prompt_text"])
        _ENG[name] = InferenceEngine(cfg)
    return _ENG[name], torch.from_numpy(frames).to(device)


@pytest.mark.parametrize("name", ["tiny", "b16_b2"])
def test_engine_merges_s1_s2(device, name):
    from core.inference import preset_to_kwargs
    eng, video = _engine(name, device)
    c, dec = eng.config, eng.model.decoder
    prefix = eng._prefix(video)
    want = [(eng._decode(prefix[b:b + 1], c.prompt1, **preset_to_kwargs(c.preset1)),
             eng._decode(prefix[b:b + 1], c.prompt2, **preset_to_kwargs(c.preset2))) for b in range(prefix.shape[0])]
    calls, inner = [], dec.generate_from_prefix
    dec.generate_from_prefix = lambda *a, **k: (calls.append(a[0].shape[0]), inner(*a, **k))[1]
    try:
        res = eng.infer_video(video[:1])
        assert calls == [2, 1]                                   # S1 + S2 in one call, then S3
        assert (res.candidates.s1, res.candidates.s2) == want[0]
        del calls[:]
        many = eng.infer_videos(video)
        assert len(calls) == 2
    finally:
        del dec.generate_from_prefix
    assert [(r.candidates.s1, r.candidates.s2) for r in many] == want
    singles = [eng.infer_video(video[b:b + 1]) for b in range(video.shape[0])]
    assert [(r.candidates.s1, r.candidates.s2) for r in many] == [(r.candidates.s1, r.candidates.s2) for r in singles]
    assert N.lib().vcap_graph_cache_size() > 0
