"""Ragged prompts without a GPU: the case table's near-tie shares on the fp64 oracle, every refusal of the
_ragged entry points that returns before the first launch (called through the C ABI, the pattern of
test_cpu_abi_refusals.py), the two workspace queries, the Python argument checks, and the engine's
candidate grouping with a fake decoder."""
import ctypes as C

import pytest
import torch

import decoder_shapes as S
import ragged_cases as R
from core.config import InferenceConfig
from core.engine import InferenceEngine
from core.postprocessing.text_cleaner import clean_text
from vcap import _native as N
from vcap.model import split_prompts

ARG, WS, UNSUP = N.E_ARG, N.E_WORKSPACE, N.E_UNSUPPORTED


# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E", R.WIDTHS)
def test_near_tie_shares_under_cap(E):
    """The near-tie shares the GPU token checks rely on (0.7 % / 2.1 - 2.8 % per case, 4.2 % worst row): per
    case and per row <= SKIP_CAP under both rules."""
    shares = R.near_tie_shares(E)
    for b, (s32, s16) in enumerate(shares):
        print(f"\nragged-cpu n_embd={E} row {b} (len {R.LENS[b]}): near-ties fp32 rule {s32:.3f} bf16 rule {s16:.3f}",
              end="")
        assert s32 <= S.SKIP_CAP and s16 <= S.SKIP_CAP, (E, b, s32, s16)
    m32 = sum(s for s, _ in shares) / len(shares)
    m16 = sum(s for _, s in shares) / len(shares)
    print(f"\nragged-cpu n_embd={E} case: fp32 rule {m32:.3f} bf16 rule {m16:.3f}", end="")
    assert m32 <= S.SKIP_CAP and m16 <= S.SKIP_CAP


def test_case_table():
    assert [S.PREFIX_LEN + n for n in R.LENS] == [4, 5, 15, 16, 17, 54]
    pr = R.prompts(128)
    assert [len(p) for p in pr] == list(R.LENS)
    assert pr[0] == [] and pr[1] == [S.arch(128).bos_token_id]
    assert pr[2][:3] == [999, 11 + 10, 48 + 10] and pr[5][1] == 11 + 25
    assert all(0 <= t < S.VOCAB for p in pr for t in p)
    assert tuple(R.prefix(256).shape) == (6, 4, 256)


# ---------------------------------------------------------------------------------------------------
_BUF = C.create_string_buffer(4096)
P = C.addressof(_BUF)                      # a non-null address no refused call reads
_GLAYERS = (N.GPT2Layer * 2)()
BIG = 1 << 30


def _gpt2(**kw):
    f = dict(dtype=N.DT_F32, n_embd=128, n_layer=2, n_head=2, vocab=512, n_positions=64, prefix_len=4, ln_eps=1e-5,
             wte=P, lm_head=P, wpe=P, lnf_g=P, lnf_b=P, layers=_GLAYERS, lm_head_screen=None, screen_bound=0.0)
    f.update(kw)
    return N.GPT2Desc(**f)


def _gen(**kw):
    f = dict(max_new_tokens=8, min_new_tokens=0, no_repeat_ngram_size=0, repetition_penalty=1.0, eos_token_id=511,
             pad_token_id=511, use_graph=0, max_blocks=0)
    f.update(kw)
    return N.GenParams(**f)


def _beam(**kw):
    f = dict(num_beams=3, max_new_tokens=8, min_new_tokens=0, no_repeat_ngram_size=0, repetition_penalty=1.0,
             length_penalty=1.0, early_stopping=0, eos_token_id=511, use_graph=0, max_blocks=0)
    f.update(kw)
    return N.BeamParams(**f)


def _samp(**kw):
    f = dict(temperature=0.7, top_k=50, top_p=0.9, seed=1)
    f.update(kw)
    return N.SampleParams(**f)


def _prompts(lens, ids=None, offsets=None, null_ids=False):
    """-> (Prompts, keep-alives).  ids default to 1s; offsets default to the running sum of lens."""
    if offsets is None:
        offsets = [0]
        for n in lens:
            offsets.append(offsets[-1] + n)
    ids = [1] * max(offsets[-1], 1) if ids is None else ids
    ia, oa = (C.c_int * max(len(ids), 1))(*ids), (C.c_int * len(offsets))(*offsets)
    pr = N.Prompts(ids=None if null_ids else ia, offsets=oa)
    return pr, (ia, oa)


def _call(entry, *, desc=None, d_null=False, gp=None, bp=None, sp=None, lens=(1, 3), B=None, prompts_null=False,
          ws_bytes=BIG, **pkw):
    lib = N.lib()
    d = None if d_null else C.byref(_gpt2(**(desc or {})))
    pr, keep = _prompts(lens, **pkw)
    prp = None if prompts_null else C.byref(pr)
    B = len(lens) if B is None else B
    if entry == "generate":
        rc = lib.vcap_gpt2_generate_ragged(d, C.byref(_gen(**(gp or {}))), P, prp, B, P, None, P, ws_bytes, None)
    elif entry == "sample":
        rc = lib.vcap_gpt2_sample_ragged(d, C.byref(_gen(**(gp or {}))), C.byref(_samp(**(sp or {}))), P, prp, B, P,
                                         None, None, None, P, ws_bytes, None)
    else:
        rc = lib.vcap_gpt2_beam_search_ragged(d, C.byref(_beam(**(bp or {}))), P, prp, B, P, P, P, ws_bytes, None)
    del keep
    return rc, (lib.vcap_last_error() or b"").decode()


# (entry point, what is made bad, code, message)
ROWS = [
    ("generate", dict(d_null=True), ARG, "gpt2 desc is null"),
    ("generate", dict(desc=dict(wte=None)), ARG, "gpt2 wte / lm_head / wpe / ln_f pointer is null"),
    ("generate", dict(prompts_null=True), ARG, "vcap_gpt2_generate_ragged: bad arguments"),
    ("generate", dict(B=0), ARG, "vcap_gpt2_generate_ragged: bad arguments"),
    ("generate", dict(offsets=[1, 2, 3]), ARG, "vcap_gpt2_generate_ragged: bad arguments"),
    ("generate", dict(offsets=[0, 3, 2]), ARG, "vcap_gpt2_generate_ragged: prompt offsets must be non-decreasing"),
    ("generate", dict(lens=(1, 65), desc=dict(n_positions=256)), ARG,
     "vcap_gpt2_generate_ragged: bad arguments (a prompt over 64 ids)"),
    ("generate", dict(lens=(1, 0), desc=dict(prefix_len=0)), UNSUP,
     "vcap_gpt2_generate_ragged: a sequence with no prefix and no prompt"),
    ("generate", dict(lens=(5,) * 60), UNSUP, "sum of (prefix+prompt) rows exceeds vcap_gpt2_max_rows()"),
    ("generate", dict(gp=dict(max_new_tokens=58)), UNSUP, "context exceeds n_positions"),
    ("generate", dict(gp=dict(max_new_tokens=0)), ARG, "max_new_tokens must be > 0"),
    ("generate", dict(gp=dict(max_new_tokens=65)), UNSUP,
     "max_new_tokens > 64 (the lm_head stages the processors' history in LDS)"),
    ("generate", dict(ids=[1, 1, 1, 512]), ARG, "prompt id out of range"),
    ("generate", dict(ids=[1, -1, 1, 1]), ARG, "prompt id out of range"),
    ("generate", dict(null_ids=True), ARG, "vcap_gpt2_generate_ragged: bad arguments"),
    ("generate", dict(ws_bytes=16), WS, "vcap_gpt2_generate_ragged: workspace too small"),
    ("sample", dict(B=0), ARG, "vcap_gpt2_sample_ragged: bad arguments"),
    ("sample", dict(sp=dict(top_k=0)), ARG,
     "vcap_gpt2_sample_ragged: needs temperature > 0, 0 < top_p <= 1, top_k >= 1"),
    ("sample", dict(sp=dict(top_k=129)), UNSUP, "vcap_gpt2_sample_ragged: top_k <= 128 and vocab <= 51200"),
    ("sample", dict(gp=dict(max_new_tokens=65)), UNSUP, "max_new_tokens must be in 1..64"),
    ("sample", dict(lens=(1, 0), desc=dict(prefix_len=0)), ARG,
     "vcap_gpt2_sample_ragged: a sequence with no prefix and no prompt"),
    ("sample", dict(lens=(5,) * 60), UNSUP, "sum of (prefix+prompt) rows exceeds vcap_gpt2_max_rows()"),
    ("sample", dict(gp=dict(max_new_tokens=58)), UNSUP, "context exceeds n_positions"),
    ("sample", dict(ids=[1, 1, 1, 512]), ARG, "prompt id out of range"),
    ("sample", dict(ws_bytes=16), WS, "vcap_gpt2_sample_ragged: workspace too small"),
    ("beam", dict(B=0), ARG, "vcap_gpt2_beam_search_ragged: bad arguments"),
    ("beam", dict(bp=dict(num_beams=9)), UNSUP,
     "vcap_gpt2_beam_search_ragged: needs 2 <= num_beams <= 8, B <= 8, max_new <= 64"),
    ("beam", dict(bp=dict(num_beams=1)), UNSUP,
     "vcap_gpt2_beam_search_ragged: needs 2 <= num_beams <= 8, B <= 8, max_new <= 64"),
    ("beam", dict(lens=(1,) * 9), UNSUP,
     "vcap_gpt2_beam_search_ragged: needs 2 <= num_beams <= 8, B <= 8, max_new <= 64"),
    ("beam", dict(bp=dict(max_new_tokens=65), desc=dict(n_positions=256)), UNSUP,
     "vcap_gpt2_beam_search_ragged: needs 2 <= num_beams <= 8, B <= 8, max_new <= 64"),
    ("beam", dict(lens=(1, 64), bp=dict(max_new_tokens=64), desc=dict(n_positions=256)), UNSUP,
     "vcap_gpt2_beam_search_ragged: needs 2 <= num_beams <= 8, B <= 8, max_new <= 64, longest prefix + prompt + "
     "max_new <= 128"),
    ("beam", dict(lens=(5,) * 8, bp=dict(num_beams=8)), UNSUP, "sum of (prefix+prompt) rows exceeds vcap_gpt2_max_rows()"),
    ("beam", dict(offsets=[0, 3, 2]), ARG, "vcap_gpt2_beam_search_ragged: prompt offsets must be non-decreasing"),
    ("beam", dict(lens=(1, 65), desc=dict(n_positions=256)), ARG,
     "vcap_gpt2_beam_search_ragged: bad arguments (a prompt over 64 ids)"),
    ("beam", dict(bp=dict(max_new_tokens=58)), UNSUP, "context exceeds n_positions"),
    ("beam", dict(bp=dict(early_stopping=1)), UNSUP, "only early_stopping=False (the reference's presets)"),
    ("beam", dict(bp=dict(max_blocks=-1)), ARG, "vcap_gpt2_beam_search_ragged: max_blocks < 0"),
    ("beam", dict(ids=[1, 1, 1, 512]), ARG, "prompt id out of range"),
    ("beam", dict(ws_bytes=16), WS, "vcap_gpt2_beam_search_ragged: workspace too small"),
]


@pytest.mark.parametrize("row", ROWS, ids=[f"{r[0]}-{i}" for i, r in enumerate(ROWS)])
def test_ragged_refusals(row):
    entry, bad, code, msg = row
    rc, err = _call(entry, **bad)
    assert (rc, err) == (code, msg)


def _al(n):
    return (n + 255) & ~255


def test_ragged_workspace_queries():
    lib = N.lib()
    d = _gpt2()

    def q(lens, max_new=8, nb=0, desc=d, offsets=None):
        _, (_, oa) = _prompts(lens, offsets=offsets)
        if nb:
            return int(lib.vcap_gpt2_beam_search_ragged_workspace_bytes(C.byref(desc), oa, len(lens), nb, max_new))
        return int(lib.vcap_gpt2_ragged_workspace_bytes(C.byref(desc), oa, len(lens), max_new))

    # equal lengths: the uniform call's state, then the tables (row_seq, row_pos [M]; seq_len, last_row [R];
    # ids_off [B]; the ids) and the gathered last rows [R][E] f32
    B, n, E = 3, 5, 128
    M = B * (4 + n)
    uni = int(lib.vcap_gpt2_workspace_bytes(C.byref(d), B, 4 + n, 8))
    assert q((n,) * B) == uni + _al(4 * (2 * M + 2 * B + B + B * n)) + _al(4 * B * E)
    nb = 3
    uni_b = int(lib.vcap_gpt2_beam_search_workspace_bytes(C.byref(d), B, nb, 4 + n, 8))
    assert q((n,) * B, nb=nb) == uni_b + _al(4 * (2 * M * nb + 2 * B * nb + B + B * n)) + _al(4 * B * nb * E)
    # ragged lengths: positive, and no larger than the equal-length call at the longest prompt
    assert 0 < q((0, 1, 13)) <= q((13,) * 3)
    assert 0 < q((0, 1, 13), nb=2) <= q((13,) * 3, nb=2)
    # every refusal of the shape gives 0
    for nbeams in (0, 3):
        assert q((1, 65), nb=nbeams, desc=_gpt2(n_positions=256)) == 0      # a prompt over 64 ids
        assert q((1, 0), nb=nbeams, desc=_gpt2(prefix_len=0)) == 0          # an empty sequence
        assert q((5,) * 60, nb=nbeams) == 0                                 # rows
        assert q((1, 3), max_new=58, nb=nbeams) == 0                        # n_positions
        assert q((1, 3), nb=nbeams, offsets=[0, 3, 2]) == 0                 # monotone
        assert q((1, 3), nb=nbeams, offsets=[1, 2, 3]) == 0                 # offsets[0]
        assert q((1, 3), max_new=0, nb=nbeams) == 0
        assert q((1, 3), max_new=65, nb=nbeams, desc=_gpt2(n_positions=256)) == 0
        assert q((1, 3), nb=nbeams, desc=_gpt2(n_embd=192)) == 0            # the descriptor's own checks
    assert q((1,) * 9, nb=2) == 0 and q((1, 3), nb=9) == 0 and q((1, 3), nb=1) == 0
    assert q((1, 64), max_new=64, nb=2, desc=_gpt2(n_positions=256)) == 0   # longest context past 128
    assert q((5,) * 8, nb=8) == 0                                           # replicated prefill rows


# ---------------------------------------------------------------------------------------------------
def test_split_prompts():
    assert split_prompts([5, 6], 3) == ([5, 6], None)                  # one flat prompt
    assert split_prompts([], 2) == ([], None)                          # the empty prompt
    assert split_prompts([[5, 6], [5, 6]], 2) == ([5, 6], None)        # equal prompts: the one-prompt path
    assert split_prompts([[5], (6, 7), torch.tensor([8])], 3) == ([5, 6, 7, 8], [[5], [6, 7], [8]])
    assert split_prompts([[], [1]], 2) == ([1], [[], [1]])
    with pytest.raises(ValueError, match="2 prompts for 3 rows"):
        split_prompts([[1], [2]], 3)
    with pytest.raises(ValueError, match="mixes ids and sequences"):
        split_prompts([1, [2]], 2)


# ---------------------------------------------------------------------------------------------------
class _FakeTok:
    def encode_prompt(self, prompt):
        return [len(prompt)] + [ord(c) for c in prompt[:3]]

    def batch_decode(self, rows, skip_special_tokens=True):
        return ["video%d prompt%d beams%d" % tuple(r) for r in rows]


class _FakeDecoder:
    """generate_from_prefix records its call and answers row r with [prefix row tag, prompt length, beams]."""

    def __init__(self):
        self.tokenizer = _FakeTok()
        self.calls = []

    def generate_from_prefix(self, prefix, prompt_ids, **kw):
        B = prefix.shape[0]
        ids, rows = split_prompts(prompt_ids, B)
        self.calls.append(dict(B=B, ragged=rows is not None, kw=kw))
        per = rows if rows is not None else [ids] * B
        return [[int(prefix[r, 0, 0]), len(per[r]), kw["num_beams"]] for r in range(B)]


def _engine(**cfg):
    eng = object.__new__(InferenceEngine)
    eng.config = InferenceConfig(**cfg)
    eng.device = "cpu"
    dec = _FakeDecoder()
    eng.model = type("M", (), {"decoder": dec, "encode_prefix": lambda self, v, a, b: (None, v)})()
    return eng, dec


def _videos(B):
    return (torch.arange(B, dtype=torch.float32) + 1)[:, None, None].expand(B, 4, 8).contiguous()


def test_engine_default_config_makes_two_decode_calls():
    eng, dec = _engine()
    res = eng.infer_videos(_videos(2))
    assert len(dec.calls) == 2
    assert dec.calls[0]["B"] == 4 and dec.calls[0]["ragged"] and dec.calls[0]["kw"]["num_beams"] == 3
    assert dec.calls[1]["B"] == 2 and not dec.calls[1]["ragged"] and dec.calls[1]["kw"]["num_beams"] == 1
    c = eng.config
    n1, n2, n3 = (len(dec.tokenizer.encode_prompt(p)) for p in (c.prompt1, c.prompt2, c.prompt3))
    for v, r in enumerate(res):   # each row went back to its (video, candidate)
        want = tuple(clean_text(f"video{v + 1} prompt{n} beams{k}") for n, k in ((n1, 3), (n2, 3), (n3, 1)))
        assert (r.candidates.s1, r.candidates.s2, r.candidates.s3) == want
        assert len(set(want)) == 3
    # ... and the same strings with merging off, in three calls
    eng2, dec2 = _engine(merge_candidates=False)
    res2 = eng2.infer_videos(_videos(2))
    assert len(dec2.calls) == 3 and not any(k["ragged"] for k in dec2.calls)
    assert [r.candidates for r in res2] == [r.candidates for r in res]
    one, dec1 = _engine()
    assert one.infer_video(_videos(1)).candidates == res[0].candidates and len(dec1.calls) == 2


def test_engine_three_presets_make_three_calls():
    eng, dec = _engine(preset1="precise", preset2="detailed", preset3="natural")
    eng.infer_videos(_videos(2))
    assert len(dec.calls) == 3 and [k["B"] for k in dec.calls] == [2, 2, 2]


def test_engine_never_merges_sampling_candidates():
    eng, dec = _engine(preset1="natural", preset2="natural", preset3="precise")
    eng.infer_videos(_videos(2))
    assert len(dec.calls) == 3 and [k["B"] for k in dec.calls] == [2, 2, 2]
    assert [idx for _, idx in eng._candidate_groups()] == [[0], [1], [2]]
    # equal presets AND equal prompts still share a call (the rows then take the one-prompt path)
    eng, dec = _engine(preset3="precise", prompt3="")
    eng.infer_videos(_videos(1))
    assert len(dec.calls) == 1 and dec.calls[0]["B"] == 3 and dec.calls[0]["ragged"]
