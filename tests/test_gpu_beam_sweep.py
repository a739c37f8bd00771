"""Device beam search (csrc/beam.hip through vcap_gpt2_beam_search) on EOS-rich searches: the case table
of tests/beam_cases.py - every vcap_beam_cand_kernel<2 NB> / vcap_beam_select_kernel<NB, NC> instance
(NB 2..8), finished-hypothesis bookkeeping (EOS among the first nb and in ranks nb..2nb-1, evictions,
sequences satisfied while others go on, a stop before max_new_tokens, lengths that differ across the
batch), length penalties 0 / 1 / 2, processors on and off, a vocabulary whose last candidate chunk has
5 columns, and a 64-position prompt (vcap_decode_attention_anc_kernel, the second ancestry word of
the select kernel, anc_ld = 128).

Per case the captured graph, the eager launches and the host-bookkeeping search.beam_search:
  * on rows the table calls certain (every oracle decision margin above GAP(E, t), beam_cases.py) give
    the fp64-forward oracle's ids and lengths - and transformers' own where tests/golden/beam_eos has
    the case;
  * graph == eager bit for bit on every row;
  * every row is well formed (length, EOS padding, MinNewTokens, no repeated n-gram, ids < V), read
    from the raw [B, L] buffer and lengths_out.
DESIGN.md "Beam search coverage" has the measured outcome."""
import numpy as np
import pytest
import torch

import beam_cases as BC
from helpers import case, golden
from vcap import _native as N
from vcap import search
from vcap.model import HipGPT2Decoder

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def decoder(device):
    made = {}

    def get(E, V, prec="fp32"):
        if (E, V, prec) not in made:
            made[(E, V, prec)] = HipGPT2Decoder(BC.state_dict(E, V), BC.arch(E, V), prec, device)
        return made[(E, V, prec)]
    return get


def _device(dec, pre, prompt, kw, use_graph=True):
    """beam_search_device -> (raw ids [B, L], lengths_out [B]) as the device left them."""
    search.beam_search_device(dec, pre, prompt, use_graph=use_graph, **kw)
    _, out, lens = dec._beam_bufs[(pre.shape[0], kw["num_beams"], kw["max_new_tokens"])]
    torch.cuda.synchronize()
    return out.cpu().numpy().copy(), lens.cpu().numpy().copy()


def _host(dec, pre, prompt, kw, L):
    """search.beam_search -> (ids EOS-padded to [B, L], lengths by the first EOS)."""
    rows = search.beam_search(dec, pre, prompt, **kw)
    eos = kw["eos"]
    raw = np.array(BC.padded(rows, L, eos), dtype=np.int32)
    lens = np.array([r.index(eos) + 1 if eos in r else len(r) for r in rows], dtype=np.int32)
    return raw, lens


def _well_formed(raw, lens, *, V, L, eos, min_new, ngram, tag):
    assert raw.shape[1] == L and ((raw >= 0) & (raw < V)).all(), tag
    for r, (row, n) in enumerate(zip(raw.tolist(), lens.tolist())):
        assert n == (row.index(eos) + 1 if eos in row else L), (tag, r, n, row)
        assert all(t == eos for t in row[n:]), (tag, r, row)
        assert eos not in row[:min(min_new, L)], (tag, r, row)
        if ngram:
            grams = [tuple(row[i:i + ngram]) for i in range(n - ngram + 1)]
            assert len(grams) == len(set(grams)), (tag, r, row)


def _wf(c, raw, lens, tag):
    _well_formed(raw, lens, V=c.V, L=c.L, eos=c.eos, min_new=c.min_new, ngram=c.ngram, tag=tag)


def _oracle_raw(c):
    rows, tr = BC.oracle(c.name)
    return np.array(BC.padded(rows, c.L, c.eos), dtype=np.int32), np.array(tr["lengths"], dtype=np.int32)


def _same_rows(raw, lens, exp, exp_lens):
    return [bool(lens[b] == exp_lens[b] and np.array_equal(raw[b], exp[b])) for b in range(len(lens))]


@pytest.mark.parametrize("name", [c.name for c in BC.CASES])
def test_case_matches_oracle(decoder, device, name):
    c = BC.BY_NAME[name]
    dec, pre, prompt, kw = decoder(c.E, c.V), BC.prefix(c).to(device), BC.prompt(c), BC.search_kwargs(c)
    exp, exp_lens = _oracle_raw(c)
    listed = BC.listed_certain(c)
    graph = _device(dec, pre, prompt, kw, True)
    eager = _device(dec, pre, prompt, kw, False)
    host = _host(dec, pre, prompt, kw, c.L)
    print(f"\nbeam-gpu {name}: certain {sum(listed)} uncertain {len(listed) - sum(listed)}", end="")
    for tag, (raw, lens) in (("graph", graph), ("eager", eager), ("host", host)):
        same = _same_rows(raw, lens, exp, exp_lens)
        print(f" | {tag} identical {sum(same)}/{len(same)} lengths {lens.tolist()}", end="")
        _wf(c, raw, lens, (name, tag))
        for b, cert in enumerate(listed):
            if cert:
                assert same[b], (name, tag, b, raw[b].tolist(), exp[b].tolist(), int(lens[b]), int(exp_lens[b]))
    assert np.array_equal(graph[0], eager[0]) and np.array_equal(graph[1], eager[1]), (name, "graph != eager")


@pytest.mark.parametrize("name", BC.GOLDEN_CASES)
def test_case_matches_transformers(decoder, device, name):
    """The device ids equal what transformers' generate() returned (tests/golden/beam_eos)."""
    c = BC.BY_NAME[name]
    _, g = golden("beam_eos")
    hf, hf_lens = g[f"{name}_ids"], g[f"{name}_lengths"]
    raw, lens = _device(decoder(c.E, c.V), BC.prefix(c).to(device), BC.prompt(c), BC.search_kwargs(c))
    hf_raw = np.array(BC.padded(hf.tolist(), c.L, c.eos), dtype=np.int32)
    same = _same_rows(raw, lens, hf_raw, hf_lens)
    print(f"\nbeam-gpu-hf {name}: identical {sum(same)}/{len(same)}", end="")
    for b, cert in enumerate(BC.listed_certain(c)):
        if cert:
            assert same[b], (name, b, raw[b].tolist(), hf_raw[b].tolist())
    if all(BC.listed_certain(c)):
        assert int(lens.max()) == hf.shape[1]   # the width generate() returns


def test_params_are_part_of_the_graph_key(decoder, device):
    """One decoder object, one shape, two searches that differ only in eos / length_penalty: each call
    gives its own result (the captured graph's key carries the beam params), before and after
    vcap_graph_cache_clear."""
    c = BC.BY_NAME["nb3_b5"]
    dec, pre, prompt = decoder(c.E, c.V), BC.prefix(c).to(device), BC.prompt(c)
    kw_a = BC.search_kwargs(c)
    kw_b = dict(kw_a, eos=450, length_penalty=2.0)
    ref_a, ref_b = _device(dec, pre, prompt, kw_a, False), _device(dec, pre, prompt, kw_b, False)
    assert not np.array_equal(ref_a[0], ref_b[0])
    exp, exp_lens = _oracle_raw(c)
    same = _same_rows(*ref_a, exp, exp_lens)
    assert all(s for s, cert in zip(same, BC.listed_certain(c)) if cert)
    for kw, ref in ((kw_a, ref_a), (kw_b, ref_b), (kw_a, ref_a), (kw_b, ref_b)):
        raw, lens = _device(dec, pre, prompt, kw, True)
        assert np.array_equal(raw, ref[0]) and np.array_equal(lens, ref[1]), kw
    _well_formed(*ref_b, V=c.V, L=c.L, eos=450, min_new=c.min_new, ngram=c.ngram, tag="eos 450")
    assert int(N.lib().vcap_graph_cache_size()) >= 2
    N.lib().vcap_graph_cache_clear()
    assert int(N.lib().vcap_graph_cache_size()) == 0
    for kw, ref in ((kw_b, ref_b), (kw_a, ref_a)):
        raw, lens = _device(dec, pre, prompt, kw, True)
        assert np.array_equal(raw, ref[0]) and np.array_equal(lens, ref[1]), ("after clear", kw)


@pytest.mark.parametrize("name", BC.BF16_CASES)
def test_bf16_rows_invariant_with_mixed_stops(decoder, device, name):
    """bf16 decoder, rows that stop at different steps: graph == eager bit for bit, every batch row is
    the row searched alone, and the output is well formed.  No token equality with the fp64 oracle: a
    bf16 search's near-ties are not bounded here."""
    c = BC.BY_NAME[name]
    dec, pre, prompt, kw = decoder(c.E, c.V, "bf16"), BC.prefix(c).to(device), BC.prompt(c), BC.search_kwargs(c)
    raw, lens = _device(dec, pre, prompt, kw, True)
    eraw, elens = _device(dec, pre, prompt, kw, False)
    assert np.array_equal(raw, eraw) and np.array_equal(lens, elens), name
    _wf(c, raw, lens, (name, "bf16"))
    print(f"\nbeam-gpu-bf16 {name}: lengths {lens.tolist()}", end="")
    for b in range(pre.shape[0]):
        raw1, lens1 = _device(dec, pre[b:b + 1].contiguous(), prompt, kw, True)
        assert lens1[0] == lens[b] and np.array_equal(raw1[0], raw[b]), (name, b, raw1[0].tolist(), raw[b].tolist())


ANY_SEEDS = (35, 73, 45, 47, 26, 17, 5, 19, 67, 64, 20)   # 11 sequences: device chunks of 8 + 3


def test_beam_search_any_chunks_a_batch_of_11(decoder, device):
    c = BC.BY_NAME["nb3_b5"]
    dec, prompt, kw = decoder(c.E, c.V), BC.prompt(c), BC.search_kwargs(c)
    pre = BC.prefix_rows(c.E, ANY_SEEDS).to(device)
    rows = search.beam_search_any(dec, pre, prompt, **kw)
    alone = [search.beam_search_device(dec, pre[b:b + 1].contiguous(), prompt, **kw)[0] for b in range(len(ANY_SEEDS))]
    width = max(len(r) for r in alone)
    assert len({len(r) for r in alone}) > 1 and width < c.L   # mixed lengths, padding to do
    assert rows == BC.padded(alone, width, c.eos), (rows, alone)
    oracle_rows, tr = BC.run_oracle(c, ANY_SEEDS)
    assert all(BC.certain(c, tr, b) for b in range(len(ANY_SEEDS)))
    assert rows == BC.padded(oracle_rows, width, c.eos)


def test_beam_search_any_host_fallback_and_nc20(device):
    """GPT-2 small (vocab 50257: 25 candidate chunks), 8 new tokens.  num_beams 6 needs 1800 candidates:
    vcap_gpt2_beam_search refuses with E_UNSUPPORTED and beam_search_any returns the host search's rows.
    num_beams 5 (1250 candidates) runs on the device in the 20-candidates-per-lane select form; its rows
    are checked structurally and graph == eager; whether they equal the host search's is printed, not
    asserted - no margin bound is derived for the 12-layer decoder, so near-ties between the two
    forwards' last bits are not excluded."""
    meta, g, va, ga, sd, frames = case("b16_b2")
    dec = HipGPT2Decoder(sd, ga, "fp32", device)
    pre = torch.from_numpy(g["inputs_embeds"][:, :4].copy()).to(device)
    L = 8
    kw = dict(num_beams=6, max_new_tokens=L, min_new_tokens=2, no_repeat_ngram_size=3, repetition_penalty=1.1,
              eos=ga.eos_token_id, length_penalty=1.0)
    with pytest.raises(N.VcapError) as err:
        search.beam_search_device(dec, pre, meta["prompt_ids"], **kw)
    assert err.value.rc == N.E_UNSUPPORTED
    host = search.beam_search(dec, pre, meta["prompt_ids"], **kw)
    assert search.beam_search_any(dec, pre, meta["prompt_ids"], **kw) == host
    kw["num_beams"] = 5
    raw, lens = _device(dec, pre, meta["prompt_ids"], kw, True)
    eraw, elens = _device(dec, pre, meta["prompt_ids"], kw, False)
    assert np.array_equal(raw, eraw) and np.array_equal(lens, elens)
    _well_formed(raw, lens, V=ga.vocab, L=L, eos=ga.eos_token_id, min_new=2, ngram=3, tag="nb5 NC20")
    hraw, hlens = _host(dec, pre, meta["prompt_ids"], kw, L)
    print(f"\nbeam-gpu nb=5 V=50257: device {raw.tolist()} host-equal {np.array_equal(raw, hraw)}", end="")
    assert search.beam_search_any(dec, pre, meta["prompt_ids"], **kw) == [r[:int(lens.max())] for r in raw.tolist()]
