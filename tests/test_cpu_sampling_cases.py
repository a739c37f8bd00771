"""CPU side of the sampling sweep (test_gpu_sampling_sweep.py): what that sweep compares the device
with is pinned here with no GPU in the loop.

  * oracle.warp_scores equals transformers' own Temperature -> TopK -> TopP warpers bit for bit (the
    one place HF is consulted; skipped where transformers is not installed);
  * oracle.philox4x32_10 gives the Random123 known answers; sample_uniform keys it as documented;
  * oracle.draw walks the kept tokens ascending, ties by vocabulary index;
  * along the fp64 oracle's own sampled path, the share of (row, step) pairs whose top-p or draw
    margin is under 1e-5 is at most half the GPU sweep's skip cap, for every case and both seeds;
  * the settings do produce n-gram bans within 8 steps, and the tie constructions put the equal
    scores where the GPU tests need them.
"""
import numpy as np
import pytest
import torch

import decoder_shapes as S
import sampling_cases as C
from oracle import vcap_oracle as O

INF = float("inf")


def _hf_warp(scores, T, k, p):
    lp = pytest.importorskip("transformers.generation.logits_process")
    s = lp.TemperatureLogitsWarper(T)(None, scores)
    s = lp.TopKLogitsWarper(top_k=k)(None, s)
    if p < 1.0:
        s = lp.TopPLogitsWarper(top_p=p, min_tokens_to_keep=1)(None, s)
    return s


def _rows(kind, V, k):
    g = torch.Generator().manual_seed(V + 31 * k)
    x = 0.6 * torch.randn(4, V, generator=g, dtype=torch.float32)
    if kind == "neg_inf":
        x[:, torch.randperm(V, generator=g)[:V // 3]] = -INF
        x[1, :] = -INF
        x[1, 5:9] = torch.tensor([0.3, -0.2, 0.4, 1.0])     # fewer finite scores than k
    if kind == "ties":
        kk = min(k, V)
        for r in range(4):          # 7 equal scores placed across the k-th rank
            srt = torch.sort(x[r], descending=True)
            lo = max(kk - 3, 0)
            x[r, srt.indices[lo:lo + 7]] = srt.values[lo]
    return x


@pytest.mark.parametrize("T,k,p", C.PARAMS + [(0.9, 128, 1.0)])
@pytest.mark.parametrize("kind", ["random", "neg_inf", "ties"])
@pytest.mark.parametrize("V", [64, 1025])
def test_warp_scores_is_hf_bit_for_bit(V, kind, T, k, p):
    """V = 64 with k = 128 is top_k >= V.  The -inf mask is part of torch.equal."""
    x = _rows(kind, V, k)
    ref = _hf_warp(x.clone(), T, k, p)
    got = O.warp_scores(x, T, k, p)
    assert got.dtype == torch.float32 and torch.equal(got, ref)
    if kind == "ties" and p == 1.0 and k < V:
        assert int(torch.isfinite(got[0]).sum()) > k      # the ties at the k-th value all stay


def test_philox_known_answers():
    """Random123's kat_vectors for philox4x32-10."""
    kat = [((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
            "d16cfe09 94fdcceb 5001e420 24126ea1")]
    for ctr, key, want in kat:
        assert " ".join(f"{w:08x}" for w in O.philox4x32_10(ctr, key)) == want


def test_sample_uniform_keying():
    seed = (0x299f31d0 << 32) | 0xa4093822
    w0 = O.philox4x32_10((5, 3, 0, 0), (0xa4093822, 0x299f31d0))[0]
    u = O.sample_uniform(seed, row=3, step=5)
    assert u == (w0 >> 8) / 2.0 ** 24 and 0.0 <= u < 1.0
    # row, step and both key words all matter
    others = {O.sample_uniform(seed, 5, 3), O.sample_uniform(seed, 3, 6), O.sample_uniform(seed, 4, 5),
              O.sample_uniform(seed ^ 1, 3, 5), O.sample_uniform(seed ^ (1 << 32), 3, 5)}
    assert u not in others and len(others) == 5


def test_draw_walks_ascending_with_ties_by_index():
    row = torch.full((8,), -INF, dtype=torch.float64)
    row[[6, 1, 4]] = torch.tensor([0.0, 0.0, np.log(2.0)])       # masses 1, 1, 2: order 1, 6, 4
    assert [O.draw(row, u)[0] for u in (0.0, 0.24, 0.25, 0.49, 0.5, 0.99)] == [1, 1, 6, 6, 4, 4]
    tok, margin = O.draw(row, 0.3)
    assert tok == 6 and margin == pytest.approx(0.05)
    assert O.draw(row, 0.25)[1] == pytest.approx(0.0, abs=1e-15)  # on a boundary: no margin


def test_top_p_margin():
    row = torch.log(torch.tensor([0.1, 0.2, 0.3, 0.4]))
    assert O.top_p_margin(row, 1.0, 4, 1.0) == INF
    # ascending cumsum 0.1, 0.3, 0.6, 1.0 against 1 - p = 0.25
    assert O.top_p_margin(row, 1.0, 4, 0.75) == pytest.approx(0.05, abs=1e-6)
    # top_k 2 first: 0.3, 0.4 renormalised -> cumsum 3/7, 1
    assert O.top_p_margin(row, 1.0, 2, 0.5) == pytest.approx(0.5 - 3 / 7, abs=1e-6)


def test_kcand_support_rule():
    ref = torch.full((1000,), -INF)
    ref[[3, 900]] = 2.0
    ref[10:310] = 1.0                                   # 300 tied below two larger scores
    keep = C.kcand_support(ref)
    assert int(keep.sum()) == C.KCAND and keep[3] and keep[900]
    assert torch.equal(torch.nonzero(keep).flatten(), torch.tensor([3] + list(range(10, 264)) + [900]))
    ref[200:] = -INF                                    # 192 survivors: HF's own support
    assert torch.equal(C.kcand_support(ref), torch.isfinite(ref))


@pytest.mark.parametrize("case", C.CASES, ids=lambda c: c.id)
def test_skipped_share_within_half_the_cap(case):
    """The oracle's own free-running sampled path, both seeds: the pairs a margin would skip."""
    for seed in C.SEEDS:
        f = C.oracle_path(case, seed)
        share = C.skipped_share(f["live"], f["top_p_margin"], f["draw_margin"])
        kept = int(f["live"].sum())
        print(f"\nsampling-cpu {case.id} seed={seed} live pairs={kept} skipped share={share:.4f} "
              f"min top-p margin={f['top_p_margin'].min():.3e} min draw margin={f['draw_margin'].min():.3e} "
              f"bans={f['bans']}", end="")
        assert kept >= case.B * C.MIN_NEW                      # EOS is banned for the first two steps
        assert share <= C.SKIP_CAP / 2, (case.id, seed, share)
        assert f["ids"].shape == (case.B, C.MAX_NEW) and (f["ids"][~f["live"]] == case.V - 1).all()


@pytest.mark.parametrize("ties", ["inside", "over"])
def test_tie_paths_skip_nothing(ties):
    """The tie tests have 16 (row, step) pairs, so one skipped pair is over the cap: the seed each runs
    is one whose oracle path (drawing from the device's documented support) skips none."""
    f = C.oracle_path(C.TIES_INSIDE, C.TIE_SEEDS[ties], ties)
    share = C.skipped_share(f["live"], f["top_p_margin"], f["draw_margin"])
    print(f"\nsampling-cpu ties {ties} seed={C.TIE_SEEDS[ties]} live pairs={int(f['live'].sum())} "
          f"skipped share={share:.4f} min draw margin={f['draw_margin'].min():.3e}", end="")
    assert share == 0.0


def test_bans_do_occur():
    """No-repeat 2-grams with 8 steps: at least one case's path carries a ban."""
    bans = {c.id: sum(C.oracle_path(c, s)["bans"] for s in C.SEEDS) for c in C.CASES}
    print(f"\nsampling-cpu n-gram bans per case: {bans}", end="")
    assert sum(bans.values()) >= 1


def test_top_k_one_path_is_the_greedy_path():
    """top_k = 1 leaves one token, whatever u is: the sampled path is the processed argmax path."""
    case = next(c for c in C.CASES if c.k == 1)
    a, b = (C.oracle_path(case, s)["ids"] for s in C.SEEDS)
    assert np.array_equal(a, b)


def test_tie_constructions():
    """Ties within kCand: 44 scores strictly above 12 equal ones at row 0's step 0 (ranks 45 .. 56
    around k = 50).  Ties past kCand: 300 equal scores at the top.  Both on the fp64 oracle's step-0
    logits of the duplicated model; no duplicate touches the prompt's row."""
    c = C.TIES_INSIDE
    ar, base = C.arch(c), S.sd64(C.E, vocab=c.V)
    for (src, dst), n, above in ((C.ties_inside_rows(), C.N_TIES_INSIDE, C.TIE_K - 6),
                                 (C.ties_over_rows(), C.N_TIES_OVER, 0)):
        rows = [src] + list(dst)
        assert len(set(rows)) == n and c.V - 1 not in rows
        sd = dict(base)
        w = base[S.WTE].clone()
        w[dst] = w[src].clone()
        sd[S.WTE] = sd["decoder.model.lm_head.weight"] = w
        with torch.no_grad():
            lg = O.gpt2_forward(sd, ar, O.build_inputs(sd, ar, C.prefix(c).double(), C.prompt(c)),
                                O.KVCache(ar.n_layer))[0, -1]
        assert (lg[rows] == lg[src]).all()
        lg[c.V - 1] = -INF                                    # EOS is banned at step 0
        assert int((lg > lg[src]).sum()) == above
        ref = O.warp_scores(lg.float()[None], c.T, c.k, 1.0)[0]
        assert int(torch.isfinite(ref).sum()) == above + n    # HF keeps every tie
        if n > C.KCAND:
            assert torch.nonzero(C.kcand_support(ref)).flatten().tolist() == sorted(rows)[:C.KCAND]
