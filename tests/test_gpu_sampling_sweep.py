"""The device sampling path (the lm_head's proc_out epilogue + csrc/sample.hip) against the CPU oracle:
every kernel instance (`vcap_sample_kernel<1|8|16|32|50>`, partial and exactly-full vocabularies),
warper parameters away from the presets, both precisions, ties at the k-th value on both sides of the
kernel's 256 slots, and a row with no finite score.  tests/sampling_cases.py holds the cases;
DESIGN.md "Sampling sweep" the table and the figures observed.

Every run is free (no force_ids) through the captured graph, 8 steps.  Per case and seed, along the
device's own ids and from its own raw logits (so no GEMM error enters):
  a. warpers: ref = oracle.warp_scores(oracle.process_logits(raw, history)).  Where the oracle's top-p
     margin is >= 1e-5 the finite set of warped_out is ref's exactly, its values are within rtol 1e-5 /
     atol 1e-4 (test_gpu_surface.py's bar), and every other column is exactly -inf;
  b. draws: the id is oracle.draw(warped_out row, oracle.sample_uniform(seed, row, step)) wherever the
     draw margin is >= 1e-5; a row that has emitted EOS pads from then on;
  c. at most 5 % of a case's live (row, step) pairs are skipped by (a) and (b) together;
  d. top_k = 1: the ids are those of a greedy decode under the same processors;
  e. the second seed replays the first seed's graph (the graph cache does not grow);
  f. vocab-axis cases: the raw logits against the teacher-forced fp64 oracle along the device's ids,
     fp32 under decoder_shapes.FP32_TOL, bf16 inside decoder_shapes.bf16_tolerance."""
import numpy as np
import pytest
import torch

import decoder_shapes as S
import sampling_cases as C
from oracle import vcap_oracle as O
from vcap import _native as N
from vcap.model import GenConfig, HipGPT2Decoder

pytestmark = pytest.mark.gpu
INF = float("inf")


@pytest.fixture(scope="module")
def decoder(device):
    made = {}

    def get(V, prec):
        if (V, prec) not in made:
            made[(V, prec)] = HipGPT2Decoder(S.state_dict(C.E, V), S.arch(C.E, V), prec, device)
        return made[(V, prec)]
    return get


def _cfg(c, seed=None, use_graph=True):
    eos = c.V - 1
    if seed is None:     # greedy under the same processors
        return GenConfig(C.MAX_NEW, C.MIN_NEW, C.NGRAM, C.REP, eos, eos, use_graph)
    return GenConfig(C.MAX_NEW, C.MIN_NEW, C.NGRAM, C.REP, eos, eos, use_graph, temperature=c.T, top_k=c.k,
                     top_p=c.p, seed=seed)


class Runner:
    """One case's device buffers, kept across calls so that a second call replays the first one's graph."""

    def __init__(self, dec, c, device, pre=None):
        self.dec, self.c = dec, c
        self.pre = (C.prefix(c) if pre is None else pre).to(device)
        self.out = torch.empty(c.B, C.MAX_NEW, dtype=torch.int32, device=device)
        self.raw = torch.empty(C.MAX_NEW, c.B, c.V, dtype=torch.float32, device=device)
        self.warped = torch.empty(C.MAX_NEW, c.B, c.V, dtype=torch.float32, device=device)

    def __call__(self, cfg):
        """-> (ids int64 [B, steps], raw [steps, B, V], warped [steps, B, V]) on the CPU."""
        self.warped.fill_(float("nan"))
        ids = self.dec.generate_ids(self.pre, C.prompt(self.c), cfg, out=self.out, logits_out=self.raw,
                                    warped_out=self.warped if cfg.do_sample else None)
        torch.cuda.synchronize()
        return ids.cpu().numpy().astype(np.int64), self.raw.cpu(), self.warped.cpu()


def _check(c, seed, ids, raw, warped, rows=None):
    """Assertions a - c for one run -> (largest |warped - ref| over the kept values, skipped share)."""
    eos = c.V - 1
    hist = torch.from_numpy(ids)
    finished = np.zeros(c.B, bool)
    live = skipped = 0
    worst = 0.0
    for step in range(C.MAX_NEW):
        proc = C.process(c, raw[step], hist[:, :step])
        ref = O.warp_scores(proc, c.T, c.k, c.p)
        for r in (range(c.B) if rows is None else rows):
            tag = (c.id, seed, step, r)
            if finished[r]:
                assert ids[r, step] == eos, tag             # the pad
                continue
            live += 1
            w = warped[step, r]
            fin = torch.isfinite(w)
            assert bool((w[~fin] == -INF).all()), tag
            skip = False
            if O.top_p_margin(proc[r], c.T, c.k, c.p) >= C.MARGIN:
                assert torch.equal(fin, C.kcand_support(ref[r])), (tag, "support")
                worst = max(worst, float((w[fin] - ref[r][fin]).abs().max()))
                torch.testing.assert_close(w[fin], ref[r][fin], rtol=C.WARPED_RTOL, atol=C.WARPED_ATOL)
            else:
                skip = True
            tok, margin = O.draw(w, O.sample_uniform(seed, r, step))
            if margin >= C.MARGIN:
                assert ids[r, step] == tok, (tag, "draw", int(ids[r, step]), tok)
            else:
                skip = True
            skipped += skip
            finished[r] = ids[r, step] == eos
    share = skipped / max(live, 1)
    assert share <= C.SKIP_CAP, (c.id, seed, share)
    return worst, share


def _check_raw_logits(c, ids, raw):
    """Assertion f, as the width sweep's _check_logits_and_tokens takes its bounds."""
    lg = raw.permute(1, 0, 2).numpy()
    assert np.isfinite(lg).all()
    pre, pr = C.prefix(c), C.prompt(c)
    ref = S.teacher_forced(C.E, pre, pr, ids, "fp64", vocab=c.V)
    err64 = float(np.abs(lg - ref.numpy()).max())
    if c.prec == "fp32":
        print(f" max|gpu-fp64|={err64:.3e} (bar {S.FP32_TOL:.0e})", end="")
        assert err64 < S.FP32_TOL, (c.id, err64)
    else:
        emu = S.teacher_forced(C.E, pre, pr, ids, "bf16", vocab=c.V)
        tol = S.bf16_tolerance(ref, emu)
        erre = float(np.abs(lg - emu.numpy()).max())
        print(f" max|gpu-fp64|={err64:.3e} (tol_bf16 {tol:.3e}) max|gpu-emulated|={erre:.3e}", end="")
        assert err64 < tol, (c.id, err64, tol)
        assert erre <= tol / 3 + 1e-3, (c.id, erre, tol / 3 + 1e-3)


@pytest.mark.parametrize("case", C.CASES, ids=lambda c: c.id)
def test_sampling_case(decoder, device, case):
    c = case
    run = Runner(decoder(c.V, c.prec), c, device)
    size = None
    for n, seed in enumerate(C.SEEDS):
        ids, raw, warped = run(_cfg(c, seed))
        if n == 0:
            size = N.lib().vcap_graph_cache_size()
        else:
            assert N.lib().vcap_graph_cache_size() == size, "a second seed captured a second graph"
        worst, share = _check(c, seed, ids, raw, warped)
        print(f"\nsampling-gpu {c.id} <{C.INSTANCE[c.V]}> seed={seed} max|warped-ref|={worst:.3e} "
              f"skipped share={share:.4f}", end="")
        if n == 0 and c in C.VOCAB_CASES:
            _check_raw_logits(c, ids, raw)
        if c.k == 1:
            assert bool((torch.isfinite(warped).sum(-1) == 1).all())
        if c.k >= c.V and c.p == 1.0:      # the whole unbanned vocabulary is the support
            proc0 = C.process(c, raw[0], torch.zeros(c.B, 0, dtype=torch.long))
            assert torch.equal(torch.isfinite(warped[0]), torch.isfinite(proc0))
            assert int(torch.isfinite(warped[0, 0]).sum()) == c.V - 1
    if c.k == 1:     # one token survives whatever u is: the greedy decode under the same processors
        gids, _, _ = run(_cfg(c))
        assert np.array_equal(gids, ids), (c.id, "top_k 1 is not the greedy path")


def test_seeds_and_determinism(decoder, device):
    """The same seed twice is bit-identical, eager and graph alike; another seed through the same
    captured graph changes at least one of the 40 draws and adds no graph."""
    c = C.VOCAB_CASES[C.VOCABS.index(8193)]
    run = Runner(decoder(c.V, c.prec), c, device)
    a, b = C.SEEDS
    first = run(_cfg(c, a))
    size = N.lib().vcap_graph_cache_size()
    again = run(_cfg(c, a))
    eager = run(_cfg(c, a, use_graph=False))
    eager2 = run(_cfg(c, a, use_graph=False))
    for other in (again, eager, eager2):
        assert np.array_equal(other[0], first[0])
        assert torch.equal(other[2].view(torch.int32), first[2].view(torch.int32))
    other_seed = run(_cfg(c, b))
    assert N.lib().vcap_graph_cache_size() == size
    assert not np.array_equal(other_seed[0], first[0])


def _tied_decoder(device, src, dst):
    c = C.TIES_INSIDE
    return HipGPT2Decoder(C.with_duplicates(S.state_dict(C.E, c.V), src, dst), C.arch(c), c.prec, device)


def _assert_columns_bit_equal(raw, cols):
    r = raw[:, :, cols].contiguous().view(torch.int32)
    assert torch.equal(r, r[:, :, :1].expand_as(r)), "equal wte rows gave different logits: column-dependent arithmetic"


def test_ties_at_the_kth_value_are_all_kept(device):
    """12 equal scores across the k-th rank (k = 50) at row 0's step 0: HF keeps them all, and so does
    the bisection - the support is the strictly greater tokens plus the 12, more than k."""
    c = C.TIES_INSIDE
    src, dst = C.ties_inside_rows()
    cols = [src] + dst
    run = Runner(_tied_decoder(device, src, dst), c, device)
    seed = C.TIE_SEEDS["inside"]
    ids, raw, warped = run(_cfg(c, seed))
    _assert_columns_bit_equal(raw, cols)
    proc0 = C.process(c, raw[0], torch.zeros(c.B, 0, dtype=torch.long))[0]
    above = int((proc0 > proc0[src]).sum())
    assert c.k - C.N_TIES_INSIDE < above < c.k, above          # the ties straddle the k-th rank
    fin = torch.isfinite(warped[0, 0])
    assert int(fin.sum()) == above + C.N_TIES_INSIDE > c.k and bool(fin[cols].all())
    worst, share = _check(c, seed, ids, raw, warped)
    print(f"\nsampling-gpu ties inside: {above} above + {C.N_TIES_INSIDE} tied kept, max|warped-ref|={worst:.3e} "
          f"skipped share={share:.4f}", end="")


def test_ties_past_the_survivor_slots_have_a_defined_result(device):
    """300 equal scores at the top: HF's support is all 300, the kernel holds 256.  Its documented
    choice (include/vcap.h): every score strictly above the threshold, then the tied tokens of lowest
    vocabulary index until 256 are kept - the same set on every run, and every draw inside it.
    Before the ordered selection the slots went by atomicAdd arrival order: row 0's step 0 happened to
    keep the expected set, but three runs of one seed were not bit-identical."""
    c = C.TIES_INSIDE
    src, dst = C.ties_over_rows()
    cols = sorted([src] + dst)
    run = Runner(_tied_decoder(device, src, dst), c, device)
    seed = C.TIE_SEEDS["over"]
    runs = [run(_cfg(c, seed)) for _ in range(3)]
    ids, raw, warped = runs[0]
    _assert_columns_bit_equal(raw, cols)
    proc0 = C.process(c, raw[0], torch.zeros(c.B, 0, dtype=torch.long))[0]
    assert int((proc0 > proc0[src]).sum()) == 0                # the ties are row 0's top score
    got = torch.nonzero(torch.isfinite(warped[0, 0])).flatten().tolist()
    same = all(torch.equal(r[2].view(torch.int32), warped.view(torch.int32)) and np.array_equal(r[0], ids)
               for r in runs[1:])
    print(f"\nsampling-gpu ties past kCand: row 0 step 0 keeps {len(got)} tokens, "
          f"{len(set(got) - set(cols[:C.KCAND]))} outside the {C.KCAND} tied tokens of lowest index; "
          f"three runs bit-identical: {same}", end="")
    assert got == cols[:C.KCAND]
    assert same
    worst, share = _check(c, seed, ids, raw, warped)           # the support rule at every step, every draw
    print(f" max|warped-ref|={worst:.3e} skipped share={share:.4f}", end="")


def test_row_without_a_finite_score_emits_eos(decoder, device):
    """Row 1's prefix is all NaN: it emits EOS at step 0 without a draw and pads afterwards, its warped
    rows are all -inf, and rows 0 and 2 are bit-identical to the same call with a finite row 1."""
    c = C.NAN_CASE
    eos, seed = c.V - 1, C.SEEDS[0]
    dec = decoder(c.V, c.prec)
    ids, raw, warped = Runner(dec, c, device)(_cfg(c, seed))
    pre = C.prefix(c)
    pre[1] = float("nan")
    nids, nraw, nwarped = Runner(dec, c, device, pre)(_cfg(c, seed))
    assert (nids[1] == eos).all()
    assert bool((nwarped[:, 1] == -INF).all())
    for r in (0, 2):
        assert np.array_equal(nids[r], ids[r])
        assert torch.equal(nraw[:, r].view(torch.int32), raw[:, r].view(torch.int32))
        assert torch.equal(nwarped[:, r].view(torch.int32), warped[:, r].view(torch.int32))
    _check(c, seed, nids, nraw, nwarped, rows=(0, 2))
