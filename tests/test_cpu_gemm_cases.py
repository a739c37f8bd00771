"""The CPU twin of tests/test_gpu_gemm_sweep.py: pins the oracle, the operand conditions, the restated dispatchers
and the case list of tests/gemm_cases.py with no GPU."""
import functools

import numpy as np
import pytest
import torch

import gemm_cases as GC

ALL = GC.CASES + GC.SPLITK_CASES + GC.ROWSPLIT_CASES + [GC.LINEAR_CASE]
EXACT = [(c, p) for c in ALL if c.kind == "exact" for p in c.pairs()]
_IDS = [f"{c.name}-{p[0]}-{p[1]}" for c, p in EXACT]


def _templates(c, pair):
    return GC.template_of(c, pair, cus=GC.ROWSPLIT_CUS if c in GC.ROWSPLIT_CASES else 256)


def test_case_names_are_unique():
    names = [c.name for c in ALL]
    assert len(names) == len(set(names))


@pytest.mark.parametrize("c, pair", EXACT, ids=_IDS)
def test_exact_operands_meet_the_magnitude_condition(c, pair):
    d = GC.operands(c, pair)
    a, w = d["a"], d["w"]
    limit = 2 ** 15 if pair[0] == "f16" else 2 ** 22
    bmax = 0 if d["bias"] is None else np.abs(d["bias"]).max()
    rmax = 0 if d["res"] is None else np.abs(d["res"]).max()
    assert c.K(pair[0]) * np.abs(a).max() * np.abs(w).max() + bmax + rmax < limit
    assert np.array_equal(a, np.rint(a)) and np.array_equal(w, np.rint(w))
    for x in (d["bias"], d["res"]):
        assert x is None or np.array_equal(4 * x, np.rint(4 * x))
    t = GC.TORCH[pair[0]]
    for x in (a, w):                                  # exact in the operand type
        assert np.array_equal(torch.from_numpy(x).to(t).double().numpy(), x)


@pytest.mark.parametrize("c, pair", EXACT, ids=_IDS)
def test_f32_products_in_any_order_equal_the_integer_result(c, pair):
    d = GC.operands(c, pair)
    a, w = d["a"], d["w"]
    want = a.astype(np.int64) @ w.astype(np.int64).T
    assert np.array_equal(a @ w.T, want)              # the float64 product the oracle uses
    a32, w32 = a.astype(np.float32), w.astype(np.float32)
    rev = a32[:, ::-1] @ w32[:, ::-1].T
    assert rev.dtype == np.float32 and np.array_equal(rev.astype(np.int64), want)
    chunked = np.zeros(want.shape, np.float32)
    for k in range(0, a.shape[1], 64):
        chunked = chunked + a32[:, k:k + 64] @ w32[:, k:k + 64].T
    assert np.array_equal(chunked.astype(np.int64), want)


def test_issue_check_holds_at_its_two_shapes():
    g = np.random.default_rng(0)
    for K, am, wm in ((3072, 8, 4), (1536, 4, 2)):
        a, w = g.integers(-am, am + 1, (64, K)), g.integers(-wm, wm + 1, (48, K))
        f = torch.from_numpy(a).float() @ torch.from_numpy(w).float().T
        assert np.array_equal(f.numpy().astype(np.int64), a @ w.T)


@pytest.mark.parametrize("fmt", ["bf16", "f16"])
def test_restated_rounding_agrees_with_torch_casts(fmt):
    g = np.random.default_rng(1)
    x = np.concatenate([g.standard_normal(20000) * np.exp2(g.integers(-30, 15, 20000)),
                        g.integers(-2 ** 17, 2 ** 17, 20000) / 4.0 * (1 if fmt == "bf16" else 0.125),   # quarter steps, ties
                        np.array([0.0, 2.0 ** -24, 2.0 ** -25, 3 * 2.0 ** -25, 2.0 ** -14, 65504.0, 1025.0, 1027.0, 2049.0,
                                  257.0, 259.0, 258.0])])
    x = x.astype(np.float32).astype(np.float64)
    want = torch.from_numpy(x).float().to(GC.TORCH[fmt]).double().numpy()
    assert np.array_equal(GC.rne(x, fmt), want)
    # the rounding is idempotent, and truncation differs from it somewhere (the fault is visible)
    assert np.array_equal(GC.rne(want, fmt), want)
    assert not np.array_equal(GC.trunc16(x, fmt), want)
    assert np.all(np.abs(GC.trunc16(x, fmt)) <= np.abs(x))


def test_16_bit_outputs_are_mostly_inexact_and_hit_ties():
    """The exact cases exercise the stores' rounding: a good share of the outputs is not representable, and
    exact ties occur."""
    inexact = ties = total = 0
    for c, pair in EXACT:
        if pair[1] == "f32" or c.act or c.splitk:
            continue
        d = GC.operands(c, pair)
        h = d["a"] @ d["w"].T + (0 if d["bias"] is None else d["bias"])
        r = GC.rne(h, pair[1])
        _, e = np.frexp(h)
        half = np.ldexp(1.0, e - (8 if pair[1] == "bf16" else 11)) / 2
        inexact += int((r != h).sum())
        ties += int((np.abs(r - h) == half).sum())
        total += h.size
    assert inexact > 0.1 * total and ties > 100, (inexact, ties, total)


def test_dense_bound_holds_for_a_reversed_f32_sum_with_margin():
    for c in [c for c in GC.CASES if c.kind == "dense"]:
        for pair in c.pairs():
            d = GC.operands(c, pair)
            a32, w32 = d["a"].astype(np.float32), d["w"].astype(np.float32)
            acc = np.zeros((c.M, c.N), np.float32)
            for k in range(c.K(pair[0]) - 1, -1, -1):             # one f32 chain per element, K reversed
                acc = acc + a32[:, k:k + 1] * w32[None, :, k]
            S = np.abs(d["a"]) @ np.abs(d["w"]).T
            err = np.abs(acc.astype(np.float64) - d["a"] @ d["w"].T)
            assert np.all(err <= 0.5 * c.K(pair[0]) * 2.0 ** -23 * S + 1e-300), (c.name, pair)


def test_every_template_is_reached():
    seen = set()
    for c in ALL:
        for pair in c.pairs():
            for t in _templates(c, pair):
                key = (t["kernel"], pair, t["epi"])
                seen.add(key)
                seen.add((t["kernel"], "store", t["store"]))
                seen.add((t["kernel"], "colgroup", t["colgroup"] > 0))
                seen.add((t["kernel"], "prefetch", t["prefetch"]))
                seen.add(("splits", t["splits"], pair[0]))
    for k in ("128", "256"):
        for pair in GC.PAIRS:
            for epi in range(4):
                legal = (epi != 2 or pair[1] == "f32") and (epi != 1 or GC.SIZE[pair[0]] == GC.SIZE[pair[1]])
                assert ((k, pair, epi) in seen) == legal, (k, pair, epi)
    for key in (("128", "store", "vec"), ("128", "store", "scalar"), ("256", "store", "16B"), ("256", "store", "8B"),
                ("256", "store", "f32x4"), ("256", "colgroup", True), ("256", "colgroup", False),
                ("256", "prefetch", True), ("256", "prefetch", False)):
        assert key in seen, key
    for s in range(1, 9):
        assert ("splits", s, "bf16") in seen and ("splits", s, "f16") in seen, s


def test_split_rule_and_colgroup_restated():
    assert [GC.gemm_splits(kt) for kt, _ in GC.SPLITK_KT] == [s for _, s in GC.SPLITK_KT] == [1, 1, 2, 3, 4, 5, 6, 7, 8, 8]
    assert [GC.colgroup(n, 128, 2) for n in (256, 512, 768, 1024)] == [0, 1, 1, 2]
    assert [GC.colgroup(n, 64, 4) for n in (512, 768, 1024)] == [1, 1, 2]


def test_row_split_is_what_the_issue_states():
    for c in GC.ROWSPLIT_CASES:
        for pair in c.pairs():
            ts = GC.template_of(c, pair, cus=GC.ROWSPLIT_CUS)
            assert [(t["kernel"], t["rows"]) for t in ts] == [("256", (0, 4096)), ("128", (4096, 4252))]
            assert GC.template_of(c, pair, cus=256)[0]["kernel"] == "128"


def test_fallback_cases_are_turned_down_for_their_reason():
    for c in GC.CASES:
        for pair in c.pairs():
            assert GC.ok256(c, pair) == c.fallback or c.policy != 2, c.name
            if c.fallback:
                assert GC.template_of(c, pair)[0]["kernel"] == "128"
    assert len({c.fallback for c in GC.CASES if c.fallback}) == 6
    assert GC.offsets_overflow(2, 2 ** 31 + 64, 16, 128, 128, 2) and GC.offsets_overflow(16, 128, 2, 2 ** 31 + 64, 128, 2)
    assert not GC.offsets_overflow(25216, 3072, 3072, 3072, 3072, 2)


def test_split_k_rounding_point_case():
    """An f16 split-K case where rounding each slab differs from rounding the slab sum (the reduce kernel's R16)."""
    c, pair = GC.by_name("splitk-21kt-130x132"), ("f16", "f32")
    d = GC.operands(c, pair)
    _, want, _ = GC.oracle(c, pair, d)
    _, slab, _ = GC.oracle(c, pair, d, fault="fp16 rounding per split-K slab")
    assert (want != slab).sum() > 100


@functools.lru_cache(maxsize=None)
def _baseline(i):
    c, pair = EXACT[i]
    ts = _templates(c, pair)
    d = GC.operands(c, pair)
    return ts, d, GC.oracle(c, pair, d, ts=ts)


@pytest.mark.parametrize("fault", GC.FAULTS)
def test_exact_cases_catch_every_injected_fault(fault):
    """Each fault, injected into the oracle's arithmetic, moves what some exact-operand case expects: its bits
    where the comparison is bit for bit, and past the GELU bound where a GELU follows (the column-group tile
    order exists in the GELU template alone).  The GPU comparison would fail on a kernel making the same mistake."""
    caught = []
    for i, (c, pair) in enumerate(EXACT):
        ts, d, (_, want, bound) = _baseline(i)
        assert c.act or not bound.any()
        _, got, _ = GC.oracle(c, pair, d, fault=fault, ts=ts)
        if c.act:
            hit = bool((np.abs(got - want) > 2 * bound).any())
        else:
            hit = not np.array_equal(GC.bits(want, pair[1]), GC.bits(got, pair[1]))
        if hit:
            caught.append(f"{c.name}-{pair[0]}-{pair[1]}")
            if len(caught) == 3:
                break
    assert caught, f"no exact case catches: {fault}"
    print(f"{fault}: e.g. {caught}")


def test_oracle_layout_sentinels_and_remap():
    c, pair = GC.by_name("p1-res2-G7"), ("bf16", "f32")
    d = GC.operands(c, pair)
    c_init, exp, bound = GC.oracle(c, pair, d)
    assert exp.shape == (3 * 9 + GC.PAD_ROWS, c.N + 8) and (c_init == GC.SENT).all() and not bound.any()
    live = np.zeros(exp.shape[0], bool)
    live[GC.orow(c, np.arange(c.M))] = True
    assert (exp[~live] == GC.SENT).all() and (exp[:, c.N:] == GC.SENT).all() and live.sum() == 21 and not live[[0, 1, 9, 10, 18, 19]].any()
    m = 8                                             # group 1, row 1 -> output row 9 + 2 + 1, residual row 1 + 0
    want = d["a"][m] @ d["w"].T + d["bias"] + d["res"][1]
    assert np.array_equal(exp[12, :c.N], want)


def test_every_case_has_sentinel_columns_unless_it_says_so():
    """C is padded by sentinel columns [N, ldc) in every case; ldc == N is held by the cases named for it (and by
    vcap_linear_bias, which has no ldc)."""
    for c in ALL:
        assert (c.ldc > c.N) != ("ldc=N" in c.name or c is GC.LINEAR_CASE), c.name
    assert sum("ldc=N" in c.name for c in ALL) >= 8
