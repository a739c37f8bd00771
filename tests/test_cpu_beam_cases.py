"""The beam case table (tests/beam_cases.py) checked from the CPU oracle alone: every row listed as
certain clears the margin bound, the table reaches every beam width, length penalty, processor setting
and finished-hypothesis event the device kernels branch on, and it has the shapes the GPU test needs.
Prints each case's minimum margin over its bound and its events (pytest -s)."""
import pytest

import beam_cases as BC

UNCERTAIN_CAP = 0.25


def _rows():
    """(case, row index, trace, listed certain) over the whole table."""
    for c in BC.CASES:
        _, tr = BC.oracle(c.name)
        for b, listed in enumerate(BC.listed_certain(c)):
            yield c, b, tr, listed


def _events(c, tr, b):
    """The event names row b of its batch shows."""
    ev = tr["events"][b]
    out = {k for k in ("did", "late", "evict", "best_replaced") if ev[k] > 0}
    if tr["sat_step"][b] is not None and tr["sat_step"][b] < tr["steps"] - 1:
        out.add("satisfied_while_others_continue")
    if tr["stopped_early"]:
        out.add("stop_before_L")
    if tr["lengths"][b] < c.L:
        out.add("best_shorter_than_L")
    return out


@pytest.mark.parametrize("name", [c.name for c in BC.CASES])
def test_listed_rows_are_certain(name):
    c = BC.BY_NAME[name]
    rows, tr = BC.oracle(name)
    ratios = [BC.margin_over_bound(c, tr, b) for b in range(len(c.seeds))]
    print(f"\nbeam-case {name}: nb={c.nb} L={c.L} lpen={c.lpen} steps={tr['steps']} lengths={tr['lengths']} "
          f"sat_step={tr['sat_step']} margin/GAP={[round(r, 2) for r in ratios]} events={tr['events']}", end="")
    assert len(set(c.seeds)) == len(c.seeds) and set(c.uncertain) <= set(c.seeds)
    for b, listed in enumerate(BC.listed_certain(c)):
        if listed:
            assert BC.certain(c, tr, b), (name, c.seeds[b], ratios[b])
        assert len(tr["margins"][b]) == (tr["sat_step"][b] + 1 if tr["sat_step"][b] is not None else tr["steps"])
    # a certain row searched alone is the same row: sequences are independent in the search
    b = BC.listed_certain(c).index(True)
    alone, tr1 = BC.run_oracle(c, [c.seeds[b]])
    n = tr["lengths"][b]
    assert tr1["lengths"] == [n] and alone[0][:n] == rows[b][:n]


def test_f32_oracle_agrees_on_certain_rows():
    """The float32 forward (what transformers runs) and the float64 forward give a certain row the same
    hypothesis - the bound is wide enough for an f32 forward's own error."""
    for c in BC.CASES:
        rows, tr = BC.oracle(c.name)
        rows32, tr32 = BC.run_oracle(c, f32=True)
        for b, listed in enumerate(BC.listed_certain(c)):
            if listed:
                n = tr["lengths"][b]
                assert tr32["lengths"][b] == n and rows32[b][:n] == rows[b][:n], (c.name, b)


def test_uncertain_rows_are_few():
    rows = list(_rows())
    unc = sum(not listed for _, _, _, listed in rows)
    print(f"\nbeam-cases: {len(rows)} rows, {len(rows) - unc} certain, {unc} uncertain", end="")
    assert unc <= UNCERTAIN_CAP * len(rows), (unc, len(rows))


def test_table_coverage():
    cert = [(c, b, tr) for c, b, tr, listed in _rows() if listed]
    have = lambda pred: any(pred(c, b, tr) for c, b, tr in cert)  # noqa: E731
    for nb in range(2, 9):
        assert have(lambda c, b, tr: c.nb == nb), nb
    for lp in (0.0, 1.0, 2.0):
        assert have(lambda c, b, tr: c.lpen == lp), lp
    assert have(lambda c, b, tr: c.min_new == 0) and have(lambda c, b, tr: c.min_new > 0)
    assert have(lambda c, b, tr: c.rep == 1.0 and c.ngram == 0)
    assert have(lambda c, b, tr: c.ngram == 2)
    seen = {}
    for c, b, tr in cert:
        for e in _events(c, tr, b):
            seen[e] = seen.get(e, 0) + 1
    print(f"\nbeam-cases events over certain rows: {seen}", end="")
    for e in ("did", "late", "evict", "best_replaced", "satisfied_while_others_continue", "stop_before_L",
              "best_shorter_than_L"):
        assert seen.get(e, 0) > 0, e


def test_required_shapes():
    by = BC.BY_NAME
    assert any(c.nb == 8 and len(c.seeds) == 8 and len(set(BC.oracle(c.name)[1]["lengths"])) > 1 for c in BC.CASES)
    assert any(len(c.seeds) == 1 for c in BC.CASES)
    assert any(c.nb == 3 and len(c.seeds) == 5 for c in BC.CASES)
    c = by["v2053_nb8"]   # two chunks of 2048, the last 5 columns wide (< 2 nb), EOS inside it
    assert c.V == 2053 and c.nb == 8 and c.eos == 2052 and c.V - 2048 < 2 * c.nb
    c = by["v2053_early"]
    tr = BC.oracle(c.name)[1]
    assert c.V == 2053 and min(tr["lengths"]) < c.L // 2 and tr["stopped_early"]
    c = by["long_s64"]    # S0 = 64, S0 + L = 128: the context crosses 64 at the first step
    tr = BC.oracle(c.name)[1]
    assert c.prompt_len + 4 == 64 and c.L == 64
    assert any(listed and len(tr["margins"][b]) >= 20 for b, listed in enumerate(BC.listed_certain(c)))
    assert any(c.E in (256, 384) for c in BC.CASES)
    assert set(BC.GOLDEN_CASES) <= set(by) and 8 <= len(BC.GOLDEN_CASES) <= 12
    gold = [by[n] for n in BC.GOLDEN_CASES]
    assert {c.nb for c in gold} == set(range(2, 9)) and {c.lpen for c in gold} == {0.0, 1.0, 2.0}
    assert "long_s64" in BC.GOLDEN_CASES
