"""The oracles of the text tower's backward tests (tests/text_grad_cases.py) pinned on the CPU: the fp64
autograd oracle against finite differences and against its plain-torch restatement, the float32 run and the
bf16 emulation finite on every case, which parameter tensors are identically zero on which case (the GPU test
asserts exact +0 there), the sparse-to-dense embedding helper against torch's dense txt_emb.weight.grad, and
the argument refusals of scripts/train_align.py.  No GPU, no native library.
"""
import numpy as np
import pytest
import torch

import text_grad_cases as GC
import text_tower_cases as TC


@pytest.mark.parametrize("case", GC.ALL_CASES, ids=GC.case_id)
def test_the_reference_runs_are_finite_and_the_restatement_is_the_modules(case):
    g64 = GC.oracle_grads(case)
    restated = GC.grads_of(case, "restated")
    for kind in ("f32", "bf16"):
        gs = GC.grads_of(case, kind)
        assert gs.keys() == g64.keys()
        assert all(bool(torch.isfinite(g).all()) for g in gs.values()), kind
    errs = GC.errors(restated, g64)
    worst = max(errs.values(), default=0.0)
    print(f"TEXT_GRAD_CPU {GC.case_id(case)} restated vs modules {worst:.3e}; f32 "
          f"{max(GC.errors(GC.grads_of(case, 'f32'), g64).values()):.3e}; bf16 "
          f"{max(GC.errors(GC.grads_of(case, 'bf16'), g64).values()):.3e}")
    assert worst <= 1e-10
    for k, g in g64.items():
        if GC.is_zero_tensor(g):
            assert GC.is_zero_tensor(restated[k]), k


@pytest.mark.parametrize("tower", GC.TOWERS)
def test_the_oracle_agrees_with_central_differences_on_two_scalars(tower):
    """d sum(G * out) / d theta for one entry each of two tensors, central difference in fp64, 1e-6 relative."""
    case = GC.find(tower, 3, 11)
    ids, G = torch.from_numpy(GC.ids_of(case)), GC.grad_out(case).double()
    g64 = GC.oracle_grads(case)
    m = TC._double(tower)
    picks = [("txt_proj.weight", (3, 5))]
    if TC.TOWERS[tower][3] > 0:
        picks.append(("txt_enc.layers.0.linear1.weight", (7, 2)))
    else:
        picks.append(("txt_emb.weight", (int(GC.ids_of(case)[2, 0]), 1)))
    params = dict(m.named_parameters())
    for name, idx in picks:
        p = params[name]
        old = float(p.data[idx])
        h = 1e-5 * max(1.0, abs(old))
        vals = []
        for sign in (+1, -1):
            with torch.no_grad():
                p.data[idx] = old + sign * h
                vals.append(float((G * GC.module_out(m, ids)).sum()))
        with torch.no_grad():
            p.data[idx] = old
        fd, an = (vals[0] - vals[1]) / (2 * h), float(g64[name][idx])
        print(f"TEXT_GRAD_FD {tower} {name}{idx} autograd {an:.10e} central difference {fd:.10e}")
        assert an != 0.0 and abs(fd - an) <= 1e-6 * abs(an)


@pytest.mark.parametrize("case", GC.ALL_CASES, ids=GC.case_id)
def test_which_tensors_are_identically_zero(case):
    """Every tensor is non-zero - except on a call whose captions are all pads, where txt_proj.bias alone is."""
    g64 = GC.oracle_grads(case)
    zero = {k for k, g in g64.items() if GC.is_zero_tensor(g)}
    if all(p == "allpad" for p in case.pads):
        assert zero == set(g64) - {"txt_proj.bias"}
    else:
        assert zero == set()
    n_layer = TC.TOWERS[case.tower][3]
    assert len(g64) == 3 + 12 * n_layer
    for i in range(n_layer):
        assert tuple(g64[f"txt_enc.layers.{i}.self_attn.in_proj_bias"].shape) == (3 * TC.TOWERS[case.tower][0],)


def test_the_key_bias_third_of_in_proj_bias_is_zero_up_to_rounding():
    case = GC.find("e128", 5, 33)
    g = GC.oracle_grads(case)["txt_enc.layers.0.self_attn.in_proj_bias"]
    E = TC.TOWERS["e128"][0]
    assert float(g[E:2 * E].abs().max()) <= 1e-12 * float(g.abs().max())


@pytest.mark.parametrize("case", [GC.find("e128", 5, 33), GC.find("ref", 2, 16), GC.find("e128", 1, 4)] + GC.CRAFTED[:1],
                         ids=GC.case_id)
def test_sparse_rows_scatter_to_torchs_dense_embedding_gradient(case):
    """(distinct non-pad ids ascending, per-id sums in position order) -> dense equals txt_emb.weight.grad,
    the pad row zero."""
    from vcap.train_align import scatter_embedding_grad
    name, ids = case.tower, GC.ids_of(case)
    V, pad = TC.TOWERS[name][5], TC.PAD_ID[name]
    m = TC._double(name)
    t = torch.from_numpy(ids)
    x = m.txt_emb(t).detach().requires_grad_(True)
    out = GC.pool_normalize(m.txt_enc(x), t, pad, m.txt_proj.weight, m.txt_proj.bias)
    (dx0,) = torch.autograd.grad((GC.grad_out(case).double() * out).sum(), x, allow_unused=True)
    dx0 = torch.zeros_like(x) if dx0 is None else dx0
    flat, dx0 = ids.reshape(-1), dx0.reshape(-1, dx0.shape[-1])
    uniq = np.unique(flat[flat != pad])
    rows = torch.zeros(uniq.size, dx0.shape[1], dtype=torch.float64)
    for i, u in enumerate(uniq):
        for pos in np.nonzero(flat == u)[0]:
            rows[i] += dx0[pos]
    dense = scatter_embedding_grad((torch.from_numpy(uniq), rows), V)
    want = GC.oracle_grads(case)["txt_emb.weight"]
    assert dense.shape == want.shape and bool((dense[pad] == 0).all())
    assert torch.equal(dense, GC.dense_embedding_grad(torch.from_numpy(uniq), rows, V))
    scale = max(float(want.abs().max()), 1e-300)
    assert float((dense - want).abs().max()) <= 1e-12 * scale


def test_train_align_refuses_what_the_device_cannot_train():
    from scripts.train_align import build_argparser, check_args
    ap = build_argparser()
    check_args(ap.parse_args(["--model", "vit", "--freeze_vit"]))
    with pytest.raises(SystemExit, match="freeze_vit"):
        check_args(ap.parse_args(["--model", "vit"]))
    with pytest.raises(SystemExit, match="simple"):
        check_args(ap.parse_args(["--model", "simple", "--freeze_vit"]))
    with pytest.raises(SystemExit, match="max_len"):
        check_args(ap.parse_args(["--freeze_vit", "--max_len", "65"]))
    a = ap.parse_args(["--freeze_vit"])
    for flag in ("ann_train", "ann_val", "batch_size", "num_frame", "max_len", "lr", "epochs", "max_steps", "val_every",
                 "run_dir", "ckpt_dir", "ckpt_name", "freeze_vit", "weights_seed", "tokenizer_dir"):
        assert hasattr(a, flag), flag


def test_synthetic_alignment_weights_carry_the_references_names():
    from vcap.train_align import synthetic_align_state_dict
    sd = synthetic_align_state_dict(3, 768, 97, 5, 128, 2, 2, 64)
    assert set(TC.state_dict("e128")) | {"vid_proj.weight", "vid_proj.bias"} == set(sd)
    assert sd["vid_proj.weight"].shape == (64, 768) and not sd["txt_emb.weight"][5].any()
    again = synthetic_align_state_dict(3, 768, 97, 5, 128, 2, 2, 64)
    assert all(np.array_equal(sd[k], again[k]) for k in sd)
