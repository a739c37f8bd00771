"""CPU side of the encoder shape sweep (test_gpu_encoder_shapes.py): everything that sweep's bounds rest on is
derived here from the fp64 oracle and the emulated forward alone, with no GPU in the loop (pytest -s prints
one line per case; profiles/encoder_shapes.txt keeps a copy).

  * the cases are the issue's table, B * T <= 8, and the emulated forward with its rounding switched off IS
    oracle.encoder + prefix_norm + mapper (1e-12);
  * the scaled q / k weights exercise the softmax: per block the scores q.k / 8 have std in [1, 4] and a
    median row max-probability in [0.05, 0.9];
  * the fp32 oracle's own error against fp64 is at most a third of the 1e-4 bar;
  * every bf16 / fp16 tolerance (3 x max |emulated - fp64|) is printed, and the fp16 bound on |gpu - emulated| is
    one a correct kernel can meet: the emulated forward run in f32 arithmetic meets it, and no output sits where
    f32 summation noise decides an fp16 rounding that the bound cannot absorb;
  * the fault table: each injected fault, where it is defined for the case, moves the fp64 enc_out by more
    than twice the fp32 bar - so the fp32 run of the sweep sees it.  In bf16 / fp16 only the dropped fc2
    K-tile and the missing frame are asserted to exceed the tolerance; which of the others do is printed.
    A padding key admitted to the softmax, an unwritten last row tile and (at some shapes) the last key
    dropped stay below it: the stated limit of a half-precision end-to-end check, and the reason for
    tests/test_gpu_attention_edges.py.

The fp8 sweep (encoder_shapes.FP8_RUNS; profiles/encoder_shapes_fp8.txt keeps the printed table):
  * the cases are the issue's, B * T <= 8, cases 24 - 26 with B = 2 so that a row encoded alone has fewer 256-row
    scale groups than the batch; the fp8 emulation with no MXFP8 GEMM selected IS the bf16 emulation;
  * every fp8 tolerance 3 x max |emulated - fp64| is printed and is below max |fp64 output| (0.11 .. 0.65 on
    outputs of max 1.4 .. 1.9: the bf16 / fp16 sanity bar of 0.25 does not apply);
  * the bound on |gpu - emulated|, tol / 3 + 1e-4, is met by the emulation run in f32 arithmetic in two
    summation orders (as written, and with the K axis of every matrix product reversed), so it does not rest on
    one sample of the e4m3 rounding flips that f32 noise sets off at 197 / 257 tokens (1e-3 .. 5e-2 there, 2e-7
    at 2 / 17 tokens); a run that missed would get another seed, chosen here on the CPU alone (none did);
  * the fault table: a missing frame exceeds the fp8 tolerance in every run; which of the others do is printed.
    One fault is fp8's own: K-block 0 of the last fc2 activation doubled, i.e. one scale byte off by one, moves
    the output by 0.09 .. 0.17, below the tolerance of every run with all four GEMMs in MXFP8.
  The end-to-end fp8 net cannot see that class of fault (at 197 / 257 tokens a wrong scale byte, a dropped fc2
  K-tile, a padding key and an unwritten row tile all stay below the tolerance): the tight net for this path is at the kernels,
  tests/test_gpu_mx_sweep.py and the mxfp8 runs of tests/test_gpu_attention_edges.py.
  * the descriptor of every run is served, and the fused QKV + attention kernel runs exactly where neither qkv nor
    attn-proj is MXFP8 (at 197 / 257 tokens)."""
import pytest
import torch

import encoder_shapes as S

IDS = [c.name for c in S.CASES]


def test_cases_are_the_table():
    got = [(c.dim, c.heads, c.patch, c.image, c.tokens, c.depth, c.B, c.T) for c in S.CASES]
    assert got == [(64, 1, 16, 16, 2, 2, 2, 3), (64, 1, 8, 32, 17, 2, 2, 3), (320, 5, 8, 40, 26, 2, 1, 1),
                   (128, 2, 16, 224, 197, 3, 2, 3), (192, 3, 16, 224, 197, 1, 2, 3), (192, 3, 16, 224, 197, 2, 2, 4),
                   (384, 6, 16, 224, 197, 2, 2, 3), (512, 8, 14, 224, 257, 2, 1, 3), (1024, 16, 16, 224, 197, 2, 1, 2),
                   (768, 12, 16, 224, 197, 2, 1, 2), (128, 2, 32, 224, 50, 2, 2, 3), (128, 2, 8, 64, 65, 2, 2, 3),
                   (128, 2, 16, 240, 226, 2, 1, 2)]
    assert all(c.B * c.T <= 8 and c.dim == 64 * c.heads for c in S.CASES)
    assert [c.precs for c in S.CASES] == [S.PRECS] * 10 + [("fp16",)] * 3
    assert len(S.RUNS) == 33 and S.REFUSED == [(i, p) for i in (11, 12, 13) for p in ("fp32", "bf16")]
    c3, c7 = S.BY_ID[3], S.BY_ID[7]
    assert c3.arch.mlp == 640 and (c7.video_dim, c7.prefix) == (100, (3, 40))
    assert (c7.prefix[0] * c7.prefix[1]) % 64 != 0 and c7.video_dim % 16 != 0


def test_rounding_is_to_nearest_even():
    x = torch.tensor([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -20, -3.0], dtype=torch.float64)
    assert S.ROUND["bf16"](x).tolist() == [1.0, 1.0 + 2.0 ** -6, 1.0 + 2.0 ** -7, -3.0]
    y = torch.tensor([1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 2.0 ** -25, 70000.0], dtype=torch.float64)
    assert S.ROUND["fp16"](y).tolist() == [1.0, 1.0 + 2.0 ** -9, 0.0, float("inf")]
    assert S.ROUND["fp64"](x) is x


@pytest.mark.parametrize("c", S.CASES, ids=IDS)
def test_case_bounds_and_fault_table(c):
    cid = c.cid
    stats = []
    ref = S.forward(cid, "fp64", stats=stats)
    for (nm, a), (_, b) in zip(S.outputs(ref), S.outputs(S.reference(cid))):
        assert torch.equal(a, b), nm                       # the shared reference is this forward
    # identity rounding reproduces the oracle
    orc = S.oracle(cid)
    ident = max(S._maxdiff(a, b) for (_, a), (_, b) in zip(S.outputs(ref), S.outputs(orc)))
    assert len(S.outputs(ref)) == (2 if c.prefix else 1) and ident < 1e-12, ident
    assert ref[0].shape == (c.B, c.video_dim) and (not c.prefix or ref[1].shape == (c.B,) + c.prefix)
    # the softmax is exercised in every block
    assert len(stats) == c.depth
    for std, maxp in stats:
        assert S.SCORE_STD[0] <= std <= S.SCORE_STD[1], (c.name, stats)
        assert S.MAXP_MEDIAN[0] <= maxp <= S.MAXP_MEDIAN[1], (c.name, stats)
    # the fp32 oracle's own error leaves two thirds of the bar to the kernels
    o32 = S.oracle(cid, torch.float32)
    e32 = [S._maxdiff(a, b) for (_, a), (_, b) in zip(S.outputs(o32), S.outputs(orc))]
    assert max(e32) <= S.FP32_TOL / 3, e32
    tols = {m: S.tolerance(cid, m) for m in ("bf16", "fp16")}
    print(f"\nencoder-cpu {c.name} qk={S.qk_scale(c):.3f} scores(std, median maxp)="
          f"{[(round(a, 2), round(b, 3)) for a, b in stats]} ident={ident:.1e} "
          f"fp32-oracle-err={'/'.join(f'{e:.1e}' for e in e32)} (bar {S.FP32_TOL:.0e}) "
          + " ".join(f"tol_{m}={'/'.join(f'{t:.3e}' for t in tols[m] if t is not None)}" for m in tols), end="")
    for m in tols:
        assert all(t is None or (0 < t < 0.25) for t in tols[m]), tols   # finite, and not a bound that admits anything
    # the fp16 bound on |gpu - emulated| is not at the mercy of one output ulp (encoder_shapes.fp16_tie_margin)
    margin, noise = S.fp16_tie_margin(cid)
    print(f"\nencoder-cpu {c.name} fp16 output ties: margin {margin:.2e}, f32-arithmetic noise {noise:.2e}", end="")
    assert margin > 4 * noise, (c.name, margin, noise)
    e32a = S.forward(cid, "fp16", arith=torch.float32)
    for i, ((nm, a), (_, b)) in enumerate(zip(S.outputs(e32a), S.outputs(S.emulated(cid, "fp16")))):
        assert S._maxdiff(a, b) <= tols["fp16"][i] / 3 + 1e-4, (c.name, nm)
    # fault table (fp64 forward, enc_out)
    moves = {}
    for f in S.FAULTS:
        if S.fault_defined(c, f):
            moves[f] = S._maxdiff(S.forward(cid, "fp64", fault=f)[0], ref[0])
            assert moves[f] > 2 * S.FP32_TOL, (c.name, f, moves[f])
    print(f"\nencoder-cpu {c.name} faults: " + " ".join(f"{f}={v:.2e}" for f, v in moves.items()), end="")
    for m in tols:
        if m in c.precs:
            tol = tols[m][0]
            seen = [f for f, v in moves.items() if v > tol]
            print(f"\nencoder-cpu {c.name} {m}: above tol {seen}; below {[f for f in moves if f not in seen]}", end="")
            for f in S.ASSERTED_16:
                assert moves[f] > tol, (c.name, m, f, moves[f], tol)


def test_generic_kernel_window_rule_and_fusion_table():
    assert [S.generic_attention("fp16", n) for n in (17, 32, 33, 50, 192, 193, 224, 225, 256, 257, 288)] == \
           [False, False, True, True, True, False, False, True, True, False, False]
    assert not S.generic_attention("bf16", 50)
    assert [S.expect_fused(c, "bf16") for c in S.CASES] == [False] * 3 + [True] * 7 + [False] * 3
    assert not any(S.expect_fused(c, "fp32") for c in S.CASES)


@pytest.mark.parametrize("run", S.RUNS + S.REFUSED, ids=S.run_id)
def test_descriptor_is_served_or_refused_up_front(run):
    """Every run of the sweep has a workspace; cases 11 - 13 outside fp16 are refused by the descriptor check
    (UNSUPPORTED, workspace 0) - the text is pinned in test_cpu_abi_refusals.py.  No GPU: nothing launches."""
    import ctypes as C

    from vcap import _native as N
    c, prec = S.BY_ID[run[0]], run[1]
    dt = {"fp32": N.DT_F32, "bf16": N.DT_BF16, "fp16": N.DT_F16}[prec]
    buf = C.create_string_buffer(64)
    p = C.addressof(buf)
    layers = (N.VitLayer * c.depth)()
    kstep = 32 if prec == "fp32" else 64
    ar = c.arch
    desc = N.VitDesc(dtype=dt, dim=ar.dim, depth=ar.depth, heads=ar.heads, patch=ar.patch, image=ar.image, mlp=ar.mlp,
                     video_dim=c.video_dim, kpad=-(-ar.patch_k // kstep) * kstep, ln_eps=ar.ln_eps, patch_w=p, patch_b=p,
                     cls=p, pos=p, norm_g=p, norm_b=p, proj_w=p, proj_b=p, layers=layers)
    ws = int(N.lib().vcap_vit_workspace_bytes(C.byref(desc), c.B, c.T))
    fuses = int(N.lib().vcap_vit_layer_fuses_qkv_attention(C.byref(desc), 0))
    if run in S.REFUSED:
        assert ws == 0 and fuses == N.E_UNSUPPORTED
        assert "fp16 only" in N.lib().vcap_last_error().decode()
    else:
        assert ws > 0 and fuses == int(S.expect_fused(c, prec))


def test_fp8_cases_are_the_table():
    got = [(c.dim, c.heads, c.tokens, c.depth, c.B, c.T) for c in S.FP8_CASES]
    assert got == [(256, 4, 2, 2, 2, 3), (256, 4, 17, 1, 2, 2), (256, 4, 197, 2, 1, 2), (512, 8, 257, 2, 2, 2),
                   (768, 12, 197, 2, 2, 2), (1024, 16, 197, 2, 2, 2)]
    # the row-alone check changes the number of 256-row scale groups at 257 tokens and at 197 tokens
    groups = lambda rows: -(-rows // 256)
    for cid, (batch, alone) in ((24, (5, 3)), (25, (4, 2)), (26, (4, 2))):
        c = S.BY_ID[cid]
        assert c.B == 2 and (groups(c.B * c.T * c.tokens), groups(c.T * c.tokens)) == (batch, alone)
    assert all(c.B * c.T <= 8 and c.dim == 64 * c.heads and c.dim % 256 == 0 for c in S.FP8_CASES)
    for a, b in ((24, 8), (25, 10), (26, 9)):                  # the architectures of cases 8, 10 and 9
        x, y = S.BY_ID[a].arch, S.BY_ID[b].arch
        assert (x.dim, x.depth, x.heads, x.patch, x.image, x.mlp_ratio) == (y.dim, y.depth, y.heads, y.patch, y.image, y.mlp_ratio)
    assert len(S.FP8_RUNS) == 11 and [r[1] for r in S.FP8_RUNS if r[0] == 23][1:] == list(S.FP8_MIXES)
    assert not set(S.BY_ID[r[0]].cid for r in S.FP8_RUNS) & {c.cid for c in S.CASES}


def test_mxq_is_the_oracle_quantiser():
    import numpy as np

    from oracle import vcap_oracle as O
    g = torch.Generator().manual_seed(5)
    x = torch.randn(7, 256, dtype=torch.float64, generator=g) * \
        torch.exp2(torch.randint(-12, 12, (7, 8, 1), generator=g).double()).repeat(1, 1, 32).reshape(7, 256)
    x[0, :32] = 0
    x = x.float().double()
    q, sb = O.mx_quantize(x.float().numpy())
    assert np.array_equal(S.mxq(x).numpy(), O.mx_dequantize(q, sb).astype(np.float64))


@pytest.mark.parametrize("run", S.FP8_RUNS, ids=S.fp8_run_id)
def test_fp8_bounds_and_fault_table(run):
    cid, mx = run
    c = S.BY_ID[cid]
    tag = S.fp8_run_id(run)
    ref, emu = S.reference(cid)[0], S.emulated_fp8(cid, mx)[0]
    tol = S.tolerance_fp8(cid, mx)
    assert 0 < tol < float(ref.abs().max()), (tag, tol)
    if mx == S.MX_GEMMS:                                       # nothing selected: the bf16 emulation, bit for bit
        assert torch.equal(S.forward(cid, "fp8", mx_gemms=())[0], S.forward(cid, "bf16")[0])
    noise = []
    for kflip in (False, True):
        e32 = S.forward(cid, "fp8", mx_gemms=mx, arith=torch.float32, kflip=kflip)[0]
        noise.append(S._maxdiff(e32, emu))
        assert noise[-1] <= tol / 3 + 1e-4, (tag, kflip, noise[-1], tol / 3 + 1e-4)
        assert S._maxdiff(e32, ref) < tol, (tag, kflip)
    print(f"\nencoder-cpu {tag}: tol_fp8={tol:.3e} max|fp64|={float(ref.abs().max()):.3f} bound|gpu-emulated|={tol / 3 + 1e-4:.3e} "
          f"f32-arithmetic noise {noise[0]:.2e} (K reversed {noise[1]:.2e})", end="")
    moves = {}
    for f in S.FAULTS + ("fc2_scale",):
        if S.fault_defined(c, f):
            moves[f] = S._maxdiff(S.forward(cid, "fp64", fault=f)[0], ref)
    seen = [f for f, v in moves.items() if v > tol]
    print(f"\nencoder-cpu {tag} faults: " + " ".join(f"{f}={v:.2e}" for f, v in moves.items()) +
          f"; above tol {seen}; below {[f for f in moves if f not in seen]}", end="")
    assert moves["frame_missing"] > tol, (tag, moves["frame_missing"], tol)
    assert moves["fc2_scale"] > 2 * S.FP32_TOL


@pytest.mark.parametrize("run", S.FP8_RUNS + [(23, ())], ids=S.fp8_run_id)
def test_fp8_descriptor_is_served_and_fuses_where_it_should(run):
    """No GPU: the descriptor check and the fusion predicate only.  A descriptor with dtype MXFP8 and no weight
    scales at all (mx_gemms = ()) is accepted: every GEMM of it is the bf16 one."""
    import ctypes as C

    from vcap import _native as N
    c, mx = S.BY_ID[run[0]], run[1]
    buf = C.create_string_buffer(64)
    p = C.addressof(buf)
    layers = (N.VitLayer * c.depth)()
    for ly in layers:
        for g in mx:
            setattr(ly, g + "_ws", p)
    ar = c.arch
    desc = N.VitDesc(dtype=N.DT_MXFP8, dim=ar.dim, depth=ar.depth, heads=ar.heads, patch=ar.patch, image=ar.image,
                     mlp=ar.mlp, video_dim=c.video_dim, kpad=-(-ar.patch_k // 64) * 64, ln_eps=ar.ln_eps, patch_w=p,
                     patch_b=p, cls=p, pos=p, norm_g=p, norm_b=p, proj_w=p, proj_b=p, layers=layers)
    assert int(N.lib().vcap_vit_workspace_bytes(C.byref(desc), c.B, c.T)) > 0
    for layer in range(c.depth):
        assert int(N.lib().vcap_vit_layer_fuses_qkv_attention(C.byref(desc), layer)) == int(S.expect_fused_fp8(c, mx))
    assert S.expect_fused_fp8(c, mx) == (c.tokens in (197, 257) and not {"qkv", "proj"} & set(mx))
