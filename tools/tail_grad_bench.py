"""Cost of GPT-2 tail fine-tuning on the device (vcap_gpt2_score_backward_tail) on GPT-2-small with seeded
weights, tools/score_grad_bench.py's method: one process, interleaved rounds, every timing a pair of device
events around the calls read after a synchronise, the figure the median over the rounds.

  1. The product alone (vcap_gpt2_weight_grad = vcap_gpt2_dw_kernel): GPT-2-small's four dW shapes at M = 224
     (8 x 28) and M = 512, bf16 and f32, against torch.matmul(X.t(), dY) on the same operands and dtype and
     against the product's byte floor (M (K + N) es + K N 4) / 6.0 TB/s (the chip's measured in-order sweep
     rate, tools/retrieval_bench.py).  Each timing covers INNER back-to-back launches.
  2. The call: forward + backward with n_tail 0 (= vcap_gpt2_score_backward), 2 and 12 at both shapes and
     precisions, against torch eager autograd of the same model with the last N blocks requiring grad (HF
     GPT2LMHeadModel where transformers imports, otherwise tests/score_cases.masked_forward; bf16 rows under
     autocast).  Per unfrozen layer the call adds 10 launches (4 products, 4 bias column sums, 2 LayerNorm
     column sums; the two LayerNorm backwards it already had gain a stats store) and 2 device copies.
  3. One training step's load_tail refresh for N = 2.
  4. --accuracy FILE: every case of tests/tail_grad_cases.py x precision at n_tail = 2, the worst tensor's
     error / bound per case.

  python tools/tail_grad_bench.py [--rounds 20] [--out profiles/tail_grad_bench.txt]
                                  [--accuracy profiles/tail_grad_accuracy.txt]
"""
from __future__ import annotations

import argparse
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
for _p in (ROOT / "video-caption-algorithm_amd", ROOT, ROOT / "tests"):
    if str(_p) not in sys.path:
        sys.path.insert(0, str(_p))

import numpy as np  # noqa: E402
import torch  # noqa: E402

SHAPES = [("train 8x28", 8, 28), ("rows512 16x32", 16, 32)]
HBM_SWEEP_BYTES_S = 6.0e12
INNER = 20


def timed(fn, dev):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize(dev)
    return a.elapsed_time(b)


def interleaved(runs, rounds, dev):
    for fn in runs.values():      # warm-up: allocations, first launches
        fn()
        fn()
    torch.cuda.synchronize(dev)
    t = {k: [] for k in runs}
    for _ in range(rounds):
        for k, fn in runs.items():
            t[k].append(timed(fn, dev))
    return {k: statistics.median(v) for k, v in t.items()}


def kernel_rows(arch, rounds, dev, lines):
    from vcap import _native as N
    E = arch.n_embd
    products = [("c_attn  [E,3E]", E, 3 * E), ("a.c_proj [E,E]", E, E), ("c_fc    [E,4E]", E, 4 * E),
                ("m.c_proj [4E,E]", 4 * E, E)]
    lines.append(f"-- the product alone, us per launch (median of {rounds} rounds of {INNER} back-to-back launches); "
                 f"floor = (M (K + N) es + 4 K N) / {HBM_SWEEP_BYTES_S / 1e12:.1f} TB/s")
    stream = torch.cuda.current_stream(dev).cuda_stream
    for prec, dt, tdt in (("bf16", N.DT_BF16, torch.bfloat16), ("fp32", N.DT_F32, torch.float32)):
        for M in (224, 512):
            for name, K, Nn in products:
                g = torch.Generator().manual_seed(M + K + Nn)
                X = torch.randn(M, K, generator=g).to(dev, tdt)
                dY = torch.randn(M, Nn, generator=g).to(dev, tdt)
                out = torch.empty(K, Nn, device=dev)

                def ours():
                    for _ in range(INNER):
                        N.lib().vcap_gpt2_weight_grad(dt, X.data_ptr(), dY.data_ptr(), out.data_ptr(), M, K, Nn, stream)

                def torch_mm():
                    for _ in range(INNER):
                        torch.matmul(X.t(), dY)

                med = interleaved({"ours": ours, "torch": torch_mm}, rounds, dev)
                ref = torch.matmul(X.double().t(), dY.double())
                err = float((out.double() - ref).abs().max() / ref.abs().max())
                es = X.element_size()
                floor_us = (M * (K + Nn) * es + 4 * K * Nn) / HBM_SWEEP_BYTES_S * 1e6
                us, tus = med["ours"] / INNER * 1e3, med["torch"] / INNER * 1e3
                row = (f"[{prec}] M={M:3d} {name:15s} dw_kernel {us:7.1f}  torch.matmul(X.t(), dY) {tus:7.1f}  "
                       f"torch / ours {tus / us:5.2f}x  floor {floor_us:5.2f}  ours / floor {us / floor_us:6.1f}x  "
                       f"max err vs fp64 {err:.1e}")
                lines.append(row)
                print(row, flush=True)


def torch_model(sd, arch, dev):
    """-> (run(x, km, tg, n_tail): forward + backward to x.grad and the tail's .grad, name)"""
    import torch.nn.functional as F
    try:
        import transformers
        cfg = transformers.GPT2Config(vocab_size=arch.vocab, n_positions=arch.n_positions, n_embd=arch.n_embd,
                                      n_layer=arch.n_layer, n_head=arch.n_head, activation_function="gelu_new",
                                      resid_pdrop=0.0, embd_pdrop=0.0, attn_pdrop=0.0, layer_norm_epsilon=arch.ln_eps)
        model = transformers.GPT2LMHeadModel(cfg).eval()
        pre = "decoder.model."
        model.load_state_dict({k[len(pre):]: torch.from_numpy(np.ascontiguousarray(v)) for k, v in sd.items()
                               if k.startswith(pre)}, strict=False)
        model = model.to(dev)

        def run(x, km, tg, n_tail):
            for p in model.parameters():
                p.requires_grad_(False)
                p.grad = None
            for block in model.transformer.h[arch.n_layer - n_tail:]:
                for p in block.parameters():
                    p.requires_grad_(True)
            x = x.clone().requires_grad_(True)
            logits = model(inputs_embeds=x, attention_mask=km.long()).logits
            F.cross_entropy(logits.float().reshape(-1, arch.vocab), tg.reshape(-1), ignore_index=-100,
                            reduction="sum").backward()
            return x.grad
        return run, f"HF GPT2LMHeadModel (transformers {transformers.__version__}) eager autograd"
    except ImportError:
        import score_cases as SC
        sdt = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in sd.items()}

        def run(x, km, tg, n_tail):
            for k, t in sdt.items():
                t.grad = None
                t.requires_grad_(any(k.startswith(f"{SC.P}h.{i}.") for i in range(arch.n_layer - n_tail, arch.n_layer)))
            x = x.clone().requires_grad_(True)
            logits = SC.masked_forward(sdt, arch, x, km)
            F.cross_entropy(logits.float().reshape(-1, arch.vocab), tg.reshape(-1), ignore_index=-100,
                            reduction="sum").backward()
            return x.grad
        return run, "plain-torch restatement (tests/score_cases.masked_forward) eager autograd"


def call_rows(sd, arch, rounds, dev, lines, no_torch):
    from vcap.model import HipGPT2Decoder
    base, base_name = (None, "") if no_torch else torch_model(sd, arch, dev)
    lines.append(f"-- the call, forward + backward, ms (median of {rounds} interleaved rounds)")
    if base is not None:
        lines.append(f"torch baseline: {base_name}, the last N blocks requiring grad")
    tails = (0, 2, arch.n_layer)
    for prec in ("fp32", "bf16"):
        dec = HipGPT2Decoder(sd, arch, prec, dev, screen=False)
        dec.enable_grad(sd)
        for name, B, S in SHAPES:
            g = torch.Generator().manual_seed(B * 1000 + S)
            x = (0.1 * torch.randn(B, S, arch.n_embd, generator=g)).to(dev)
            km = torch.ones(B, S, dtype=torch.uint8, device=dev)
            tg = torch.randint(0, arch.vocab, (B, S), generator=g).to(dev)
            tg[:, :4] = -100
            runs = {}
            for n in tails:
                if n == 0:
                    runs["dev 0"] = lambda: dec.score_backward(x, km, tg, None, check_mask=False)
                else:
                    runs[f"dev {n}"] = lambda n=n: dec.score_backward_tail(x, km, tg, None, n, check_mask=False)
                if base is not None:
                    def torch_fb(n=n):
                        if prec == "bf16":
                            with torch.autocast("cuda", dtype=torch.bfloat16):
                                base(x, km.bool(), tg, n)
                        else:
                            base(x, km.bool(), tg, n)
                    runs[f"torch {n}"] = torch_fb
            med = interleaved(runs, rounds, dev)
            row = f"[{prec}] {name:14s}"
            for n in tails:
                row += f"  n_tail {n:2d}: device {med[f'dev {n}']:.3f}"
                if base is not None:
                    row += f" torch {med[f'torch {n}']:.3f} ({med[f'torch {n}'] / med[f'dev {n}']:.2f}x)"
            row += (f"  | added per unfrozen layer: {(med['dev 2'] - med['dev 0']) / 2 * 1e3:.0f} us (N = 2), "
                    f"{(med[f'dev {arch.n_layer}'] - med['dev 0']) / arch.n_layer * 1e3:.0f} us (N = {arch.n_layer})")
            lines.append(row)
            print(row, flush=True)
        # one training step's device-weight refresh, N = 2
        names = dec.tail_names(2)
        state = {k: torch.from_numpy(np.ascontiguousarray(sd[k], np.float32)).to(dev) for k in names}
        med = interleaved({"load_tail": lambda: dec.load_tail(state)}, rounds, dev)
        row = (f"[{prec}] load_tail, N = 2 ({sum(v.numel() for v in state.values()) / 1e6:.1f} M parameters, f32 masters on "
               f"the device, synchronise included): {med['load_tail']:.3f} ms")
        lines.append(row)
        print(row, flush=True)
        del dec
        torch.cuda.empty_cache()


def accuracy(path):
    import score_cases as SC
    import tail_grad_cases as TG
    from vcap.model import HipGPT2Decoder
    lines = ["tail_grad accuracy: per case and precision at n_tail = 2, err = max |g - g64| / max |g64| per parameter "
             "tensor against the fp64 autograd oracle; bound = 10 x CPU float32 autograd's error (fp32), 3 x the bf16 "
             "emulation's (bf16); the tensor with the largest err / bound is shown"]
    for prec in ("fp32", "bf16"):
        for c in TG.CASES:
            dec = HipGPT2Decoder(SC.state_dict(c.E, c.V), SC.arch(c.E, c.V), prec, "cuda", screen=False)
            dec.enable_grad(SC.state_dict(c.E, c.V))
            x, km, tg, w = TG.inputs(c)
            _, _, pg = dec.score_backward_tail(x, km, tg, w, 2)
            g64, tol = TG.oracle(c), TG.tolerance(c, "rand", prec)
            worst = max(pg, key=lambda k: TG.err(pg[k].cpu(), g64[k]) / tol[k])
            e = TG.err(pg[worst].cpu(), g64[worst])
            lines.append(f"[{prec}] {c.name:14s} M={c.B * c.S:3d} E={c.E:4d}  worst {worst[len(TG.P):]:24s} err {e:.3e} "
                         f"bound {tol[worst]:.3e} err/bound {e / tol[worst]:.3f}")
            print(lines[-1], flush=True)
            del dec
    Path(path).parent.mkdir(parents=True, exist_ok=True)
    Path(path).write_text("\n".join(lines) + "\n")


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--no-torch", action="store_true", help="skip the torch baselines of the call (profiling runs)")
    ap.add_argument("--out", default="")
    ap.add_argument("--accuracy", default="", help="also write the accuracy sweep to this file")
    args = ap.parse_args()
    from vcap import configs, weights
    dev = torch.device("cuda:0")
    arch = configs.gpt2_arch("gpt2")
    sd = weights.synthetic_gpt2(1, arch)
    lines = [f"tail_grad_bench: GPT-2-small ({arch.n_layer} layers, E {arch.n_embd}, V {arch.vocab}), seeded weights, "
             f"{torch.cuda.get_device_name(0)}"]
    kernel_rows(arch, args.rounds, dev, lines)
    call_rows(sd, arch, args.rounds, dev, lines, args.no_torch)
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text)
    if args.accuracy:
        accuracy(args.accuracy)
    return 0


if __name__ == "__main__":
    sys.exit(main())
