"""Cost of the scoring call's backward (vcap_gpt2_score_backward) on GPT-2-small with seeded weights:
forward + backward of the new call against vcap_gpt2_score alone, and against torch eager autograd of the same
model on the same weights (HF GPT2LMHeadModel where transformers imports, otherwise the plain-torch
restatement of tests/score_cases.py; f32, and under bf16 autocast for the bf16 row).

Shapes: the training shape, 8 sequences x (4 prefix + 24 caption) positions, and 512 rows (16 x 32).  Rounds
are interleaved in one process; each timing is a pair of device events around the calls, read after a
synchronise; the figure is the median over the rounds.

  python tools/score_grad_bench.py [--rounds 20] [--out profiles/score_grad_bench.txt]
  rocprofv3 --kernel-trace --stats -- python tools/score_grad_bench.py --rounds 3 --no-torch   (per-kernel times)
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


def timed(fn, stream_dev):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize(stream_dev)
    return a.elapsed_time(b)


def torch_model(sd, arch, dev):
    """-> (callable(x, km, tg) doing forward + backward to x.grad, name)"""
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
        for p in model.parameters():
            p.requires_grad_(False)

        def run(x, km, tg):
            x = x.clone().requires_grad_(True)
            logits = model(inputs_embeds=x, attention_mask=km.long()).logits
            loss = F.cross_entropy(logits.float().reshape(-1, arch.vocab), tg.reshape(-1), ignore_index=-100,
                                   reduction="sum")
            loss.backward()
            return x.grad
        return run, f"HF GPT2LMHeadModel (transformers {transformers.__version__}) eager autograd"
    except ImportError:
        import score_cases as SC
        sdt = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in sd.items()}

        def run(x, km, tg):
            x = x.clone().requires_grad_(True)
            logits = SC.masked_forward(sdt, arch, x, km)
            loss = F.cross_entropy(logits.float().reshape(-1, arch.vocab), tg.reshape(-1), ignore_index=-100,
                                   reduction="sum")
            loss.backward()
            return x.grad
        return run, "plain-torch restatement (tests/score_cases.masked_forward) eager autograd"


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--no-torch", action="store_true", help="skip the torch baseline (profiling runs)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    from vcap import configs, weights
    from vcap.model import HipGPT2Decoder
    dev = torch.device("cuda:0")
    arch = configs.gpt2_arch("gpt2")
    sd = weights.synthetic_gpt2(1, arch)
    lines = [f"score_grad_bench: GPT-2-small ({arch.n_layer} layers, E {arch.n_embd}, V {arch.vocab}), seeded weights, "
             f"{torch.cuda.get_device_name(0)}, median of {args.rounds} interleaved rounds, ms"]
    base, base_name = (None, "") if args.no_torch else torch_model(sd, arch, dev)
    if base is not None:
        lines.append(f"torch baseline: {base_name}")
    for prec in ("fp32", "bf16"):
        dec = HipGPT2Decoder(sd, arch, prec, dev, screen=False)
        nbytes = dec.enable_grad(sd)
        lines.append(f"[{prec}] grad weight copies {nbytes / 2 ** 20:.0f} MiB")
        for name, B, S in SHAPES:
            g = torch.Generator().manual_seed(B * 1000 + S)
            x = (0.1 * torch.randn(B, S, arch.n_embd, generator=g)).to(dev)
            km = torch.ones(B, S, dtype=torch.uint8, device=dev)
            tg = torch.randint(0, arch.vocab, (B, S), generator=g).to(dev)
            tg[:, :4] = -100

            def fwd():
                dec.score(x, km, tg, check_mask=False)

            def fwd_bwd():
                dec.score_backward(x, km, tg, None, check_mask=False)

            def torch_fb():
                if prec == "bf16":
                    with torch.autocast("cuda", dtype=torch.bfloat16):
                        base(x, km.bool(), tg)
                else:
                    base(x, km.bool(), tg)

            runs = {"vcap_gpt2_score": fwd, "vcap_gpt2_score_backward": fwd_bwd}
            if base is not None:
                runs["torch fwd+bwd"] = torch_fb
            for fn in runs.values():      # warm-up: allocations, first launches
                fn()
                fn()
            torch.cuda.synchronize(dev)
            t = {k: [] for k in runs}
            for _ in range(args.rounds):
                for k, fn in runs.items():
                    t[k].append(timed(fn, dev))
            med = {k: statistics.median(v) for k, v in t.items()}
            row = f"[{prec}] {name:14s}  score {med['vcap_gpt2_score']:.3f}  score_backward (fwd+bwd) " \
                  f"{med['vcap_gpt2_score_backward']:.3f}  backward alone " \
                  f"{med['vcap_gpt2_score_backward'] - med['vcap_gpt2_score']:.3f}"
            if base is not None:
                row += f"  torch fwd+bwd {med['torch fwd+bwd']:.3f}  torch / device " \
                       f"{med['torch fwd+bwd'] / med['vcap_gpt2_score_backward']:.2f}x"
            lines.append(row)
            print(row, flush=True)
        del dec
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
