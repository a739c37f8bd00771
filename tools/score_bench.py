"""Teacher-forced scoring cost: GPT-2 small, seeded weights, bf16 and fp32 decoders, at the bench caption
shape (B = 8, S = 28: 4 prefix + 24 tokens) and at vcap_gpt2_max_rows() (B = 8, S = 64: 512 rows).

Three lines per (precision, shape), timed in one process after a warm-up, interleaved over the rounds
(host clock around work that ends in a device synchronise):
  (a) HipGPT2Decoder.score without logits      one vcap_gpt2_score pass -> log-probs + loss pair
  (b) the same with [B, S, V] logits stored
  (c) the step-wise way to the same numbers    fidelity.teacher_forced_logits along the same tokens (one
                                               launch chain + one lm_head stream per position), then torch
                                               log_softmax + gather
It also checks that (a) and (c) agree.  `--only a --rounds N` runs line (a) alone, for a profiler run of
its kernels (rocprofv3 --kernel-trace --stats -- python tools/score_bench.py --only a): the lm_head +
cross-entropy kernel is vcap_score_lm_kernel, whose floors the last lines print: V * E weight bytes once
from HBM, and 2 * rows * V * E FLOP at the dense MFMA peak."""
import argparse
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "video-caption-algorithm_amd"))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from vcap import configs, fidelity, weights  # noqa: E402
from vcap.model import HipGPT2Decoder  # noqa: E402

HBM_BYTES_S = 6.29e12                               # measured float4 copy rate of the MI355X
PEAK_FLOPS = {"bf16": 2.5e15, "fp32": 157.3e12}     # dense MFMA peaks (fp32: the f32-input MFMA)
SHAPES = [(8, 28), (8, 64)]
P = 4


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--only", choices=["a", "b", "c"], default=None)
    ap.add_argument("--precisions", default="bf16,fp32")
    args = ap.parse_args()
    ga = configs.gpt2_arch("gpt2")
    dev = torch.device("cuda:0")
    sd = weights.synthetic_gpt2(1, ga)
    for prec in args.precisions.split(","):
        dec = HipGPT2Decoder(sd, ga, prec, dev, screen=False)
        for B, S in SHAPES:
            g = torch.Generator().manual_seed(S)
            prefix = (0.1 * torch.randn(B, P, ga.n_embd, generator=g)).to(dev)
            toks = torch.randint(0, ga.vocab - 1, (B, S - P), generator=g).to(dev)   # prompt token + S - P - 1 steps
            prompt, steps = [int(ga.bos_token_id)], S - P
            ids = torch.cat([torch.full((B, 1), prompt[0], device=dev), toks[:, :-1]], dim=1)
            x = torch.cat([prefix, dec.wte[ids].float()], dim=1)                      # [B, S, E]
            # position P + k (input: the prompt token, then toks[:, k - 1]) predicts toks[:, k]
            tgt = torch.full((B, S), -100, device=dev)
            tgt[:, P:] = toks

            def line_a():
                return dec.score(x, None, tgt)

            def line_b():
                return dec.score(x, None, tgt, want_logits=True)

            def line_c():
                lg = fidelity.teacher_forced_logits(dec, prefix, prompt, toks, steps)    # [steps, B, V]
                lp = F.log_softmax(lg.float(), dim=-1).gather(2, toks.t()[..., None])[..., 0]
                return lp.t()

            lines = {"a": line_a, "b": line_b, "c": line_c}
            if args.only:
                lines = {args.only: lines[args.only]}
            else:
                lp_a, lp_c = line_a().logprobs[:, P:], line_c()
                print(f"{prec} B={B} S={S}: max |logprob (a) - (c)| = {float((lp_a - lp_c).abs().max()):.3e}")
            for fn in lines.values():
                for _ in range(2):
                    fn()
            ms = {k: [] for k in lines}
            for _ in range(args.rounds):
                for k, fn in lines.items():
                    ms[k].append(timed(fn))
            for k, v in ms.items():
                print(f"{prec} B={B} S={S} rows={B * S} ({k}): median {statistics.median(v):8.3f} ms   "
                      f"min {min(v):8.3f} ms   ({len(v)} rounds)", flush=True)
            es = 2 if prec == "bf16" else 4
            wbytes, flop = ga.vocab * ga.n_embd * es, 2.0 * B * S * ga.vocab * ga.n_embd
            print(f"{prec} rows={B * S} vcap_score_lm_kernel floors: weights {wbytes / 1e6:.1f} MB once = "
                  f"{wbytes / HBM_BYTES_S * 1e6:.1f} us at {HBM_BYTES_S / 1e12:.2f} TB/s; {flop / 1e9:.1f} GFLOP = "
                  f"{flop / PEAK_FLOPS[prec] * 1e6:.1f} us at the dense peak", flush=True)
        del dec
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
