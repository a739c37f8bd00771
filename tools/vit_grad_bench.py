"""ViT training cost: HipViTEncoder.encode_backward (one vcap_vit_encode_backward call per chunk: forward +
backward, every gradient of the last n_tail blocks) of ViT-B/16 at B x T = 2 x 8 and 8 x 16 frames, n_tail in
{2, 12}, f32 and bf16 operands.

Two lines per cell, timed in one process after a warm-up with device events around `reps` back-to-back calls,
interleaved ABAB over the rounds, medians reported:
  ours   one encode_backward call on device frames and a device grad_out
  step   what a training step through vcap.train_align.EncodeVideo pays on the device for the encoder: one
         encode (the autograd forward) and then encode_backward, which runs the forward again
  torch  torch-ROCm's own eager autograd of the same architecture and weights on the same device
         (oracle.vcap_oracle.encoder over device parameters; only the parameters ours trains require grad):
         forward, sum(G * out).backward().  float32, or under torch.autocast(bfloat16) for the bf16 row.
Every cell is reported, the ones torch wins included.  Also: the attention-backward kernels alone
(vcap_vit_attention_backward at 16 frames x 197 tokens x 12 heads) against their algorithmic FLOP floor (5
products of 2 N^2 64 per frame and head at the MFMA peak) and byte floor (q | k | v and dO read, dq | dk | dv
written once, at the HBM peak); the cost per unfrozen block, (n_tail 12 - n_tail 2) / 10; and the per-step
in-place refresh of the device operands from f32 masters (load_state_dict).

    python tools/vit_grad_bench.py --out profiles/vit_grad_bench.txt
"""
import argparse
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "video-caption-algorithm_amd"))
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))
import torch  # noqa: E402

from oracle import vcap_oracle as O  # noqa: E402
from text_encode_bench import event_ms  # noqa: E402
from vcap import _native as N  # noqa: E402
from vcap import configs, weights  # noqa: E402
from vcap.model import HipViTEncoder  # noqa: E402

PEAK_FLOPS = {"f32": 157.3e12, "bf16": 2.5e15}   # MI355X dense MFMA peaks (f32 16x16x4, bf16 16x16x32)
PEAK_BYTES = 8.0e12                              # HBM3E


def attention_alone(dtype, dev, frames=16, tokens=197, heads=12, reps=20):
    dt, tdt = {"f32": (N.DT_F32, torch.float32), "bf16": (N.DT_BF16, torch.bfloat16)}[dtype]
    lib = N.lib()
    D = 64 * heads
    qkv = torch.randn(frames * tokens, 3 * D, device=dev).to(tdt)
    dout = torch.randn(frames * tokens, D, device=dev)
    dqkv = torch.empty(frames * tokens, 3 * D, device=dev)
    ws = torch.empty(int(lib.vcap_vit_attention_backward_workspace_bytes(dt, frames, tokens, heads)),
                     dtype=torch.uint8, device=dev)
    s = torch.cuda.current_stream().cuda_stream

    def call():
        N.check(lib.vcap_vit_attention_backward(dt, qkv.data_ptr(), dout.data_ptr(), dqkv.data_ptr(), frames, tokens,
                                                heads, ws.data_ptr(), s), "vcap_vit_attention_backward")

    event_ms(call, 3)
    ms = statistics.median(event_ms(call, reps) for _ in range(5))
    flops = 5 * 2.0 * tokens * tokens * 64 * frames * heads
    nbytes = frames * tokens * (3 * D * qkv.element_size() + D * 4 + 3 * D * 4)
    return ms, flops / PEAK_FLOPS[dtype] * 1e3, nbytes / PEAK_BYTES * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--shapes", default="2x8,8x16")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    arch = configs.vit_arch("vit_base_patch16_224")
    sd = weights.synthetic_vit(1, arch)
    shapes = [tuple(int(v) for v in s.split("x")) for s in args.shapes.split(",")]
    emit(f"# {torch.cuda.get_device_name(0)}; {arch.name}; forward + backward, medians of {args.rounds} interleaved "
         f"rounds of {args.reps} calls; one box, one run")
    emit(f"# {'dtype':5} {'BxT':>6} {'n_tail':>6} {'ours ms':>10} {'torch ms':>10} {'ours/torch':>10} {'step ms':>10} {'step/torch':>10} {'chunk clips':>11}")
    for dtype, prec in (("f32", "fp32"), ("bf16", "bf16")):
        enc = HipViTEncoder(sd, arch, prec, dev)
        enc.enable_grad(sd, arch.depth)
        params = {k: torch.from_numpy(v).to(dev) for k, v in sd.items()}
        per_tail = {}
        for B, T in shapes:
            g = torch.Generator().manual_seed(B * 100 + T)
            video = torch.randn(B, T, 3, arch.image, arch.image, generator=g).to(dev)
            G = torch.randn(B, enc.video_dim, generator=g).to(dev)
            for n_tail in (2, 12):
                names = enc.param_names(n_tail)
                for k, p in params.items():
                    p.requires_grad_(k in names)
                    p.grad = None

                def ours():
                    enc.encode_backward(video, G, n_tail)

                def step():
                    enc.encode(video)
                    enc.encode_backward(video, G, n_tail)

                def base():
                    for k in names:
                        params[k].grad = None
                    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=(dtype == "bf16")):
                        out = O.encoder(params, arch, video)
                    (G * out).sum().backward()

                for fn in (ours, base):
                    event_ms(fn, 1)
                t = {"ours": [], "step": [], "torch": []}
                for _ in range(args.rounds):
                    t["ours"].append(event_ms(ours, args.reps))
                    t["step"].append(event_ms(step, args.reps))
                    t["torch"].append(event_ms(base, args.reps))
                o, st, r = (statistics.median(t[k]) for k in ("ours", "step", "torch"))
                per_tail[(B, T, n_tail)] = o
                emit(f"  {dtype:5} {f'{B}x{T}':>6} {n_tail:6d} {o:10.3f} {r:10.3f} {o / r:10.2f} {st:10.3f} {st / r:10.2f} "
                     f"{enc.grad_chunk_clips(B, T, n_tail):11d}")
            emit(f"# {dtype} {B}x{T}: per unfrozen block {(per_tail[(B, T, 12)] - per_tail[(B, T, 2)]) / 10:.3f} ms")
        for p in params.values():
            p.requires_grad_(False)
        refresh = statistics.median(event_ms(lambda: enc.load_state_dict(params), 3) for _ in range(5))
        ms, ff, bf = attention_alone(dtype, dev)
        emit(f"# {dtype}: load_state_dict refresh of every device operand from device f32 masters {refresh:.3f} ms per step")
        emit(f"# {dtype}: attention backward alone, 16 frames x 197 tokens x 12 heads: {ms:.4f} ms; FLOP floor {ff:.4f} ms, "
             f"byte floor {bf:.4f} ms")
        del enc
        torch.cuda.empty_cache()
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
