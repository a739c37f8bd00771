"""Text-tower training cost: HipTextEmbedder.encode_text_backward (one vcap_text_encode_backward call: forward
+ backward, every parameter gradient) at the reference's tower shape (E = 512, 8 heads, F = 2048, 2 layers,
P = 256, GPT-2's vocabulary of 50257) for (B, L) in {(1, 16), (16, 32), (8, 64)}, f32 and bf16 operands.

Two lines per shape, timed in one process after a warm-up with device events around `reps` back-to-back
calls, interleaved ABAB over the rounds, medians reported:
  ours   one encode_text_backward call on a device id tensor and a device grad_out; the embedding gradient
         stays row-sparse (ids, rows)
  torch  torch-ROCm's own eager autograd of the same modules in eval mode on the same device and weights:
         forward, sum(G * out).backward(), gradients zeroed by set_to_none (its embedding gradient is a dense
         [V, E] tensor: 103 MB).  float32, or the modules converted to bfloat16 for the bf16 row.  There is no
         earlier implementation of ours to compare with.
Reported separately, per dtype: the per-step in-place refresh of the device weights from f32 masters
(load_state_dict), the dense scatter of the sparse embedding rows (vcap.train_align.scatter_embedding_grad) and
the host time to enqueue one of our calls.

    python tools/text_grad_bench.py --out profiles/text_grad_bench.txt
"""
import argparse
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "video-caption-algorithm_amd"))
sys.path.insert(0, str(ROOT / "tools"))
import torch  # noqa: E402

from text_encode_bench import PAD, SHAPES, H, LAYERS, Tower, V, enqueue_ms, event_ms  # noqa: E402
from vcap import retrieval as R  # noqa: E402
from vcap.train_align import scatter_embedding_grad  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    torch.manual_seed(0)
    ref32 = Tower().eval()
    with torch.no_grad():
        ref32.txt_emb.weight[PAD].normal_()
    sd = {k: v.detach().numpy() for k, v in ref32.state_dict().items()}
    ref32 = ref32.to(dev)
    emit(f"# {torch.cuda.get_device_name(0)}; reference tower, V={V}; forward + backward, medians of {args.rounds} "
         f"interleaved rounds of {args.reps} calls; one box, one run")
    emit(f"# {'dtype':5} {'B':>3} {'L':>3} {'ours ms':>9} {'torch ms':>9} {'ours/torch':>10} {'enqueue ms':>10} "
         f"{'scatter ms':>10}")
    for dtype in ("f32", "bf16"):
        emb = R.HipTextEmbedder.from_state_dict(sd, PAD, H, dtype, dev).enable_grad()
        ref = ref32 if dtype == "f32" else Tower().eval().to(dev).to(torch.bfloat16)
        if dtype == "bf16":
            ref.load_state_dict({k: v.to(torch.bfloat16) for k, v in ref32.state_dict().items()})
        params = list(ref.parameters())
        for B, L in SHAPES:
            g = torch.Generator().manual_seed(B * 100 + L)
            ids = torch.randint(0, V - 1, (B, L), generator=g)
            ids[-1, L - L // 4:] = PAD
            G = torch.randn(B, 256, generator=g).to(dev)
            ids = ids.to(dev)
            ids32 = ids.to(torch.int32)
            last = {}

            def ours():
                last["g"] = emb.encode_text_backward(ids32, G)[1]

            def base():
                for p in params:
                    p.grad = None
                (G * ref(ids)).sum().backward()

            def scatter():
                return scatter_embedding_grad(last["g"]["txt_emb.weight"], V)

            for fn in (ours, base):
                event_ms(fn, 3)
            t = {"ours": [], "torch": []}
            for _ in range(args.rounds):
                t["ours"].append(event_ms(ours, args.reps))
                t["torch"].append(event_ms(base, args.reps))
            o, r = statistics.median(t["ours"]), statistics.median(t["torch"])
            q = statistics.median(enqueue_ms(ours, args.reps) for _ in range(3))
            sc = statistics.median(event_ms(scatter, args.reps) for _ in range(3))
            emit(f"  {dtype:5} {B:3d} {L:3d} {o:9.4f} {r:9.4f} {o / r:10.2f} {q:10.4f} {sc:10.4f}")
        masters = {k: torch.from_numpy(v).to(dev) for k, v in sd.items()}
        refresh = statistics.median(event_ms(lambda: emb.load_state_dict(masters), 10) for _ in range(5))
        emit(f"# {dtype}: load_state_dict refresh of every device weight from device f32 masters {refresh:.4f} ms per "
             f"step; launches and copies per call {6 + (50 if dtype == 'bf16' else 46) * LAYERS}")
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
