"""Text-tower cost: HipTextEmbedder.encode_text (one vcap_text_encode call) at the reference's tower shape
(E = 512, 8 heads, F = 2048, 2 layers, P = 256, GPT-2's vocabulary of 50257) for (B, L) in {(1, 16), (16, 32),
(8, 64)}, f32 and bf16 operands.

Two lines per shape, timed in one process after a warm-up with device events around `reps` back-to-back
calls, interleaved ABAB over the rounds, medians reported:
  ours   one encode_text call on a device id tensor: 2 + 7 * layers = 16 launches
  torch  torch-ROCm's own eager modules on the same device and weights - nn.Embedding -> nn.TransformerEncoder
         -> masked mean -> nn.Linear -> F.normalize, the lines of the reference's encode_text - in float32, or
         converted to bfloat16 for the bf16 row.  There is no earlier implementation of ours to compare with.
Also printed per shape: the host time to enqueue one of our calls (a host clock around `reps` calls with no
synchronise in between, then one synchronise that is not counted) over the device time per call - the launch
share.  Near 1, the call is bound by its launches, not by its kernels.

    python tools/text_encode_bench.py --out profiles/text_encoder_bench.txt
"""
import argparse
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "video-caption-algorithm_amd"))
import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

from vcap import retrieval as R  # noqa: E402

E, H, F, LAYERS, P, V, PAD = 512, 8, 2048, 2, 256, 50257, 50256
SHAPES = ((1, 16), (16, 32), (8, 64))


class Tower(nn.Module):
    def __init__(self):
        super().__init__()
        self.txt_emb = nn.Embedding(V, E, padding_idx=PAD)
        layer = nn.TransformerEncoderLayer(d_model=E, nhead=H, dim_feedforward=F, dropout=0.1, batch_first=True)
        self.txt_enc = nn.TransformerEncoder(layer, num_layers=LAYERS, enable_nested_tensor=False)
        self.txt_proj = nn.Linear(E, P)

    def forward(self, ids):
        mask = ids != PAD
        x = self.txt_enc(self.txt_emb(ids))
        x = (x * mask.unsqueeze(-1)).sum(dim=1) / mask.sum(dim=1, keepdim=True).clamp_min(1)
        return nn.functional.normalize(self.txt_proj(x).float(), dim=-1)


def event_ms(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def enqueue_ms(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    t = (time.perf_counter() - t0) / reps * 1e3
    torch.cuda.synchronize()
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--reps", type=int, default=50)
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
    emit(f"# {torch.cuda.get_device_name(0)}; tower E={E} H={H} F={F} layers={LAYERS} P={P} V={V}; medians of "
         f"{args.rounds} interleaved rounds of {args.reps} calls; one box, one run")
    emit(f"# ours: {2 + 7 * LAYERS} launches per call; torch: eager modules, same weights")
    emit(f"# {'dtype':5} {'B':>3} {'L':>3} {'ours ms':>9} {'torch ms':>9} {'ours/torch':>10} {'enqueue ms':>10} "
         f"{'launch share':>12} {'max |ours - torch|':>18}")
    for dtype in ("f32", "bf16"):
        emb = R.HipTextEmbedder.from_state_dict(sd, PAD, H, dtype, dev)
        ref = ref32 if dtype == "f32" else Tower().eval().to(dev).to(torch.bfloat16)
        if dtype == "bf16":
            ref.load_state_dict({k: v.to(torch.bfloat16) for k, v in ref32.state_dict().items()})
        for B, L in SHAPES:
            g = torch.Generator().manual_seed(B * 100 + L)
            ids = torch.randint(0, V - 1, (B, L), generator=g)
            ids[-1, L - L // 4:] = PAD
            ids = ids.to(dev)
            ids32 = ids.to(torch.int32)

            def ours():
                return emb.encode_text(ids32)

            def base():
                with torch.no_grad():
                    return ref(ids)

            diff = float((ours() - base()).abs().max())
            for fn in (ours, base):
                event_ms(fn, 5)
            t = {"ours": [], "torch": []}
            for _ in range(args.rounds):
                t["ours"].append(event_ms(ours, args.reps))
                t["torch"].append(event_ms(base, args.reps))
            o, r = statistics.median(t["ours"]), statistics.median(t["torch"])
            q = statistics.median(enqueue_ms(ours, args.reps) for _ in range(3))
            emit(f"  {dtype:5} {B:3d} {L:3d} {o:9.4f} {r:9.4f} {o / r:10.2f} {q:10.4f} {min(q / o, 1.0):12.2f} {diff:18.2e}")
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
