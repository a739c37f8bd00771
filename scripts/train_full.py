"""Train the text/video alignment model on the device path - the reference's src/cli/train_full.py --model vit
with its name and flag names.  AdamW runs over every parameter of ViTTextAlignModel: the ViT (forward and
backward on the HIP kernels, vcap_vit_encode_backward), vid_proj (the encoder's own encoder.proj on the device)
and the text tower (vcap_text_encode_backward), on CosineEmbeddingLoss(encode_video, encode_text, +1).
F.normalize, the loss and AdamW stay in torch (vcap/train_align.py).

  --freeze_vit            the frozen recipe: delegates to scripts.train_align (cached clip features)
  --unfreeze_vit_last N   this project's addition: train only the last N ViT blocks (with the final norm and
                          vid_proj); 0, the default, trains every block and the embedding - the reference's
                          behaviour

Annotations, tokenisation, the run directory and the checkpoint ({"model_state": vit.* + vid_proj.* + txt_*, ...},
which scripts/query_text.py and scripts/query_video.py load) are scripts/train_align.py's.  Every step decodes
and encodes its own clips' frames: nothing is cached, since the ViT changes, and no clip is held between steps.

Refused up front: --model simple; --precision fp16 and fp8 with an unfrozen ViT (ViT training serves fp32 and
bf16 operands).  The device towers apply no dropout.

  python -m scripts.train_full --model vit --ann_train train/annotations.json --ann_val val/annotations.json \\
      --weights_seed 1 --epochs 1
"""
from __future__ import annotations

import random
import sys
from pathlib import Path

from scripts import train_align as TA
from scripts._common import read_annotations


def build_argparser():
    p = TA.build_argparser()
    p.prog = "Train the alignment model (ViT, vid_proj and the text tower on the HIP path)"
    p.add_argument("--unfreeze_vit_last", type=int, default=0,
                   help="train only the last N ViT blocks; 0 (default): every block, as the reference does")
    return p


def check_args(args) -> None:
    """The refusals, before anything is imported or loaded."""
    if args.model != "vit":
        raise SystemExit("[ERROR] --model simple is not supported: only ViTTextAlignModel (--model vit) is on the "
                         "device path")
    if args.freeze_vit:
        return   # scripts.train_align checks the rest
    if args.precision in ("fp16", "fp8"):
        raise SystemExit(f"[ERROR] --precision {args.precision} with an unfrozen ViT is not supported: ViT training "
                         "serves fp32 and bf16 operands (add --freeze_vit, or choose --precision bf16 / fp32)")
    if args.unfreeze_vit_last < 0:
        raise SystemExit("[ERROR] --unfreeze_vit_last must be >= 0")
    if not 1 <= args.max_len <= 64:
        raise SystemExit("[ERROR] --max_len must be in 1..64: the device text tower takes at most 64 ids")


def frozen_argv(argv):
    """argv for scripts.train_align: this script's own flag removed."""
    out, skip = [], False
    for a in argv:
        if skip:
            skip = False
        elif a == "--unfreeze_vit_last":
            skip = True
        elif not a.startswith("--unfreeze_vit_last="):
            out.append(a)
    return out


def main(argv=None) -> int:
    argv = list(sys.argv[1:] if argv is None else argv)
    args = build_argparser().parse_args(argv)
    check_args(args)
    if args.freeze_vit:
        return TA.main(frozen_argv(argv))
    import numpy as np
    import torch
    from core.preprocessing.frame_loader import load_video_tensor
    from vcap import configs
    from vcap.model import HipViTEncoder
    from vcap.retrieval import HipTextEmbedder, remap_alignment_state_dict
    from vcap.tokenizer import load_tokenizer
    from vcap.train_align import VID_B, VID_W, AlignTrainer, align_param_name, synthetic_align_state_dict
    from vcap.weights import synthetic_vit

    random.seed(args.seed)
    torch.manual_seed(args.seed)
    rng = random.Random(args.seed)
    run_dir, ckpt_dir = Path(args.run_dir), Path(args.ckpt_dir)
    run_dir.mkdir(parents=True, exist_ok=True)
    ckpt_dir.mkdir(parents=True, exist_ok=True)

    tok = load_tokenizer(args.tokenizer_dir)
    pad_id = int(tok.pad_token_id if args.pad_id is None else args.pad_id)
    arch = configs.vit_arch(args.vit_name)
    if args.unfreeze_vit_last > arch.depth:
        raise SystemExit(f"[ERROR] --unfreeze_vit_last {args.unfreeze_vit_last}: {args.vit_name} has {arch.depth} blocks")
    seed = 1 if args.weights_seed is None else int(args.weights_seed)
    # the whole alignment model under its own names: vit.*, vid_proj.*, txt_*
    sd = synthetic_align_state_dict(seed, arch.dim, args.vocab_size, pad_id, args.txt_dim, args.txt_layers,
                                    args.txt_nhead, args.proj_dim)
    sd.update({align_param_name(k): v for k, v in synthetic_vit(seed, arch, video_dim=args.proj_dim).items()
               if k.startswith("encoder.backbone.")})
    if args.ckpt:
        state = torch.load(args.ckpt, map_location="cpu", weights_only=True)
        state = state.get("model_state", state)
        for k in sd:
            if k in state:
                sd[k] = np.ascontiguousarray(torch.as_tensor(state[k]).float().numpy())
    if sd[VID_W].shape != (args.proj_dim, arch.dim) or sd[VID_B].shape != (args.proj_dim,):
        raise SystemExit(f"[ERROR] vid_proj {sd[VID_W].shape} does not map the ViT's {arch.dim} to --proj_dim {args.proj_dim}")
    encoder = HipViTEncoder(remap_alignment_state_dict(sd), arch, args.precision, args.device, args.proj_dim)
    text = HipTextEmbedder.from_state_dict(sd, pad_id, args.txt_nhead, args.text_dtype, args.device)

    train_anns, val_anns = read_annotations(args.ann_train), read_annotations(args.ann_val)
    train_rows, val_rows = TA.caption_rows(train_anns, tok, args.max_len), TA.caption_rows(val_anns, tok, args.max_len)
    if not train_rows:
        raise SystemExit(f"[ERROR] {args.ann_train}: no captions")
    print(f"[data] {len(train_anns)} train clips / {len(train_rows)} captions, {len(val_anns)} val clips / "
          f"{len(val_rows)} captions")

    def clip(a):
        """one clip's frames [1, T, 3, H, W] on the device, decoded when its batch is built: nothing is held"""
        return load_video_tensor(str(a["frames_dir"]), args.num_frame, args.image_size, args.device)

    trainer = AlignTrainer(text, sd, lr=args.lr, video_encoder=encoder, unfreeze_vit_last=args.unfreeze_vit_last)
    n = sum(p.numel() for p in trainer.params) + sum(p.numel() for p in trainer.vit_params)
    print(f"[trainable] last {trainer.vit_n_tail} of {arch.depth} ViT blocks + vid_proj + text tower | "
          f"params={n:,} | lr={args.lr}")

    def batches(rows, anns, shuffle: bool):
        order = list(range(len(rows)))
        if shuffle:
            rng.shuffle(order)
        for b0 in range(0, len(order), args.batch_size):
            pick = [rows[j] for j in order[b0:b0 + args.batch_size]]
            width = max(len(ids) for _, ids in pick)
            caps = torch.full((len(pick), width), pad_id, dtype=torch.long)
            for r, (_, ids) in enumerate(pick):
                caps[r, :len(ids)] = torch.tensor(ids, dtype=torch.long)
            yield torch.cat([clip(anns[i]) for i, _ in pick], dim=0), caps

    def validate() -> float:
        total, k = 0.0, 0
        for video, caps in batches(val_rows, val_anns, False):
            total += trainer.evaluate(video, caps)
            k += 1
            if k >= 50:
                break
        return total / max(k, 1)

    def save(step: int, epoch: int, best: float) -> None:
        path = ckpt_dir / args.ckpt_name
        torch.save({"model_state": trainer.state_dict(), "step": step, "epoch": epoch, "best_val": best,
                    "args": vars(args)}, path)
        print(f"[ckpt] saved best -> {path} (val={best:.4f})")

    best, step, done = float("inf"), 0, False
    for epoch in range(args.epochs):
        for video, caps in batches(train_rows, train_anns, True):
            loss = trainer.step(video, caps)
            step += 1
            if step == 1 or step % 10 == 0:
                print(f"[train] step {step:05d} | loss {loss:.4f}")
            with open(run_dir / "events.csv", "a", encoding="utf-8") as f:
                f.write(f"{step},{loss:.6f}\n")
            if args.val_every > 0 and step % args.val_every == 0 and val_rows:
                v = validate()
                print(f"[val]   step {step:05d} | val_loss {v:.4f}")
                with open(run_dir / "val.csv", "a", encoding="utf-8") as f:
                    f.write(f"{step},{v:.6f}\n")
                if v < best:
                    best = v
                    save(step, epoch, best)
            if args.max_steps > 0 and step >= args.max_steps:
                done = True
                break
        v = validate() if val_rows else float(loss)
        print(f"[val][epoch end] epoch {epoch} | val_loss {v:.4f}")
        with open(run_dir / "val.csv", "a", encoding="utf-8") as f:
            f.write(f"{step},{v:.6f}\n")
        if v < best:
            best = v
            save(step, epoch, best)
        if done:
            break
    print("[OK] alignment training finished.")
    return 0


if __name__ == "__main__":
    sys.exit(main())
