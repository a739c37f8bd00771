"""Clip embeddings for an annotations file (the reference's scripts/extract_features.py): every record's
frames_dir -> <out_dir>/<video_id>.npy holding its [video_dim] f32 L2-normalised embedding
(ViTFrameEncoder pool="cls", l2norm=True).

    python -m scripts.extract_features --annotations ann.json --out_dir features [--ckpt x.pt]
"""
from __future__ import annotations

import argparse
from pathlib import Path

import numpy as np

from scripts import _common as common


def parse(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--annotations", required=True)
    ap.add_argument("--out_dir", required=True)
    common.add_model_args(ap)
    return ap.parse_args(argv)


def main(argv=None) -> int:
    args = parse(argv)
    from core.preprocessing.frame_loader import list_frames
    anns = common.read_annotations(args.annotations)
    out = Path(args.out_dir)
    out.mkdir(parents=True, exist_ok=True)
    emb = common.load_embedder(args)
    print(f"[INFO] Extracting features for {len(anns)} videos...")
    done = 0
    for rec in anns:
        if not list_frames(rec["frames_dir"]):    # the reference skips a record without frames
            continue
        feat = common.embed_frames_dir(emb, rec["frames_dir"], args)[0]
        np.save(out / f"{rec['video_id']}.npy", feat.cpu().numpy().astype(np.float32))
        done += 1
    print(f"[OK] Saved {done} features to {out}")
    return done


if __name__ == "__main__":
    main()
