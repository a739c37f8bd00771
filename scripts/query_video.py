"""Query a clip against a built index (the reference's scripts/query_video.py): embed the frame
directory, normalise as the reference's l2norm does, search, print the neighbours with their captions.

    python -m scripts.query_video --frames_dir clip_dir --k 5 --index index_dir [--meta index_dir/meta.json]

Only a directory of frame_*.jpg is accepted: extracting frames from a video file needs ffmpeg or OpenCV,
neither of which is in this environment, so --video is refused with a message.
"""
from __future__ import annotations

import argparse
import json
import time
from pathlib import Path

from scripts import _common as common


def parse(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--frames_dir", default="")
    ap.add_argument("--video", default="", help="refused: no video decoder here; extract frames first")
    ap.add_argument("--k", type=int, default=5)
    ap.add_argument("--index", required=True, help="index directory written by scripts.build_index")
    ap.add_argument("--meta", default="", help="meta.json (default: <index>/meta.json)")
    ap.add_argument("--nprobe", type=int, default=0, help="lists an IVF_FLAT index scans (0: the saved value)")
    common.add_model_args(ap)
    return ap.parse_args(argv)


def main(argv=None):
    args = parse(argv)
    if args.video:
        raise SystemExit("[ERROR] --video needs a frame extractor (ffmpeg / OpenCV), none of which is in this "
                         "environment; extract frames first (e.g. `ffmpeg -i clip.mp4 -vf fps=2 "
                         "dir/frame_%06d.jpg`) and pass --frames_dir dir")
    if not args.frames_dir:
        raise SystemExit("[ERROR] give --frames_dir (a directory of frame_*.jpg)")
    from core.preprocessing.frame_loader import list_frames
    from vcap.retrieval import SCRIPT_L2NORM_EPS, l2_normalize, meta_caption
    idx_dir = Path(args.index)
    meta_path = Path(args.meta) if args.meta else idx_dir / "meta.json"
    if not (idx_dir / "index.json").exists() or not meta_path.exists():
        raise SystemExit(f"[ERROR] Missing index/meta under {idx_dir}")
    if not list_frames(args.frames_dir):
        raise SystemExit(f"[ERROR] No frames found in {args.frames_dir}")
    print(f"[INFO] Loading index from {idx_dir}")
    index = common.load_index_for_query(idx_dir, args)
    meta = json.loads(meta_path.read_text("utf-8"))
    emb = common.load_embedder(args)
    print("[INFO] Encoding query video ...")
    t0 = time.time()
    q = l2_normalize(common.embed_frames_dir(emb, args.frames_dir, args), SCRIPT_L2NORM_EPS, 1)
    D, I = index.search(q, args.k)
    D, I = D.cpu().numpy(), I.cpu().numpy()
    print(f"[INFO] Search done in {time.time() - t0:.2f}s\n")
    print("[TOP-K RESULTS]")
    results = []
    for rank, (idx, score) in enumerate(zip(I[0], D[0]), start=1):
        if idx < 0:     # fewer than k vectors in the index
            break
        item = meta[idx]
        print(f"[{rank}] score={score:.4f} | id={item.get('video_id', '?')} | caption={meta_caption(item)}")
        results.append((int(idx), float(score)))
    print("\nDone.")
    return results


if __name__ == "__main__":
    main()
