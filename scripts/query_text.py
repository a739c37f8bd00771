"""Query a built index with captions: embed them with the alignment model's text tower
(ViTTextAlignModel.encode_text) on the HIP path, search, print the neighbours as scripts.query_video does.

    python -m scripts.query_text --index_dir index_dir --ckpt align.pt --pad_id 0 --topk 5 --ids "464 3290 318"
    python -m scripts.query_text --index_dir index_dir --ckpt align.pt --pad_id 0 --text "a dog runs" \
        --tokenizer_dir dir_with_vocab_json_and_merges_txt

--ids / --text may be repeated, one caption each; captions are right-padded to the longest with pad_id.
Text needs a LOCAL vocab.json + merges.txt (vcap/tokenizer.py: nothing is fetched); without one, give ids
(an "ids:" prefix is accepted, as in the caption prompts).
"""
from __future__ import annotations

import argparse
import json
import time
from pathlib import Path

from scripts import _common as common  # (also puts the package on sys.path)


def parse(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--index_dir", required=True, help="index directory written by scripts.build_index")
    ap.add_argument("--meta", default="", help="meta.json (default: <index_dir>/meta.json; optional)")
    ap.add_argument("--ckpt", "--checkpoint", dest="ckpt", required=True,
                    help="alignment-model checkpoint holding the txt_* weights")
    ap.add_argument("--pad_id", type=int, required=True)
    ap.add_argument("--nhead", type=int, default=8)
    ap.add_argument("--dtype", default="f32", choices=["f32", "bf16"])
    ap.add_argument("--topk", type=int, default=5)
    ap.add_argument("--nprobe", type=int, default=0, help="lists an IVF_FLAT index scans (0: the saved value)")
    ap.add_argument("--ids", action="append", default=[], help='one caption as token ids, e.g. "464 3290 318"')
    ap.add_argument("--text", action="append", default=[], help="one caption as text (needs --tokenizer_dir)")
    ap.add_argument("--tokenizer_dir", default="")
    ap.add_argument("--device", default="cuda")
    ap.add_argument("--out_json", default="", help="also write the hits, per query a list of [id, score], here")
    return ap.parse_args(argv)


def caption_ids(args):
    """The captions of --ids / --text as id lists, --ids first."""
    caps = []
    for s in args.ids:
        s = s.strip()
        try:
            caps.append([int(t) for t in (s[4:] if s.startswith("ids:") else s).split()])
        except ValueError:
            raise SystemExit(f"[ERROR] --ids takes space-separated integers, got {s!r}")
    if args.text:
        from vcap.tokenizer import BPETokenizer, load_tokenizer
        tok = load_tokenizer(args.tokenizer_dir)
        if not isinstance(tok, BPETokenizer):
            raise SystemExit("[ERROR] --text needs --tokenizer_dir <dir with vocab.json, merges.txt>; "
                             "without a local vocab pass --ids")
        caps += [tok.encode_prompt(t) for t in args.text]
    if not caps or any(not c for c in caps):
        raise SystemExit("[ERROR] give at least one non-empty caption with --ids or --text")
    return caps


def pad_right(caps, pad_id):
    longest = max(len(c) for c in caps)
    return [c + [pad_id] * (longest - len(c)) for c in caps]


def main(argv=None):
    args = parse(argv)
    caps = caption_ids(args)
    import torch
    from vcap.retrieval import HipTextEmbedder, meta_caption
    idx_dir = Path(args.index_dir)
    if not (idx_dir / "index.json").exists():
        raise SystemExit(f"[ERROR] Missing index under {idx_dir}")
    meta_path = Path(args.meta) if args.meta else idx_dir / "meta.json"
    meta = json.loads(meta_path.read_text("utf-8")) if meta_path.exists() else None
    print(f"[INFO] Loading index from {idx_dir}")
    index = common.load_index_for_query(idx_dir, args)
    state = torch.load(args.ckpt, map_location="cpu", weights_only=True)
    try:
        emb = HipTextEmbedder.from_state_dict(state, args.pad_id, args.nhead, args.dtype, args.device)
        if emb.proj_dim != index.dim:
            raise ValueError(f"the text tower projects to {emb.proj_dim}, the index holds {index.dim}")
        print("[INFO] Encoding query text ...")
        t0 = time.time()
        q = emb.encode_text(pad_right(caps, args.pad_id))
    except ValueError as e:
        raise SystemExit(f"[ERROR] {e}")
    D, I = index.search(q, args.topk)
    D, I = D.cpu().numpy(), I.cpu().numpy()
    print(f"[INFO] Search done in {time.time() - t0:.2f}s\n")
    results = []
    for qi, cap in enumerate(caps):
        print(f"[TOP-K RESULTS] query {qi}: ids {' '.join(map(str, cap))}")
        hits = []
        for rank, (idx, score) in enumerate(zip(I[qi], D[qi]), start=1):
            if idx < 0:     # fewer than topk vectors in the index
                break
            item = meta[idx] if meta is not None else {"video_id": str(int(idx))}
            print(f"[{rank}] score={score:.4f} | id={item.get('video_id', '?')} | caption={meta_caption(item)}")
            hits.append((int(idx), float(score)))
        results.append(hits)
    if args.out_json:
        Path(args.out_json).write_text(json.dumps(results))
    print("\nDone.")
    return results


if __name__ == "__main__":
    main()
