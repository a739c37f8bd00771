"""What the four retrieval scripts share: repository paths, the embedder from a checkpoint or seeded
weights, and one clip's embedding from its frame directory."""
from __future__ import annotations

import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
for _p in (ROOT / "video-caption-algorithm_amd", ROOT):
    if str(_p) not in sys.path:
        sys.path.insert(0, str(_p))


def add_model_args(ap) -> None:
    ap.add_argument("--ckpt", "--checkpoint", dest="ckpt", default="",
                    help="caption-model or alignment-model (vit.* / vid_proj.*) checkpoint")
    ap.add_argument("--weights_seed", type=int, default=None, help="seeded random-init weights when no --ckpt")
    ap.add_argument("--vit_name", default="vit_base_patch16_224")
    ap.add_argument("--precision", default="bf16", choices=["bf16", "fp16", "fp32", "fp8"])
    ap.add_argument("--num_frames", type=int, default=8)
    ap.add_argument("--image_size", type=int, default=224)
    ap.add_argument("--device", default="cuda")


def load_embedder(args):
    import torch
    from vcap import configs
    from vcap.retrieval import HipVideoEmbedder, remap_alignment_state_dict
    from vcap.weights import synthetic_vit
    arch = configs.vit_arch(args.vit_name)
    sd = synthetic_vit(1 if args.weights_seed is None else int(args.weights_seed), arch)
    if args.ckpt:
        state = remap_alignment_state_dict(torch.load(args.ckpt, map_location="cpu", weights_only=True))
        for k in sd:
            if k in state and tuple(state[k].shape) != tuple(sd[k].shape):
                raise SystemExit(f"[ERROR] size mismatch for {k}: checkpoint {tuple(state[k].shape)} vs model "
                                 f"{tuple(sd[k].shape)}")
        sd = {k: state.get(k, v) for k, v in sd.items()}
    return HipVideoEmbedder.from_state_dict(sd, arch, args.precision, args.device)


def embed_frames_dir(embedder, frames_dir, args):
    """frames_dir/frame_*.jpg -> [1, video_dim] f32 unit row on the device (JPEGs decode on the GPU)."""
    from core.preprocessing.frame_loader import load_video_tensor
    video = load_video_tensor(str(frames_dir), args.num_frames, args.image_size, args.device)
    return embedder.encode_video(video)


def add_index_type_args(ap) -> None:
    """The reference's scripts/build_index_with_captions.py index flags."""
    ap.add_argument("--index_type", choices=["Flat", "IVF_FLAT"], default="Flat")
    ap.add_argument("--nlist", type=int, default=50, help="clusters of an IVF_FLAT index")


def build_index_from(feats, args, normalize: bool):
    """A Flat or IVF_FLAT index (args.index_type / nlist / storage / device) holding the f32 rows `feats`;
    an IVF index is trained on the same rows first, as the reference does."""
    from vcap.retrieval import FlatIPIndex, IVFFlatIPIndex
    if args.index_type == "IVF_FLAT":
        index = IVFFlatIPIndex(feats.shape[1], args.nlist, args.storage, args.device, normalize=normalize)
        index.train(feats)
    else:
        index = FlatIPIndex(feats.shape[1], args.storage, args.device, normalize=normalize)
    index.add(feats)
    return index


def load_index_for_query(directory, args):
    """load_index plus --nprobe (an IVF index only; 0 keeps the saved value)."""
    from vcap.retrieval import load_index
    index = load_index(directory, args.device)
    if getattr(args, "nprobe", 0) and hasattr(index, "nprobe"):
        index.nprobe = int(args.nprobe)
    return index


def read_annotations(path):
    """The reference's annotations.json: a list of {"video_id", "frames_dir", "captions": [...]}."""
    anns = json.loads(Path(path).read_text("utf-8"))
    if not isinstance(anns, list):
        raise SystemExit(f"[ERROR] {path}: expected a list of annotation records")
    return anns
