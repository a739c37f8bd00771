"""Video retrieval on the HIP path: clip embeddings, a device flat inner-product index, retrieval metrics.

The inference half of the reference's second product (scripts/extract_features.py, build_index.py,
query_video.py, eval_retrieval.py over src/models/vit_text_align.py::encode_video):

  * `HipVideoEmbedder.encode_video` = ViTTextAlignModel.encode_video (vit_text_align.py:54-65) =
    ViTFrameEncoder(pool="cls", l2norm=True) (video_encoder.py:318-319): vcap_vit_encode's enc_out
    followed by vcap_l2_normalize (mode 0, F.normalize's eps).
  * `FlatIPIndex` = faiss.IndexFlatIP (+ faiss.normalize_L2 on add, build_index.py:40-42): one device
    tensor of f32 or bf16 rows searched exactly by vcap_ip_search.  The FAISS file format is not
    reproduced: `save` writes vectors.npy + index.json (+ the reference's meta.json).
  * `retrieval_metrics` = the Recall@k / MRR loop of eval_retrieval.py:32-54.
  * `HipTextEmbedder.encode_text` = ViTTextAlignModel.encode_text (vit_text_align.py:67-79): one
    vcap_text_encode call per chunk of captions; `HipAlignModel` = the model's forward over both towers.
    A caption query searches the same index a clip query does (scripts/query_text.py).

There is no torch fallback: a CPU tensor is moved to the index's device, and the search is the kernel.
"""
from __future__ import annotations

import ctypes as C
import json
from pathlib import Path
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import _native as N
from .configs import VIDEO_DIM

F_NORMALIZE_EPS = 1e-12      # torch.nn.functional.normalize (mode 0)
SCRIPT_L2NORM_EPS = 1e-8     # l2norm of query_video.py:20-21 / eval_retrieval.py:10 (mode 1)
MAX_K, MAX_NQ, MAX_QUERY_FLOATS = 128, 64, 16384
_STORAGE = {"f32": (N.DT_F32, torch.float32), "bf16": (N.DT_BF16, torch.bfloat16)}


def _stream(device) -> int:
    return torch.cuda.current_stream(device).cuda_stream


def slab_rows() -> int:
    """Database rows a scan workgroup takes per step (the kernel's own constant)."""
    return int(N.lib().vcap_ip_search_slab_rows())


def scan_workgroups(n: int, max_blocks: int = 0) -> int:
    """Scan grid for n rows on the current device; workgroup w takes slabs w, w + grid, ..."""
    return int(N.lib().vcap_ip_search_workgroups(int(n), int(max_blocks)))


def _f32_rows(x, device, dim: Optional[int] = None) -> torch.Tensor:
    t = torch.from_numpy(np.ascontiguousarray(x)) if isinstance(x, np.ndarray) else torch.as_tensor(x)
    if t.dim() == 1:
        t = t[None]
    if t.dim() != 2 or (dim is not None and t.shape[1] != dim):
        raise ValueError(f"expect [rows, {dim if dim is not None else 'dim'}], got {tuple(t.shape)}")
    return t.to(device=device, dtype=torch.float32).contiguous()


def l2_normalize(x: torch.Tensor, eps: float = F_NORMALIZE_EPS, mode: int = 0,
                 out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Rows of a device f32 [rows, dim] tensor (unit inner stride) through vcap_l2_normalize; `out` may be x."""
    if x.dim() != 2 or x.dtype != torch.float32 or not x.is_cuda or x.stride(1) != 1:
        raise ValueError("l2_normalize: expect a device f32 [rows, dim] tensor with unit inner stride")
    y = torch.empty(x.shape, dtype=torch.float32, device=x.device) if out is None else out
    if y.shape != x.shape or y.dtype != torch.float32 or y.device != x.device or y.stride(1) != 1:
        raise ValueError("l2_normalize: out must match x")
    rows, dim = x.shape
    if rows:
        N.check(N.lib().vcap_l2_normalize(x.data_ptr(), x.stride(0), y.data_ptr(), y.stride(0), rows, dim, eps, mode,
                                          _stream(x.device)), "vcap_l2_normalize")
    return y


def ip_search(db: torch.Tensor, n: int, queries: torch.Tensor, k: int, workspace: Optional[torch.Tensor] = None,
              max_blocks: int = 0, stream: Optional[int] = None):
    """One vcap_ip_search call: the first n rows of the contiguous device tensor db [rows, dim] (f32 or
    bf16) against queries [nq, dim] f32 -> (scores [nq, k] f32, ids [nq, k] int64)."""
    dt = {torch.float32: N.DT_F32, torch.bfloat16: N.DT_BF16}.get(db.dtype)
    if dt is None or db.dim() != 2 or not db.is_contiguous() or not db.is_cuda:
        raise ValueError("ip_search: db must be a contiguous device f32 / bf16 [rows, dim] tensor")
    if queries.dtype != torch.float32 or queries.dim() != 2 or not queries.is_contiguous() or queries.device != db.device:
        raise ValueError("ip_search: queries must be contiguous f32 [nq, dim] on the database's device")
    if not 0 <= n <= db.shape[0] or queries.shape[1] != db.shape[1]:
        raise ValueError("ip_search: n / dim do not match the database")
    nq, dim = queries.shape
    lib = N.lib()
    need = int(lib.vcap_ip_search_workspace_bytes(n, dim, nq, k))
    if workspace is None or workspace.numel() < need:
        workspace = torch.empty(max(need, 8), dtype=torch.uint8, device=db.device)
    scores = torch.empty(nq, k, dtype=torch.float32, device=db.device)
    ids = torch.empty(nq, k, dtype=torch.int64, device=db.device)
    N.check(lib.vcap_ip_search(dt, db.data_ptr(), n, dim, queries.data_ptr(), nq, k, scores.data_ptr(), ids.data_ptr(),
                               workspace.data_ptr(), workspace.numel(), max_blocks,
                               _stream(db.device) if stream is None else stream), "vcap_ip_search")
    return scores, ids


class FlatIPIndex:
    """faiss.IndexFlatIP on the device: exact inner-product top-k over f32 or bf16 rows.

    Results are ordered by score descending, then id ascending; where fewer than k rows exist the tail is
    id -1 with score -inf.  A row whose score is NaN is never returned."""

    def __init__(self, dim: int, storage: str = "f32", device="cuda", normalize: bool = False):
        if storage not in _STORAGE:
            raise ValueError(f"storage must be one of {sorted(_STORAGE)}, got {storage!r}")
        if dim % 64 or not 64 <= dim <= 1024:
            raise ValueError("dim must be a multiple of 64 in 64..1024")
        self.dim, self.storage, self.device, self.normalize = int(dim), storage, torch.device(device), bool(normalize)
        self.ntotal = 0
        self.metadata: Optional[List[Dict[str, str]]] = None
        self._dt, self._tdt = _STORAGE[storage]
        self._rows: Optional[torch.Tensor] = None     # [capacity, dim], grown by doubling
        self._ws: Optional[torch.Tensor] = None

    @property
    def vectors(self) -> torch.Tensor:
        """The stored rows [ntotal, dim] in the storage dtype (a view)."""
        if self._rows is None:
            return torch.empty(0, self.dim, dtype=self._tdt, device=self.device)
        return self._rows[:self.ntotal]

    def reset(self) -> None:
        self.ntotal, self._rows, self.metadata = 0, None, None

    def _reserve(self, total: int) -> None:
        have = 0 if self._rows is None else self._rows.shape[0]
        if total <= have:
            return
        grown = torch.empty(max(total, 2 * have, 64), self.dim, dtype=self._tdt, device=self.device)
        if self.ntotal:
            grown[:self.ntotal].copy_(self._rows[:self.ntotal])
        self._rows = grown

    def add(self, x) -> None:
        x = _f32_rows(x, self.device, self.dim)
        rows = x.shape[0]
        if not rows:
            return
        if self.normalize:
            x = l2_normalize(x, F_NORMALIZE_EPS, 0)
        self._reserve(self.ntotal + rows)
        dst = self._rows[self.ntotal:self.ntotal + rows]
        N.check(N.lib().vcap_ip_index_convert(x.data_ptr(), self.dim, rows, self.dim, self._dt, dst.data_ptr(),
                                              _stream(self.device)), "vcap_ip_index_convert")
        self.ntotal += rows

    def search(self, q, k: int, max_blocks: int = 0):
        """q [nq, dim] (torch or numpy, any nq) -> (D [nq, k] f32, I [nq, k] int64) on the index's device."""
        if not 1 <= k <= MAX_K:
            raise ValueError(f"k must be in 1..{MAX_K}")
        q = _f32_rows(q, self.device, self.dim)
        nq = q.shape[0]
        D = torch.empty(nq, k, dtype=torch.float32, device=self.device)
        I = torch.empty(nq, k, dtype=torch.int64, device=self.device)
        db = self._rows if self._rows is not None else torch.empty(1, self.dim, dtype=self._tdt, device=self.device)
        chunk = min(MAX_NQ, MAX_QUERY_FLOATS // self.dim)
        for s in range(0, nq, chunk):
            part = q[s:s + chunk]
            need = int(N.lib().vcap_ip_search_workspace_bytes(self.ntotal, self.dim, part.shape[0], k))
            if self._ws is None or self._ws.numel() < need:
                self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
            d, i = ip_search(db, self.ntotal, part, k, self._ws, max_blocks)
            D[s:s + chunk], I[s:s + chunk] = d, i
        return D, I

    # ---- persistence: vectors.npy (f32 as given, bf16 bits as uint16) + index.json (+ meta.json)
    def save(self, directory) -> None:
        d = Path(directory)
        d.mkdir(parents=True, exist_ok=True)
        v = self.vectors
        arr = v.cpu().numpy() if self.storage == "f32" else v.view(torch.int16).cpu().numpy().view(np.uint16)
        np.save(d / "vectors.npy", arr)
        (d / "index.json").write_text(json.dumps({"dim": self.dim, "storage": self.storage, "ntotal": self.ntotal,
                                                  "normalize": self.normalize}))
        if self.metadata is not None:
            write_meta(d / "meta.json", self.metadata)

    @classmethod
    def load(cls, directory, device="cuda") -> "FlatIPIndex":
        d = Path(directory)
        info = json.loads((d / "index.json").read_text())
        idx = cls(info["dim"], info["storage"], device, info.get("normalize", False))
        arr = np.load(d / "vectors.npy")
        if arr.shape != (info["ntotal"], info["dim"]):
            raise ValueError(f"vectors.npy holds {arr.shape}, index.json says {(info['ntotal'], info['dim'])}")
        if arr.shape[0]:
            idx._reserve(arr.shape[0])
            t = torch.from_numpy(arr) if info["storage"] == "f32" else \
                torch.from_numpy(arr.view(np.int16)).view(torch.bfloat16)
            idx._rows[:arr.shape[0]].copy_(t.to(idx.device))     # stored bits, not re-normalised
            idx.ntotal = arr.shape[0]
        if (d / "meta.json").exists():
            idx.metadata = json.loads((d / "meta.json").read_text("utf-8"))
        return idx


def check_meta(meta) -> List[Dict[str, str]]:
    """The reference's meta.json: a list of {"video_id": str, "caption": str} (build_index.py:31-34)."""
    if not isinstance(meta, list):
        raise ValueError("metadata must be a list")
    for m in meta:
        if not isinstance(m, dict) or set(m) != {"video_id", "caption"} or \
                not all(isinstance(m[key], str) for key in ("video_id", "caption")):
            raise ValueError('metadata entries must be {"video_id": str, "caption": str}')
    return meta


def write_meta(path, meta) -> None:
    Path(path).write_text(json.dumps(check_meta(meta), ensure_ascii=False, indent=2), encoding="utf-8")


def first_caption(rec) -> str:
    """build_index.py:30: the first caption of an annotation record, "" when it has none."""
    caps = rec.get("captions")
    return caps[0] if isinstance(caps, list) and caps else ""


def meta_caption(item) -> str:
    """query_video.py:133-139: a meta entry's printable caption ("captions" list or "caption" string)."""
    if isinstance(item.get("captions"), list) and item["captions"]:
        return item["captions"][0]
    if isinstance(item.get("caption"), str):
        return item["caption"]
    return "(no caption)"


def retrieval_metrics(ranked_ids, gold_ids: Sequence[int], ks: Sequence[int] = (1, 5)) -> Dict[str, float]:
    """eval_retrieval.py:32-54: ranked_ids [n, >= max(ks)] (row i = the ids returned for query i, best
    first), gold_ids [n].  A gold id absent from its row contributes 0 to every figure."""
    rows = ranked_ids.tolist() if hasattr(ranked_ids, "tolist") else [list(r) for r in ranked_ids]
    gold = gold_ids.tolist() if hasattr(gold_ids, "tolist") else list(gold_ids)
    if len(rows) != len(gold):
        raise ValueError("ranked_ids and gold_ids differ in length")
    hit = {k: 0 for k in ks}
    mrr = 0.0
    for row, g in zip(rows, gold):
        if g in row:
            rank = row.index(g) + 1
            mrr += 1.0 / rank
            for k in ks:
                hit[k] += rank <= k
    n = len(rows)
    out = {f"recall@{k}": (hit[k] / n if n else 0.0) for k in ks}
    out.update(mrr=(mrr / n if n else 0.0), n=n)
    return out


def remap_alignment_state_dict(state) -> Dict[str, np.ndarray]:
    """A caption-model state dict (encoder.backbone.* / encoder.proj.*) or an alignment-model one
    (ViTTextAlignModel: vit.* -> encoder.backbone.*, vid_proj.* -> encoder.proj.*; the text tower txt_*
    is dropped), either bare or under {"model_state": ...} as query_video.py:106-107 loads it."""
    if isinstance(state, dict) and "model_state" in state:
        state = state["model_state"]
    out: Dict[str, np.ndarray] = {}
    for k, v in state.items():
        if k.startswith("txt_"):
            continue
        if k.startswith("vit."):
            k = "encoder.backbone." + k[len("vit."):]
        elif k.startswith("vid_proj."):
            k = "encoder.proj." + k[len("vid_proj."):]
        if hasattr(v, "detach"):
            v = v.detach().float().cpu().numpy()
        out[k] = np.ascontiguousarray(v, dtype=np.float32)
    return out


class HipVideoEmbedder:
    """ViTTextAlignModel.encode_video on the HIP path: HipViTEncoder.encode -> L2 normalisation."""

    def __init__(self, encoder):
        self.encoder = encoder
        self.device = encoder.device
        self.video_dim = encoder.video_dim

    @classmethod
    def from_state_dict(cls, sd, arch, precision: str = "bf16", device="cuda", video_dim: int = VIDEO_DIM):
        from .model import HipViTEncoder
        return cls(HipViTEncoder(remap_alignment_state_dict(sd), arch, precision, device, video_dim))

    def encode_video(self, video: torch.Tensor) -> torch.Tensor:
        """video [B, T, 3, H, W] f32 on the device -> [B, video_dim] f32, unit rows."""
        enc, _ = self.encoder.encode(video)
        return l2_normalize(enc, F_NORMALIZE_EPS, 0, out=enc)


# ---- text tower: ViTTextAlignModel.encode_text (vit_text_align.py:67-79) through vcap_text_encode
TEXT_MAX_LEN = 64
_TEXT_DTYPE = {"f32": (N.DT_F32, torch.float32), "bf16": (N.DT_BF16, torch.bfloat16)}


def text_tower_state_dict(state) -> Dict[str, np.ndarray]:
    """The txt_* entries (txt_emb, txt_enc.layers.*, txt_proj) of an alignment-model state dict as f32
    numpy, names unchanged; the dict bare or under {"model_state": ...}."""
    if isinstance(state, dict) and "model_state" in state:
        state = state["model_state"]
    out: Dict[str, np.ndarray] = {}
    for k, v in state.items():
        if not k.startswith("txt_"):
            continue
        if hasattr(v, "detach"):
            v = v.detach().float().cpu().numpy()
        out[k] = np.ascontiguousarray(v, dtype=np.float32)
    return out


class HipTextEmbedder:
    """ViTTextAlignModel.encode_text on the HIP path: one vcap_text_encode call per chunk of captions.

    The reference's text side is never autocast, so f32 is the default; "bf16" rounds the GEMV operands,
    the stored q/k/v, the attention output and the ReLU output to bf16 and keeps the rest f32."""

    def __init__(self, sd: Dict[str, np.ndarray], pad_id: int, nhead: int = 8, dtype: str = "f32", device="cuda"):
        if dtype not in _TEXT_DTYPE:
            raise ValueError(f"dtype must be one of {sorted(_TEXT_DTYPE)}, got {dtype!r}")
        sd = text_tower_state_dict(sd)
        for k in ("txt_emb.weight", "txt_proj.weight", "txt_proj.bias"):
            if k not in sd:
                raise ValueError(f"state dict has no {k}: not an alignment-model text tower")
        self.vocab, self.dim = (int(v) for v in sd["txt_emb.weight"].shape)
        self.proj_dim = int(sd["txt_proj.weight"].shape[0])
        if sd["txt_proj.weight"].shape[1] != self.dim:
            raise ValueError("txt_proj.weight does not match txt_emb.weight's width")
        if nhead <= 0 or self.dim != 64 * nhead:
            raise ValueError(f"dim / nhead must be 64 (dim {self.dim}, nhead {nhead}): the kernels' head width")
        if not 0 <= int(pad_id) < self.vocab:
            raise ValueError(f"pad_id {pad_id} outside the vocabulary of {self.vocab}")
        pre = "txt_enc.layers."
        self.n_layer = 1 + max((int(k[len(pre):].split(".")[0]) for k in sd if k.startswith(pre)), default=-1)
        self.ffn = int(sd[pre + "0.linear1.weight"].shape[0]) if self.n_layer else 4 * self.dim
        self.pad_id, self.nhead, self.dtype, self.device = int(pad_id), int(nhead), dtype, torch.device(device)
        self.dt, tdt = _TEXT_DTYPE[dtype]
        self._keep: List[torch.Tensor] = []
        dev = self.device

        def f32(k):
            t = torch.from_numpy(sd[k]).to(dev).contiguous()
            self._keep.append(t)
            return t

        def packed(k):  # [N, K] Linear weight -> operand dtype -> rows-packed (vcap_rows_pack)
            w = torch.from_numpy(sd[k]).to(dev).to(tdt).contiguous()
            rows, kk = w.shape
            nbytes = int(N.lib().vcap_rows_packed_bytes(self.dt, rows, kk))
            if nbytes == 0:
                raise ValueError(f"cannot pack {k} {tuple(w.shape)}")
            p = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            N.check(N.lib().vcap_rows_pack(self.dt, w.data_ptr(), w.stride(0), rows, kk, p.data_ptr(), _stream(dev)),
                    "vcap_rows_pack")
            self._keep.append(p)
            return p

        self.layers = (N.TextLayer * max(self.n_layer, 1))()
        for i in range(self.n_layer):
            b, ly = f"{pre}{i}.", self.layers[i]
            ly.in_w, ly.in_b = packed(b + "self_attn.in_proj_weight").data_ptr(), f32(b + "self_attn.in_proj_bias").data_ptr()
            ly.out_w, ly.out_b = packed(b + "self_attn.out_proj.weight").data_ptr(), f32(b + "self_attn.out_proj.bias").data_ptr()
            ly.ln1_g, ly.ln1_b = f32(b + "norm1.weight").data_ptr(), f32(b + "norm1.bias").data_ptr()
            ly.fc1_w, ly.fc1_b = packed(b + "linear1.weight").data_ptr(), f32(b + "linear1.bias").data_ptr()
            ly.fc2_w, ly.fc2_b = packed(b + "linear2.weight").data_ptr(), f32(b + "linear2.bias").data_ptr()
            ly.ln2_g, ly.ln2_b = f32(b + "norm2.weight").data_ptr(), f32(b + "norm2.bias").data_ptr()
        self.desc = N.TextDesc(dtype=self.dt, vocab=self.vocab, dim=self.dim, n_layer=self.n_layer, n_head=self.nhead,
                               ffn=self.ffn, proj_dim=self.proj_dim, pad_id=self.pad_id, ln_eps=1e-5,
                               emb=f32("txt_emb.weight").data_ptr(), proj_w=f32("txt_proj.weight").data_ptr(),
                               proj_b=f32("txt_proj.bias").data_ptr(), layers=self.layers)
        self.max_rows = int(N.lib().vcap_gpt2_max_rows())
        self._ws: Optional[torch.Tensor] = None
        torch.cuda.synchronize(dev)   # packing ran on the current stream; encodes may use others

    @classmethod
    def from_state_dict(cls, sd, pad_id: int, nhead: int = 8, dtype: str = "f32", device="cuda") -> "HipTextEmbedder":
        return cls(sd, pad_id, nhead, dtype, device)

    def _ids(self, ids) -> torch.Tensor:
        """[B, L] or [L] ids (list, numpy, torch) -> int32 [B, L] on the device.  Ids that arrive on the host
        are range-checked here; a device tensor is not read back (the kernel turns a bad id into NaN)."""
        on_device = isinstance(ids, torch.Tensor) and ids.is_cuda
        t = ids if isinstance(ids, torch.Tensor) else torch.as_tensor(np.asarray(ids))
        if t.dim() == 1:
            t = t[None]
        if t.dim() != 2 or t.shape[0] < 1 or t.shape[1] < 1 or t.dtype.is_floating_point or t.dtype == torch.bool:
            raise ValueError(f"ids must be integers of shape [B, L] or [L], got {tuple(t.shape)} {t.dtype}")
        if t.shape[1] > TEXT_MAX_LEN:
            raise ValueError(f"captions of {t.shape[1]} ids: the text tower takes at most {TEXT_MAX_LEN}")
        if not on_device and (int(t.min()) < 0 or int(t.max()) >= self.vocab):
            raise ValueError(f"token id outside [0, {self.vocab})")
        if on_device and t.dtype != torch.int32:
            t = t.clamp(-1, self.vocab)     # a wide id must not wrap into the vocabulary in the int32 cast
        return t.to(device=self.device, dtype=torch.int32).contiguous()

    def encode_text(self, ids, return_hidden: bool = False):
        """ids [B, L] or [L] -> [B, proj_dim] f32 unit rows on the device (and, on request, the encoder
        output [B, L, dim] before the pool).  Batches of more than max_rows / L captions go in chunks."""
        t = self._ids(ids)
        B, L = t.shape
        out = torch.empty(B, self.proj_dim, dtype=torch.float32, device=self.device)
        hidden = torch.empty(B, L, self.dim, dtype=torch.float32, device=self.device) if return_hidden else None
        lib, per = N.lib(), max(1, self.max_rows // L)
        for s in range(0, B, per):
            n = min(per, B - s)
            need = int(lib.vcap_text_workspace_bytes(C.byref(self.desc), n, L))
            if need == 0:
                raise N.VcapError(f"vcap_text_workspace_bytes refused B={n}, L={L}: "
                                  f"{(lib.vcap_last_error() or b'').decode()}")
            if self._ws is None or self._ws.numel() < need:
                self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
            N.check(lib.vcap_text_encode(C.byref(self.desc), t[s:s + n].data_ptr(), n, L, out[s:s + n].data_ptr(),
                                         N.ptr(hidden[s:s + n]) if return_hidden else None, self._ws.data_ptr(),
                                         self._ws.numel(), _stream(self.device)), "vcap_text_encode")
        return (out, hidden) if return_hidden else out


class HipAlignModel:
    """ViTTextAlignModel's forward surface over the two HIP towers (inference only)."""

    def __init__(self, video_embedder: HipVideoEmbedder, text_embedder: HipTextEmbedder):
        self.video_embedder, self.text_embedder = video_embedder, text_embedder

    def encode_video(self, video: torch.Tensor) -> torch.Tensor:
        return self.video_embedder.encode_video(video)

    def encode_text(self, ids) -> torch.Tensor:
        return self.text_embedder.encode_text(ids)

    def forward(self, video: torch.Tensor, ids) -> torch.Tensor:
        """nn.CosineEmbeddingLoss()(encode_video, encode_text, ones) (vit_text_align.py:81-86), computed
        in torch on the device from the two embeddings."""
        v, t = self.encode_video(video), self.encode_text(ids)
        target = torch.ones(v.shape[0], device=v.device)
        return torch.nn.functional.cosine_embedding_loss(v, t, target)

    __call__ = forward
