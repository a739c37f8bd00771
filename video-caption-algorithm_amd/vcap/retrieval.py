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


MAX_NPROBE = 128


def ivf_slice_rows() -> int:
    """Rows of one list a scan workgroup takes (a work item is (query, probe, slice))."""
    return int(N.lib().vcap_ivf_slice_rows())


def ivf_chunk_rows() -> int:
    """Member rows one wave sums in the centroid update."""
    return int(N.lib().vcap_ivf_chunk_rows())


def ivf_assign(x: torch.Tensor, centroids: torch.Tensor, want_scores: bool = True):
    """vcap_ivf_assign: device f32 rows [n, dim] (unit inner stride) against contiguous f32 centroids
    [nlist, dim] -> (assign int32 [n], score f32 [n] or None): the best centroid by inner product."""
    if x.dim() != 2 or x.dtype != torch.float32 or not x.is_cuda or x.stride(1) != 1:
        raise ValueError("ivf_assign: expect a device f32 [rows, dim] tensor with unit inner stride")
    if centroids.dtype != torch.float32 or centroids.dim() != 2 or not centroids.is_contiguous() or \
            centroids.device != x.device or centroids.shape[1] != x.shape[1]:
        raise ValueError("ivf_assign: centroids must be contiguous f32 [nlist, dim] on the rows' device")
    n, dim = x.shape
    assign = torch.empty(n, dtype=torch.int32, device=x.device)
    score = torch.empty(n, dtype=torch.float32, device=x.device) if want_scores else None
    N.check(N.lib().vcap_ivf_assign(x.data_ptr(), x.stride(0) if n > 1 else max(x.stride(0), dim), n,
                                    centroids.data_ptr(), centroids.shape[0], dim, assign.data_ptr(), N.ptr(score),
                                    _stream(x.device)), "vcap_ivf_assign")
    return assign, score


def ivf_group(assign: torch.Tensor, nlist: int):
    """The grouping the centroid update and the index read: assign [n] (list id, or -1) -> (order int64 [n]:
    row indices by list, ascending within a list, the unassigned rows first; offsets int64 [nlist + 1]).
    A stable sort plus bincount / cumsum on the device."""
    a = assign.to(torch.int64)
    order = torch.sort(a, stable=True).indices
    counts = torch.bincount(a.clamp_min(0), weights=(a >= 0).to(torch.float64), minlength=nlist).to(torch.int64)
    offsets = torch.empty(nlist + 1, dtype=torch.int64, device=assign.device)
    offsets[0] = (a < 0).sum()
    offsets[1:] = offsets[0] + torch.cumsum(counts, 0)
    return order.contiguous(), offsets


def ivf_centroid_update(x: torch.Tensor, order: torch.Tensor, offsets: torch.Tensor, prev: torch.Tensor,
                        workspace: Optional[torch.Tensor] = None, stream: Optional[int] = None) -> torch.Tensor:
    """vcap_ivf_centroid_update: the L2-normalised sums of the grouped member rows; an empty list keeps prev's row."""
    n, dim = x.shape
    nlist = prev.shape[0]
    if x.dtype != torch.float32 or x.stride(1) != 1 or not prev.is_contiguous() or prev.dtype != torch.float32 or \
            order.dtype != torch.int64 or offsets.dtype != torch.int64 or order.numel() != n or \
            offsets.numel() != nlist + 1 or not order.is_contiguous() or not offsets.is_contiguous():
        raise ValueError("ivf_centroid_update: f32 rows / centroids, int64 order [n] and offsets [nlist + 1]")
    lib = N.lib()
    need = int(lib.vcap_ivf_centroid_update_workspace_bytes(n, nlist, dim))
    if workspace is None or workspace.numel() < need:
        workspace = torch.empty(max(need, 16), dtype=torch.uint8, device=x.device)
    out = torch.empty_like(prev)
    N.check(lib.vcap_ivf_centroid_update(x.data_ptr(), x.stride(0) if n > 1 else max(x.stride(0), dim), n, dim,
                                         order.data_ptr(), offsets.data_ptr(), nlist, prev.data_ptr(), out.data_ptr(),
                                         workspace.data_ptr(), workspace.numel(),
                                         _stream(x.device) if stream is None else stream), "vcap_ivf_centroid_update")
    return out


class IVFFlatIPIndex:
    """faiss.IndexIVFFlat(IndexFlatIP(d), d, nlist, METRIC_INNER_PRODUCT) on the device (the reference's
    scripts/build_index_with_captions.py --index_type IVF_FLAT): a coarse quantiser of nlist centroids, the
    rows grouped into inverted lists, and a search over the nprobe lists whose centroids score best.

    Within the probed lists the search is exact and ordered as FlatIPIndex's (score descending, then id
    ascending, filler -1 / -inf); with nprobe == nlist it returns FlatIPIndex's bits.  The FAISS file format
    is not reproduced, and training is spherical k-means without FAISS's splitting of large clusters."""

    def __init__(self, dim: int, nlist: int, storage: str = "f32", device="cuda", normalize: bool = False,
                 nprobe: int = 1):
        if storage not in _STORAGE:
            raise ValueError(f"storage must be one of {sorted(_STORAGE)}, got {storage!r}")
        if dim % 64 or not 64 <= dim <= 1024:
            raise ValueError("dim must be a multiple of 64 in 64..1024")
        if not 1 <= int(nlist) <= 1 << 20:
            raise ValueError("nlist must be in 1..1048576")
        if int(nprobe) < 1:
            raise ValueError("nprobe must be at least 1")
        self.dim, self.nlist, self.storage, self.device = int(dim), int(nlist), storage, torch.device(device)
        self.normalize, self.nprobe = bool(normalize), int(nprobe)
        self.ntotal = 0
        self.metadata: Optional[List[Dict[str, str]]] = None
        self.train_objective: List[float] = []        # mean best inner product of each training round's assignment
        self._dt, self._tdt = _STORAGE[storage]
        self._centroids: Optional[torch.Tensor] = None
        self._rows = torch.empty(0, self.dim, dtype=self._tdt, device=self.device)      # grouped by list
        self._ids = torch.empty(0, dtype=torch.int64, device=self.device)               # original id of each grouped row
        self._lists = torch.empty(0, dtype=torch.int32, device=self.device)             # list of each grouped row
        self._offsets = torch.zeros(self.nlist + 1, dtype=torch.int64, device=self.device)
        self._host_offsets = np.zeros(self.nlist + 1, np.int64)
        self._ws: Optional[torch.Tensor] = None

    # ---- the coarse quantiser
    @property
    def is_trained(self) -> bool:
        return self._centroids is not None

    @property
    def centroids(self) -> torch.Tensor:
        """The coarse centroids [nlist, dim] f32 (a view)."""
        if self._centroids is None:
            raise RuntimeError("the index is not trained")
        return self._centroids

    def set_centroids(self, centroids) -> None:
        """Install coarse centroids [nlist, dim] trained elsewhere, as given (the index must be empty)."""
        if self.ntotal:
            raise RuntimeError("set_centroids on an index that holds rows")
        c = _f32_rows(centroids, self.device, self.dim)
        if c.shape[0] != self.nlist:
            raise ValueError(f"expect [{self.nlist}, {self.dim}] centroids, got {tuple(c.shape)}")
        self._centroids = c.clone()

    def training_set(self, x, seed: int = 1234, max_points_per_centroid: int = 256):
        """What train starts from: (the f32 training rows on the device - normalised if the index normalises,
        subsampled to at most max_points_per_centroid * nlist - and the initial centroids [nlist, dim])."""
        x = _f32_rows(x, self.device, self.dim)
        n = x.shape[0]
        if n < self.nlist:
            raise ValueError(f"train needs at least nlist = {self.nlist} rows, got {n}")
        if self.normalize:
            x = l2_normalize(x, F_NORMALIZE_EPS, 0)
        rng = np.random.default_rng(seed)
        cap = max(1, int(max_points_per_centroid)) * self.nlist
        if n > cap:
            x = x[torch.from_numpy(rng.permutation(n)[:cap]).to(self.device)].contiguous()
            n = cap
        first = torch.from_numpy(np.sort(rng.choice(n, self.nlist, replace=False))).to(self.device)
        return x, l2_normalize(x[first].contiguous(), F_NORMALIZE_EPS, 0)

    def train(self, x, niter: int = 10, seed: int = 1234, max_points_per_centroid: int = 256) -> None:
        """Spherical k-means on the device.  One numpy.random.default_rng(seed) draws the subsample (at most
        max_points_per_centroid * nlist rows) and then nlist distinct rows as the initial centroids
        (L2-normalised); niter rounds of assign (vcap_ivf_assign) -> group (stable sort) -> update
        (vcap_ivf_centroid_update) follow.  The same rows and seed give the same centroid bits.

        nprobe = 1, niter = 10 and 256 points per centroid are FAISS's defaults as remembered - FAISS was not
        available to compare with, and no bit parity with FAISS's centroids is claimed: FAISS minimises L2
        (on unit rows the same assignment as arg-max inner product against unit centroids) and splits a large
        cluster to refill an empty one, where this index lets an empty list keep its centroid."""
        x, cent = self.training_set(x, seed, max_points_per_centroid)
        n = x.shape[0]
        need = int(N.lib().vcap_ivf_centroid_update_workspace_bytes(n, self.nlist, self.dim))
        ws = torch.empty(max(need, 16), dtype=torch.uint8, device=self.device)
        objective = []
        for _ in range(int(niter)):
            assign, score = ivf_assign(x, cent)
            objective.append(torch.where(assign >= 0, score, torch.zeros_like(score)).double().mean())
            order, offsets = ivf_group(assign, self.nlist)
            cent = ivf_centroid_update(x, order, offsets, cent, ws)
        self.train_objective = [float(v) for v in objective]
        self._centroids = cent

    # ---- the inverted lists
    @property
    def vectors(self) -> torch.Tensor:
        """The stored rows [ntotal, dim] in the storage dtype, grouped by list (a view)."""
        return self._rows

    @property
    def ids(self) -> torch.Tensor:
        """The original id of every grouped row [ntotal] int64."""
        return self._ids

    def list_sizes(self) -> np.ndarray:
        return np.diff(self._host_offsets)

    def reset(self) -> None:
        """Drop the stored rows; the trained centroids stay."""
        self.ntotal, self.metadata = 0, None
        self._rows = torch.empty(0, self.dim, dtype=self._tdt, device=self.device)      # not views: the table is freed
        self._ids = torch.empty(0, dtype=torch.int64, device=self.device)
        self._lists = torch.empty(0, dtype=torch.int32, device=self.device)
        self._offsets = torch.zeros(self.nlist + 1, dtype=torch.int64, device=self.device)
        self._host_offsets = np.zeros(self.nlist + 1, np.int64)

    def add(self, x) -> None:
        """Rows get the sequential ids ntotal, ntotal + 1, ... (as under FAISS) and join the list of their best
        centroid; the table is regrouped (stable: ascending id within a list), so add(a); add(b) stores what
        add(cat(a, b)) stores.  The row is assigned as stored (bf16 storage: after the rounding), so a stored
        vector used as a query probes its own list first; a row with no non-NaN score goes to list 0.

        Cost: every call concatenates, stable-sorts and gathers the WHOLE table (peak memory about twice the
        table) and copies the nlist + 1 offsets back to the host, so k small adds cost O(k * ntotal); add in
        large batches.  Merging into the grouped table instead would keep the same contract; it is not built."""
        if not self.is_trained:
            raise RuntimeError("train the index before add")
        x = _f32_rows(x, self.device, self.dim)
        rows = x.shape[0]
        if not rows:
            return
        if self.ntotal + rows >= 1 << 31:
            raise ValueError("ids must stay below 2^31")
        if self.normalize:
            x = l2_normalize(x, F_NORMALIZE_EPS, 0)
        stored = torch.empty(rows, self.dim, dtype=self._tdt, device=self.device)
        N.check(N.lib().vcap_ip_index_convert(x.data_ptr(), self.dim, rows, self.dim, self._dt, stored.data_ptr(),
                                              _stream(self.device)), "vcap_ip_index_convert")
        assign, _ = ivf_assign(stored if self.storage == "f32" else stored.float(), self._centroids, False)
        lists = torch.cat([self._lists, assign.clamp_min(0)])
        order = torch.sort(lists.to(torch.int64), stable=True).indices
        ids = torch.cat([self._ids, torch.arange(self.ntotal, self.ntotal + rows, dtype=torch.int64, device=self.device)])
        self._rows = torch.cat([self._rows, stored])[order].contiguous()
        self._ids, self._lists = ids[order].contiguous(), lists[order].contiguous()
        self._offsets = torch.zeros(self.nlist + 1, dtype=torch.int64, device=self.device)
        self._offsets[1:] = torch.cumsum(torch.bincount(self._lists.to(torch.int64), minlength=self.nlist), 0)
        self._host_offsets = self._offsets.cpu().numpy()       # the scan grid is sized from the longest list
        self.ntotal += rows

    # ---- search
    def _search(self, q, k: int, max_blocks: int, want_probes: bool):
        if not self.is_trained:
            raise RuntimeError("train the index before search")
        if not 1 <= k <= MAX_K:
            raise ValueError(f"k must be in 1..{MAX_K}")
        q = _f32_rows(q, self.device, self.dim)
        nq = q.shape[0]
        nprobe = max(1, min(self.nprobe, self.nlist, MAX_NPROBE))
        D = torch.empty(nq, k, dtype=torch.float32, device=self.device)
        I = torch.empty(nq, k, dtype=torch.int64, device=self.device)
        P = torch.empty(nq, nprobe, dtype=torch.int64, device=self.device) if want_probes else None
        rows = self._rows if self.ntotal else torch.empty(1, self.dim, dtype=self._tdt, device=self.device)
        ids = self._ids if self.ntotal else torch.zeros(1, dtype=torch.int64, device=self.device)
        longest = int(np.diff(self._host_offsets).max())
        lib = N.lib()
        chunk = min(MAX_NQ, MAX_QUERY_FLOATS // self.dim)
        for s in range(0, nq, chunk):
            part = q[s:s + chunk]
            need = int(lib.vcap_ivf_search_workspace_bytes(self.nlist, longest, self.dim, part.shape[0], nprobe, k))
            if need == 0:
                raise N.VcapError(f"vcap_ivf_search_workspace_bytes refused: {(lib.vcap_last_error() or b'').decode()}")
            if self._ws is None or self._ws.numel() < need:
                self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
            N.check(lib.vcap_ivf_search(self._dt, rows.data_ptr(), ids.data_ptr(), self._offsets.data_ptr(), self.ntotal,
                                        self._centroids.data_ptr(), self.nlist, longest, self.dim, part.data_ptr(),
                                        part.shape[0], nprobe, k, D[s:s + chunk].data_ptr(), I[s:s + chunk].data_ptr(),
                                        P[s:s + chunk].data_ptr() if want_probes else None, self._ws.data_ptr(),
                                        self._ws.numel(), max_blocks, _stream(self.device)), "vcap_ivf_search")
        return D, I, P

    def search(self, q, k: int, max_blocks: int = 0):
        """q [nq, dim] (torch or numpy, any nq) -> (D [nq, k] f32, I [nq, k] int64) on the index's device: the
        exact top-k over the rows of the min(nprobe, nlist) lists each query probes."""
        D, I, _ = self._search(q, k, max_blocks, False)
        return D, I

    def probe_lists(self, q) -> torch.Tensor:
        """The list ids [nq, min(nprobe, nlist)] int64 the search scans for each query, best centroid first
        (-1 where fewer centroids have a non-NaN score), as the search call itself reports them.  For tests and
        diagnostics: it costs a whole search call (coarse stage, list scan and merge at k = 1), not the coarse
        stage alone."""
        return self._search(q, 1, 0, True)[2]

    # ---- persistence: index.json ("type": "IVF_FLAT") + centroids.npy + vectors.npy (grouped) + ids.npy + offsets.npy
    def save(self, directory) -> None:
        if not self.is_trained:
            raise RuntimeError("train the index before save")
        d = Path(directory)
        d.mkdir(parents=True, exist_ok=True)
        v = self._rows
        arr = v.cpu().numpy() if self.storage == "f32" else v.view(torch.int16).cpu().numpy().view(np.uint16)
        np.save(d / "vectors.npy", arr)
        np.save(d / "centroids.npy", self._centroids.cpu().numpy())
        np.save(d / "ids.npy", self._ids.cpu().numpy())
        np.save(d / "offsets.npy", self._host_offsets)
        (d / "index.json").write_text(json.dumps({"type": "IVF_FLAT", "dim": self.dim, "storage": self.storage,
                                                  "ntotal": self.ntotal, "normalize": self.normalize,
                                                  "nlist": self.nlist, "nprobe": self.nprobe}))
        if self.metadata is not None:
            write_meta(d / "meta.json", self.metadata)

    @classmethod
    def load(cls, directory, device="cuda") -> "IVFFlatIPIndex":
        d = Path(directory)
        info = json.loads((d / "index.json").read_text())
        if info.get("type") != "IVF_FLAT":
            raise ValueError(f"{d} does not hold an IVF_FLAT index")
        idx = cls(info["dim"], info["nlist"], info["storage"], device, info.get("normalize", False), info.get("nprobe", 1))
        arr, cent = np.load(d / "vectors.npy"), np.load(d / "centroids.npy")
        ids, offsets = np.load(d / "ids.npy"), np.load(d / "offsets.npy")
        n = info["ntotal"]
        if arr.shape != (n, idx.dim) or cent.shape != (idx.nlist, idx.dim) or ids.shape != (n,) or \
                offsets.shape != (idx.nlist + 1,) or offsets[0] != 0 or offsets[-1] != n or (np.diff(offsets) < 0).any():
            raise ValueError(f"the arrays under {d} do not match index.json")
        if n and (np.sort(ids) != np.arange(n)).any():
            raise ValueError(f"{d / 'ids.npy'} is not a permutation of 0..ntotal-1")
        idx._centroids = torch.from_numpy(cent.astype(np.float32)).to(idx.device).contiguous()
        t = torch.from_numpy(arr) if info["storage"] == "f32" else torch.from_numpy(arr.view(np.int16)).view(torch.bfloat16)
        idx._rows = t.to(idx.device).contiguous()              # stored bits, not re-normalised or re-assigned
        idx._ids = torch.from_numpy(ids.astype(np.int64)).to(idx.device)
        idx._host_offsets = offsets.astype(np.int64)
        idx._offsets = torch.from_numpy(idx._host_offsets).to(idx.device)
        idx._lists = torch.repeat_interleave(torch.arange(idx.nlist, dtype=torch.int32, device=idx.device),
                                             torch.from_numpy(np.diff(idx._host_offsets)).to(idx.device))
        idx.ntotal = n
        if (d / "meta.json").exists():
            idx.metadata = json.loads((d / "meta.json").read_text("utf-8"))
        return idx


def load_index(directory, device="cuda"):
    """The index a directory holds: index.json's "type" picks the class; a directory without one is a
    flat index (everything written before the key existed)."""
    kind = json.loads((Path(directory) / "index.json").read_text()).get("type", "Flat")
    if kind == "IVF_FLAT":
        return IVFFlatIPIndex.load(directory, device)
    if kind == "Flat":
        return FlatIPIndex.load(directory, device)
    raise ValueError(f"unknown index type {kind!r} in {Path(directory) / 'index.json'}")


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
        self._f32: Dict[str, torch.Tensor] = {}      # name -> the f32 device tensor the descriptor points at
        self._packed: Dict[str, torch.Tensor] = {}   # name -> the rows-packed operand copy
        self._tr: Dict[str, torch.Tensor] = {}       # name -> the transposed operand copy (enable_grad)
        self._host_w: Dict[str, np.ndarray] = {}     # projection weights until enable_grad uploads their transposes
        self.grad_desc = None
        self._gws: Optional[torch.Tensor] = None
        dev = self.device

        def f32(k):
            t = torch.from_numpy(sd[k]).to(dev).contiguous()
            self._keep.append(t)
            self._f32[k] = t
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
            self._packed[k] = p
            self._host_w[k] = sd[k]
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

    # ---- training: vcap_text_encode_backward
    _PROJ = ("self_attn.in_proj_weight", "self_attn.out_proj.weight", "linear1.weight", "linear2.weight")
    _LAYER_GRADS = (("in_w", "self_attn.in_proj_weight"), ("in_b", "self_attn.in_proj_bias"),
                    ("out_w", "self_attn.out_proj.weight"), ("out_b", "self_attn.out_proj.bias"),
                    ("ln1_g", "norm1.weight"), ("ln1_b", "norm1.bias"), ("fc1_w", "linear1.weight"),
                    ("fc1_b", "linear1.bias"), ("fc2_w", "linear2.weight"), ("fc2_b", "linear2.bias"),
                    ("ln2_g", "norm2.weight"), ("ln2_b", "norm2.bias"))

    def param_names(self) -> List[str]:
        """The state dict's names of the tower's parameters, in the state dict's order."""
        names = ["txt_emb.weight"]
        for i in range(self.n_layer):
            names += [f"txt_enc.layers.{i}.{k}" for _, k in self._LAYER_GRADS]
        return names + ["txt_proj.weight", "txt_proj.bias"]

    def enable_grad(self) -> "HipTextEmbedder":
        """Upload the operand-dtype transposed ([in, out]) copies of the projection weights the backward's
        dx = dy . W products read (from the host copies kept since construction / the last load_state_dict)."""
        if self.grad_desc is not None:
            return self
        tdt = _TEXT_DTYPE[self.dtype][1]
        self._glayers = (N.TextGradLayer * max(self.n_layer, 1))()
        for i in range(self.n_layer):
            b = f"txt_enc.layers.{i}."
            for field, k in zip(("in_t", "out_t", "fc1_t", "fc2_t"), self._PROJ):
                rows, kk = self._shape_of(b + k)
                t = torch.from_numpy(self._host_w[b + k]).to(self.device).to(tdt).t().contiguous()
                self._tr[b + k] = t
                setattr(self._glayers[i], field, t.data_ptr())
        self.grad_desc = N.TextGradDesc(dtype=self.dt, dim=self.dim, ffn=self.ffn, n_layer=self.n_layer,
                                        layers=self._glayers)
        self._host_w = {}          # the transposed copies follow load_state_dict from here on
        return self

    def _shape_of(self, k: str):
        E, F = self.dim, self.ffn
        return {"self_attn.in_proj_weight": (3 * E, E), "self_attn.out_proj.weight": (E, E),
                "linear1.weight": (F, E), "linear2.weight": (E, F)}[k.split(".", 3)[3]]

    def load_state_dict(self, sd) -> None:
        """Rewrite every device weight in place from `sd` (numpy or torch values under the state dict's
        names): the f32 tensors, the rows-packed forward operands and, after enable_grad, the transposed
        copies.  No pointer of desc / grad_desc changes and nothing is reallocated."""
        tdt = _TEXT_DTYPE[self.dtype][1]
        if isinstance(sd, dict) and "model_state" in sd:
            sd = sd["model_state"]
        lib = N.lib()

        def dev(k):
            v = sd[k]
            v = v.detach() if hasattr(v, "detach") else torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32))
            return v.to(device=self.device, dtype=torch.float32)

        for k, t in self._f32.items():
            v = dev(k)
            if v.shape != t.shape:
                raise ValueError(f"{k}: shape {tuple(v.shape)} does not match the embedder's {tuple(t.shape)}")
            t.copy_(v)
        for k, p in self._packed.items():
            w = dev(k).to(tdt).contiguous()
            rows, kk = w.shape
            if (rows, kk) != self._shape_of(k):
                raise ValueError(f"{k}: shape {tuple(w.shape)} does not match the embedder's")
            N.check(lib.vcap_rows_pack(self.dt, w.data_ptr(), w.stride(0), rows, kk, p.data_ptr(), _stream(self.device)),
                    "vcap_rows_pack")
            if k in self._tr:
                self._tr[k].copy_(w.t())
            else:
                self._host_w[k] = dev(k).cpu().numpy()

    def _backward_chunk(self, t: torch.Tensor, g: torch.Tensor, out: torch.Tensor) -> Dict[str, object]:
        """One vcap_text_encode_backward call: ids t [n, L] int32, grad_out g [n, P] -> out [n, P] filled;
        returns {name: f32 tensor}, the embedding gradient as (ids int64 [count], rows [count, E]), and the
        ABI's untrimmed (emb_ids [M], emb_rows [M, E], count)."""
        n, L = t.shape
        M, E, F, P, lib, dev = n * L, self.dim, self.ffn, self.proj_dim, N.lib(), self.device
        shapes = {"in_w": (3 * E, E), "in_b": (3 * E,), "out_w": (E, E), "out_b": (E,), "ln1_g": (E,), "ln1_b": (E,),
                  "fc1_w": (F, E), "fc1_b": (F,), "fc2_w": (E, F), "fc2_b": (E,), "ln2_g": (E,), "ln2_b": (E,)}
        res: Dict[str, object] = {}
        glayers = (N.TextParamGradsLayer * max(self.n_layer, 1))()
        for i in range(self.n_layer):
            for field, k in self._LAYER_GRADS:
                buf = torch.empty(shapes[field], dtype=torch.float32, device=dev)
                res[f"txt_enc.layers.{i}.{k}"] = buf
                setattr(glayers[i], field, buf.data_ptr())
        pw = torch.empty(P, E, dtype=torch.float32, device=dev)
        pb = torch.empty(P, dtype=torch.float32, device=dev)
        eids = torch.empty(M, dtype=torch.int32, device=dev)
        erows = torch.empty(M, E, dtype=torch.float32, device=dev)
        cnt = torch.empty(1, dtype=torch.int32, device=dev)
        grads = N.TextParamGrads(proj_w=pw.data_ptr(), proj_b=pb.data_ptr(), emb_ids=eids.data_ptr(),
                                 emb_rows=erows.data_ptr(), emb_count=cnt.data_ptr(), layers=glayers)
        need = int(lib.vcap_text_encode_backward_workspace_bytes(C.byref(self.desc), C.byref(self.grad_desc), n, L))
        if need == 0:
            raise N.VcapError(f"vcap_text_encode_backward_workspace_bytes refused B={n}, L={L}: "
                              f"{(lib.vcap_last_error() or b'').decode()}")
        if self._gws is None or self._gws.numel() < need:
            self._gws = torch.empty(need, dtype=torch.uint8, device=dev)
        N.check(lib.vcap_text_encode_backward(C.byref(self.desc), C.byref(self.grad_desc), t.data_ptr(), n, L,
                                              g.data_ptr(), C.byref(grads), out.data_ptr(), self._gws.data_ptr(),
                                              self._gws.numel(), _stream(dev)), "vcap_text_encode_backward")
        c = int(cnt.item())
        res["txt_emb.weight"] = (eids[:c].long(), erows[:c])
        res["txt_proj.weight"], res["txt_proj.bias"] = pw, pb
        return res, (eids, erows, c)

    def encode_text_backward(self, ids, grad_out):
        """ids [B, L], grad_out [B, proj_dim] (d scalar / d out) -> (out [B, proj_dim], grads).  grads maps the
        state dict's names to f32 device tensors in torch's layouts; "txt_emb.weight" comes back row-sparse as
        (ids int64 [count] ascending, rows [count, dim]) - embedding_grad_dense() scatters it.  Batches of more
        than max_rows / L captions go in chunks whose gradients are added in chunk order, the embedding rows
        merged by id."""
        if self.grad_desc is None:
            raise RuntimeError("encode_text_backward needs enable_grad() first")
        t = self._ids(ids)
        B, L = t.shape
        g = torch.as_tensor(grad_out).to(device=self.device, dtype=torch.float32).contiguous()
        if g.shape != (B, self.proj_dim):
            raise ValueError(f"grad_out must be [{B}, {self.proj_dim}], got {tuple(g.shape)}")
        out = torch.empty(B, self.proj_dim, dtype=torch.float32, device=self.device)
        per, total = max(1, self.max_rows // L), None
        for s in range(0, B, per):
            n = min(per, B - s)
            part, _ = self._backward_chunk(t[s:s + n], g[s:s + n], out[s:s + n])
            total = part if total is None else self._merge(total, part)
        return out, total

    @staticmethod
    def _merge(a: Dict[str, object], b: Dict[str, object]) -> Dict[str, object]:
        res: Dict[str, object] = {}
        for k, v in a.items():
            if k != "txt_emb.weight":
                res[k] = v + b[k]
                continue
            (ia, ra), (ib, rb) = v, b[k]
            ids = torch.unique(torch.cat([ia, ib]))          # sorted
            rows = torch.zeros(ids.numel(), ra.shape[1], dtype=ra.dtype, device=ra.device)
            rows.index_copy_(0, torch.searchsorted(ids, ia), ra)        # each chunk's ids are distinct
            rows.index_add_(0, torch.searchsorted(ids, ib), rb)         # distinct too: one add per row
            res[k] = (ids, rows)
        return res

    def embedding_grad_dense(self, sparse) -> torch.Tensor:
        """(ids, rows) -> the dense [vocab, dim] gradient of txt_emb.weight: zeros but the listed rows (the
        ids are distinct, so index_copy_ is deterministic; the pad row stays zero)."""
        ids, rows = sparse
        dense = torch.zeros(self.vocab, self.dim, dtype=torch.float32, device=rows.device)
        return dense.index_copy_(0, ids, rows)


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
