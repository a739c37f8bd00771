"""Cases and oracles of the text-tower tests (ViTTextAlignModel.encode_text, vit_text_align.py:67-79).

`tower(name)` builds, from a seed, the torch modules the reference builds - nn.Embedding(padding_idx),
nn.TransformerEncoder of nn.TransformerEncoderLayer(batch_first=True) (post-LN, ReLU, eps 1e-5) or
nn.Identity for 0 layers, nn.Linear - under the reference's attribute names, with non-trivial LayerNorm
affines, biases and pad row (a trained checkpoint's pad row is not zero).

Oracles, all on the CPU:
  * `oracle(case)`: those modules in float64, followed by our restatement of the pool / proj / normalise
    lines.  THE reference of the GPU tests.
  * `np_tower(...)`: a float64 numpy restatement of the whole tower.  It also returns the encoder output
    before the pool (hidden_out), and with rounding="bf16" it rounds where the device's bf16 mode rounds -
    the GEMV operands (activations and weights), the stored q/k/v, the attention output and the ReLU
    output - while every sum stays fp64.  test_cpu_text_tower.py pins it to the torch modules at 1e-10.

Bounds.
  f32 `out`: atol 1e-5, rtol 0 (the project's f32 bar for the projected prefix, test_gpu_parity.py).
  f32 `hidden_out`: 200 x the spread between the torch modules run in float32 and in float64 on the CPU,
    maximised over the whole case table: HIDDEN_F32_SPREAD (measured by `measure_f32_spread()`, value
    below), so HIDDEN_ATOL = 200 * HIDDEN_F32_SPREAD.  The same factor as for `out`, whose spread is 5e-8.
  bf16: nothing fixed in advance.  Per case, budget = max |np_tower(rounding="bf16") - np_tower()|, a CPU
    quantity.  The device may deviate from the fp64 oracle by 4 x budget (the budget is a maximum over a
    few hundred entries, not a bound, and other sum orders flip roundings at about ten rounding points)
    plus the f32 bound above: the bf16 mode shares the f32 mode's arithmetic everywhere else, and where a
    case meets no bf16 rounding at all (0 layers; a caption of pads only, whose output is
    normalize(proj.bias)) its budget is exactly 0 and only the f32 error is left.
"""
from __future__ import annotations

import copy
from functools import lru_cache
from typing import Dict, NamedTuple, Optional

import numpy as np
import torch
import torch.nn as nn

# name -> (E, H, F, layers, P, V)
TOWERS = {
    "e128": (128, 2, 512, 2, 64, 97),
    "ref": (512, 8, 2048, 2, 256, 3001),      # the reference's shape (vocabulary cut down)
    "ref_0layers": (512, 8, 2048, 0, 256, 3001),
}
PAD_ID = {"e128": 5, "ref": 0, "ref_0layers": 0}

# (B, L) -> the pad pattern of each caption.  "none": no pad; "trailing": 1..L-1 pads at the end;
# "interior": one pad inside; "allpad": pads only
SHAPES = {
    (1, 1): ["none"],
    (1, 15): ["trailing"],
    (1, 16): ["none"],
    (1, 17): ["interior"],
    (2, 16): ["none", "allpad"],                                   # M = 32
    (3, 11): ["trailing", "interior", "none"],                     # M = 33: past the 32-row chunk
    (5, 33): ["none", "trailing", "interior", "allpad", "trailing"],
    (1, 64): ["trailing"],
    (8, 64): ["none", "trailing", "interior", "allpad", "trailing", "none", "interior", "trailing"],  # the row limit
}


class Case(NamedTuple):
    tower: str
    B: int
    L: int
    pads: tuple

    @property
    def id(self):
        return f"{self.tower}-B{self.B}-L{self.L}" + ("-padonly" if self.pads == ("allpad",) else "")


CASES = [Case(t, B, L, tuple(p)) for t in TOWERS for (B, L), p in SHAPES.items()]
CASES += [Case(t, 1, 1, ("allpad",)) for t in TOWERS]             # L = 1 holding only the pad
CASE_IDS = [c.id for c in CASES]

F32_OUT_ATOL = 1e-5
# max over CASES of |hidden(torch float32) - hidden(torch float64)| on the CPU: measure_f32_spread()
# gave 3.537e-06 (tower "ref", B=8, L=64); values are O(1) after LayerNorm
HIDDEN_F32_SPREAD = 3.537e-6
HIDDEN_ATOL = 200 * HIDDEN_F32_SPREAD


class _TextTower(nn.Module):
    """The text half of the alignment model, under the reference's attribute names."""

    def __init__(self, E, H, F, layers, P, V, pad_id):
        super().__init__()
        self.pad_id = pad_id
        self.txt_emb = nn.Embedding(V, E, padding_idx=pad_id)
        if layers > 0:
            layer = nn.TransformerEncoderLayer(d_model=E, nhead=H, dim_feedforward=F, dropout=0.1, batch_first=True)
            self.txt_enc = nn.TransformerEncoder(layer, num_layers=layers, enable_nested_tensor=False)
        else:
            self.txt_enc = nn.Identity()
        self.txt_proj = nn.Linear(E, P)


@lru_cache(maxsize=None)
def tower(name: str) -> _TextTower:
    """Seeded float32 modules in eval mode; every parameter non-trivial."""
    E, H, F, layers, P, V = TOWERS[name]
    g = torch.Generator().manual_seed(1000 + sorted(TOWERS).index(name))
    m = _TextTower(E, H, F, layers, P, V, PAD_ID[name]).eval()
    with torch.no_grad():
        for k, p in m.named_parameters():
            r = torch.randn(p.shape, generator=g)
            if "norm" in k and k.endswith("weight"):
                p.copy_(1.0 + 0.2 * r)
            elif k.endswith("bias"):
                p.copy_(0.1 * r)
            elif k == "txt_emb.weight":
                p.copy_(r)                                  # N(0, 1) as nn.Embedding, pad row included
            else:
                p.copy_(r / np.sqrt(p.shape[1]))
    return m


def state_dict(name: str) -> Dict[str, np.ndarray]:
    return {k: v.detach().numpy().copy() for k, v in tower(name).state_dict().items()}


@lru_cache(maxsize=None)
def ids_of(case: Case) -> np.ndarray:
    V, pad = TOWERS[case.tower][5], PAD_ID[case.tower]
    rs = np.random.RandomState(7 + 131 * case.B + case.L)
    ids = rs.randint(0, V - 1, size=(case.B, case.L))
    ids[ids >= pad] += 1                                    # every id but the pad
    for b, pat in enumerate(case.pads):
        if pat == "trailing" and case.L > 1:
            ids[b, case.L - rs.randint(1, case.L):] = pad
        elif pat == "interior" and case.L > 2:
            ids[b, rs.randint(1, case.L - 1)] = pad
        elif pat == "allpad":
            ids[b, :] = pad
    return ids.astype(np.int64)


def pool_project(hidden: np.ndarray, ids: np.ndarray, pad_id: int, pw: np.ndarray, pb: np.ndarray) -> np.ndarray:
    """Our restatement of vit_text_align.py:72-78 in float64: masked mean (count >= 1), proj, F.normalize."""
    mask = (ids != pad_id).astype(np.float64)
    pooled = (hidden * mask[..., None]).sum(1) / np.maximum(mask.sum(1, keepdims=True), 1.0)
    y = pooled @ pw.astype(np.float64).T + pb.astype(np.float64)
    return y / np.maximum(np.linalg.norm(y, axis=-1, keepdims=True), 1e-12)


def torch_hidden(name: str, ids: np.ndarray, dtype=torch.float64) -> np.ndarray:
    """txt_enc(txt_emb(ids)) through the torch modules in `dtype` -> float64 numpy [B, L, E]."""
    m = tower(name) if dtype == torch.float32 else _double(name)
    with torch.no_grad():
        return m.txt_enc(m.txt_emb(torch.from_numpy(ids))).double().numpy()


@lru_cache(maxsize=None)
def _double(name: str) -> _TextTower:
    return copy.deepcopy(tower(name)).double().eval()


def oracle_ids(name: str, ids: np.ndarray):
    """(out [B, P], hidden [B, L, E]) float64: the torch modules in float64, then pool_project."""
    sd = state_dict(name)
    hidden = torch_hidden(name, ids)
    return pool_project(hidden, ids, PAD_ID[name], sd["txt_proj.weight"], sd["txt_proj.bias"]), hidden


@lru_cache(maxsize=None)
def oracle(case: Case):
    return oracle_ids(case.tower, ids_of(case))


def bf16_round(x: np.ndarray) -> np.ndarray:
    """float64 -> nearest bf16 (ties to even, through float32 as the device's f32 accumulators go) -> float64."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32).astype(np.float64).reshape(np.shape(x))


def _ln(x, g, b, eps=1e-5):
    mu = x.mean(-1, keepdims=True)
    var = ((x - mu) ** 2).mean(-1, keepdims=True)
    return (x - mu) / np.sqrt(var + eps) * g + b


def np_tower(sd: Dict[str, np.ndarray], ids: np.ndarray, pad_id: int, nhead: int, rounding: Optional[str] = None):
    """(out, hidden) float64 of the whole tower restated in numpy; rounding in (None, "bf16")."""
    rnd = bf16_round if rounding == "bf16" else (lambda a: a)
    w = {k: np.asarray(v, np.float64) for k, v in sd.items()}
    x = w["txt_emb.weight"][ids]                            # [B, L, E]; the pad row as stored
    B, L, E = x.shape
    n_layer = 1 + max((int(k.split(".")[2]) for k in w if k.startswith("txt_enc.layers.")), default=-1)
    for i in range(n_layer):
        p = f"txt_enc.layers.{i}."
        qkv = rnd(rnd(x) @ rnd(w[p + "self_attn.in_proj_weight"]).T + w[p + "self_attn.in_proj_bias"])
        q, k, v = (t.reshape(B, L, nhead, E // nhead).transpose(0, 2, 1, 3) for t in np.split(qkv, 3, axis=-1))
        s = (q / np.sqrt(E // nhead)) @ k.transpose(0, 1, 3, 2)        # no mask: pads are keys and queries
        s = np.exp(s - s.max(-1, keepdims=True))
        a = rnd(((s / s.sum(-1, keepdims=True)) @ v).transpose(0, 2, 1, 3).reshape(B, L, E))
        x = _ln(x + a @ rnd(w[p + "self_attn.out_proj.weight"]).T + w[p + "self_attn.out_proj.bias"],
                w[p + "norm1.weight"], w[p + "norm1.bias"])
        h = rnd(np.maximum(rnd(x) @ rnd(w[p + "linear1.weight"]).T + w[p + "linear1.bias"], 0.0))
        x = _ln(x + h @ rnd(w[p + "linear2.weight"]).T + w[p + "linear2.bias"], w[p + "norm2.weight"], w[p + "norm2.bias"])
    return pool_project(x, ids, pad_id, w["txt_proj.weight"], w["txt_proj.bias"]), x


@lru_cache(maxsize=None)
def restated(case: Case, rounding: Optional[str] = None):
    return np_tower(state_dict(case.tower), ids_of(case), PAD_ID[case.tower], TOWERS[case.tower][1], rounding)


def bf16_budget(case: Case):
    """(out budget, hidden budget): max |bf16-rounded restatement - plain restatement| of the case."""
    (o0, h0), (o1, h1) = restated(case), restated(case, "bf16")
    return float(np.abs(o1 - o0).max()), float(np.abs(h1 - h0).max())


def measure_f32_spread() -> float:
    """max over CASES of |hidden(torch float32) - hidden(torch float64)|: the source of HIDDEN_F32_SPREAD."""
    worst = 0.0
    for c in CASES:
        d = np.abs(torch_hidden(c.tower, ids_of(c), torch.float32) - torch_hidden(c.tower, ids_of(c))).max()
        worst = max(worst, float(d))
    return worst


if __name__ == "__main__":
    print(f"HIDDEN_F32_SPREAD measured: {measure_f32_spread():.3e}")
