"""Child process of test_gpu_graph_cache.py: greedy, sampling and beam decodes through one tiny fp32
decoder with the graph cache capped at two entries (VCAP_GRAPH_CACHE_MAX, which the library reads
once per process and the parent sets).  Every check is an assert; the last line printed is "ok"."""
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "video-caption-algorithm_amd"))

import torch  # noqa: E402

from vcap import _native as N  # noqa: E402
from vcap import configs, weights  # noqa: E402
from vcap.model import GenConfig, HipGPT2Decoder  # noqa: E402

B, MAX_NEW, CAP = 2, 6, 2


def main():
    dev = torch.device("cuda:0")
    ga = configs.gpt2_arch("gpt2_tiny_test")
    sd = weights.synthetic_state_dict(1, configs.vit_arch("vit_tiny_test"), ga)
    dec = HipGPT2Decoder(sd, ga, "fp32", dev)
    lib = N.lib()
    prefix = (torch.rand(B, dec.prefix_len, ga.n_embd, generator=torch.Generator().manual_seed(3)) - 0.5).to(dev)
    eos = ga.eos_token_id

    def size():
        n = int(lib.vcap_graph_cache_size())
        assert n <= CAP, n
        return n

    def greedy(prompt, out, use_graph=True):
        dec.generate_ids(prefix, prompt, GenConfig(MAX_NEW, 2, 3, 1.1, eos, eos, use_graph), out=out)
        torch.cuda.synchronize()
        return out.cpu().numpy().copy()

    outs = {k: torch.empty(B, MAX_NEW, dtype=torch.int32, device=dev) for k in "ABCE"}
    prompts = {"A": [eos], "B": [5], "C": [7]}
    assert size() == 0
    eager_a = greedy(prompts["A"], outs["E"], use_graph=False)
    assert size() == 0                                  # an eager decode caches nothing
    first_a = greedy(prompts["A"], outs["A"])
    assert size() == 1
    greedy(prompts["B"], outs["B"])
    assert size() == 2
    greedy(prompts["C"], outs["C"])                     # evicts A, the least recently used
    assert size() == 2
    again_a = greedy(prompts["A"], outs["A"])           # captured again, evicts B
    assert size() == 2
    assert (again_a == first_a).all() and (again_a == eager_a).all(), (first_a, again_a, eager_a)

    # a sampling graph and a beam graph go through the same bounded cache
    force = torch.tensor([[3, 4, 5, 6, 7, 8], [9, 10, 11, 12, 13, 14]], dtype=torch.int32, device=dev)
    out_s = torch.empty(B, MAX_NEW, dtype=torch.int32, device=dev)
    dec.generate_ids(prefix, prompts["A"], GenConfig(MAX_NEW, 2, 3, 1.1, eos, eos, True, temperature=0.7, top_k=20),
                     out=out_s, force_ids=force)
    torch.cuda.synchronize()
    assert size() == 2
    assert (out_s.cpu() == force.cpu()).all(), out_s
    out_b = torch.empty(B, MAX_NEW, dtype=torch.int32, device=dev)
    lens = torch.empty(B, dtype=torch.int32, device=dev)
    dec.generate_ids(prefix, prompts["A"], GenConfig(MAX_NEW, 2, 3, 1.1, eos, eos, True, num_beams=3),
                     out=out_b, lengths_out=lens)
    torch.cuda.synchronize()
    assert size() == 2
    assert ((lens.cpu() >= 1) & (lens.cpu() <= MAX_NEW)).all(), lens

    lib.vcap_graph_cache_clear()
    assert size() == 0
    after = greedy(prompts["A"], outs["A"])
    assert size() == 1
    assert (after == first_a).all(), (first_a, after)
    print("ok", flush=True)


if __name__ == "__main__":
    main()
