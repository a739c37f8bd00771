"""The JPEG decode (vcap_jpeg_decode_batch: host parse + entropy decode, device dequantise + islow IDCT + fancy
upsampling + YCbCr -> RGB) over the case table of tests/jpeg_cases.py, whose expectations test_cpu_jpeg_cases.py
pins to libjpeg's C path: streams no encoder of real pixels writes (long Huffman codes, every run/size shape,
DC / AC values at the limit of the entropy coding, 16-bit and signed-wrapping quantisers, table ids 2 and 3,
merged segments, fill bytes, every accepted chroma layout down to a downsampled width of 3).  Every comparison is
array_equal against the oracle; cases tagged "in" are compared with Pillow's own decode as well."""
import io
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch
from PIL import Image

import jpeg_cases as JC
from vcap import _native as N
from vcap.jpeg import decode_jpegs

pytestmark = pytest.mark.gpu
HERE = Path(__file__).resolve().parent
ACCEPTED, REFUSED = JC.accepted(), JC.refused()
CODES = {"ARG": N.E_ARG, "UNSUPPORTED": N.E_UNSUPPORTED}


def _decode(cases, device):
    got = decode_jpegs([c.data for c in cases], device)
    torch.cuda.synchronize()
    return got.cpu().numpy()


@pytest.mark.parametrize("case", ACCEPTED, ids=[c.name for c in ACCEPTED])
def test_case_equals_oracle(device, case):
    got = _decode([case], device)[0]
    assert np.array_equal(got, JC.expected(case))
    if case.tag == "in":
        assert np.array_equal(got, np.asarray(Image.open(io.BytesIO(case.data)).convert("RGB")))


@pytest.mark.parametrize("key, n", [("b420", 6), ("b420", 1), ("b420", 3), ("b420", 33), ("bgrey", 3), ("bgrey", 33),
                                    ("b64", 4)])
def test_batch_each_image_equals_its_own_expectation(device, key, n):
    """One call, images of one size and sampling that differ in Huffman tables, restart interval, component ids and
    quantisation tables (one of them 16-bit): the image index strides the per-image tables.  33 images: the block
    count is no multiple of the IDCT kernel's 32 blocks per workgroup (16 Y and 4 + 4 chroma blocks per image, or 6)."""
    members = JC.batch(key)
    cases = [members[(5 * k) % len(members)] for k in range(n)] if n > len(members) else members[:n]
    if n > len(members):
        assert {c.name for c in cases} == {c.name for c in members}
    got = _decode(cases, device)
    for k, c in enumerate(cases):
        assert np.array_equal(got[k], JC.expected(c)), (k, c.name)


def test_staging_buffer_grows_and_is_reused_across_calls_streams_and_threads():
    """tests/jpeg_stage_worker.py, in a fresh process so that the buffer's first allocation and its growth happen."""
    r = subprocess.run([sys.executable, str(HERE / "jpeg_stage_worker.py")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().splitlines()[-1] == "ok", r.stdout + r.stderr


@pytest.mark.parametrize("case", REFUSED, ids=[c.name for c in REFUSED])
def test_refused_case_raises_the_listed_code(device, case):
    with pytest.raises(N.VcapError) as e:
        decode_jpegs([case.data], device)
    assert e.value.rc == CODES[case.refuse]
    with pytest.raises(N.VcapError) as e:                     # as a later image of a batch too
        decode_jpegs([JC.case("samp_444_19x13").data, case.data], device)
    assert e.value.rc == CODES[case.refuse]


@pytest.mark.parametrize("case", [c for c in REFUSED if c.narrow], ids=[c.name for c in REFUSED if c.narrow])
def test_narrow_chroma_decodes_by_the_pil_fallback(device, tmp_path, case):
    """A downsampled chroma width of 2 or less (libjpeg upsamples it without the triangle filter) is refused by the
    device decoder; load_video_tensor(backend="auto") falls back to PIL for it and equals the PIL path."""
    from core.preprocessing.frame_loader import load_video_tensor
    for i in range(2):
        (tmp_path / f"frame_{i:04d}.jpg").write_bytes(case.data)
    got = load_video_tensor(tmp_path, 2, 32, device=str(device), backend="auto")
    ref = load_video_tensor(tmp_path, 2, 32, device="cpu", backend="pil")
    assert got.shape == (1, 2, 3, 32, 32) and torch.equal(got.cpu(), ref)
    with pytest.raises(N.VcapError) as e:
        load_video_tensor(tmp_path, 2, 32, device=str(device), backend="hip")
    assert e.value.rc == N.E_UNSUPPORTED
