"""GPU frame preprocessing (vcap_frames_preprocess) against PIL itself and the reference's
transform chain (core/preprocessing/frame_loader.py:34-45): resized pixels bit-identical to
PIL Image.resize(BILINEAR) (integer parity), normalised f32 bit-identical to ToTensor + Normalize
on those pixels (oracle.frames_to_tensor restates the chain; PIL is the resize oracle)."""
import numpy as np
import pytest
import torch
from PIL import Image

from oracle import vcap_oracle as O
from vcap.preprocess import preprocess_frames

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("hw", [(240, 320), (360, 480), (224, 224), (100, 150), (1080, 1920), (224, 300),
                                (300, 224), (37, 500)])
def test_preprocess_bit_exact_vs_pil(device, hw):
    h, w = hw
    g = np.random.default_rng(h + 3 * w)
    frames = np.stack([g.integers(0, 256, (h, w, 3), dtype=np.uint8),
                       (np.add.outer(np.arange(h), 3 * np.arange(w))[:, :, None] * np.array([1, 2, 5]) % 256)
                       .astype(np.uint8)])
    out, u8 = preprocess_frames(torch.from_numpy(frames).to(device), 224, out_u8=True)
    torch.cuda.synchronize()
    ref_u8 = np.stack([np.asarray(Image.fromarray(f).resize((224, 224), Image.BILINEAR)) for f in frames])
    assert np.array_equal(u8.cpu().numpy(), ref_u8)
    assert np.array_equal(out.cpu().numpy(), O.frames_to_tensor(frames, 224))


def test_loader_hip_matches_pil_backend(device, tmp_path):
    """core.preprocessing.load_video_tensor: GPU path == host PIL path on real JPEG files."""
    from core.preprocessing.frame_loader import load_video_tensor
    g = np.random.default_rng(5)
    for i in range(20):
        img = (g.random((180, 320, 3)) * 255).astype(np.uint8)
        Image.fromarray(img).save(tmp_path / f"frame_{i:04d}.jpg", quality=90)
    a = load_video_tensor(tmp_path, 8, 224, device=str(device), backend="hip")
    b = load_video_tensor(tmp_path, 8, 224, device="cpu", backend="pil")
    assert a.shape == (1, 8, 3, 224, 224)
    assert torch.equal(a.cpu(), b)


# ---------------------------------------------------------------------------------------------------------
# The sweep: vcap_frames_preprocess through the C ABI (so that out_h != out_w is reachable), every output buffer
# with a sentinel tail.  Resized bytes against PIL Image.resize(BILINEAR), f32 against the oracle's normalise chain
# (oracle.frames_to_tensor's two lines, here with the case's own mean / std) on those bytes; both bit-exact.
import ctypes as C  # noqa: E402

from vcap import _native as N  # noqa: E402

IMAGENET = ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
CUSTOM = ((0.1, 0.5, 0.9), (0.3, 0.25, 1.7))
TAIL = 64


def _frames(n, h, w, seed):
    """Even frames: 0/255 stripes (R: alternating columns, G: alternating rows, B: both), which put the largest step
    under every weight and reach the clamp; odd frames: random bytes."""
    g = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    out = []
    for k in range(n):
        ph = (k // 2) % 2
        stripes = np.stack([(xx + ph) % 2, (yy + ph) % 2, (xx + yy + ph) % 2], -1) * 255
        out.append(stripes.astype(np.uint8) if k % 2 == 0 else g.integers(0, 256, (h, w, 3), dtype=np.uint8))
    return np.stack(out)


def _normalise(u8, mean, std):
    m = np.array(mean, np.float32)[:, None, None]
    s = np.array(std, np.float32)[:, None, None]
    return np.stack([(r.transpose(2, 0, 1).astype(np.float32) / np.float32(255.0) - m) / s for r in u8])


def _call(device, frames, out_h, out_w, norm=IMAGENET, want=("out", "u8")):
    n, h, w, _ = frames.shape
    lib = N.lib()
    x = torch.from_numpy(frames).to(device)
    out = torch.full((n * 3 * out_h * out_w + TAIL,), -7.0, dtype=torch.float32, device=device)
    u8 = torch.full((n * out_h * out_w * 3 + TAIL,), 77, dtype=torch.uint8, device=device)
    nbytes = int(lib.vcap_frames_workspace_bytes(n, h, w, out_h, out_w))
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=device)
    rc = lib.vcap_frames_preprocess(x.data_ptr(), n, h, w, out_h, out_w, (C.c_float * 3)(*norm[0]), (C.c_float * 3)(*norm[1]),
                                    out.data_ptr() if "out" in want else None, u8.data_ptr() if "u8" in want else None,
                                    ws.data_ptr(), nbytes, torch.cuda.current_stream(device).cuda_stream)
    torch.cuda.synchronize()
    return int(rc), out.cpu().numpy(), u8.cpu().numpy()


# (name, n, (in_h, in_w), (out_h, out_w))
SWEEP = [
    ("out_8x8", 2, (20, 30), (8, 8)), ("out_16x24", 2, (37, 50), (16, 24)), ("out_32x32", 2, (45, 33), (32, 32)),
    ("out_224x112", 2, (100, 150), (224, 112)), ("out_1x1", 2, (5, 7), (1, 1)),
    ("in_1x1", 2, (1, 1), (8, 8)), ("in_1x7", 2, (1, 7), (8, 8)), ("in_2x3", 2, (2, 3), (16, 24)), ("in_3x2", 2, (3, 2), (8, 8)),
    ("only_horizontal", 2, (8, 20), (8, 8)), ("only_vertical", 2, (20, 8), (8, 8)), ("identity", 2, (8, 8), (8, 8)),
    # the downscale cap: ksize = ceil(in / out) * 2 + 1 <= 64 (csrc/preprocess.hip axis_of; the kernel's w[64]), i.e.
    # in <= 31 * out (runtime.hip's refusal): 248 -> 8 is the last accepted factor, 63 taps
    ("cap_width_248_to_8", 2, (16, 248), (8, 8)), ("cap_height_248_to_8", 2, (248, 16), (8, 8)),
    ("cap_both_axes", 2, (248, 248), (8, 8)),
    ("below_cap_247_to_8_width", 2, (16, 247), (8, 8)), ("below_cap_247_to_8_height", 2, (247, 16), (8, 8)),
    ("below_cap_495_to_16_width", 2, (12, 495), (8, 16)), ("below_cap_495_to_16_height", 2, (495, 12), (16, 8)),
    ("n_1", 1, (19, 23), (8, 8)), ("n_3", 3, (19, 23), (16, 24)), ("n_17", 17, (19, 23), (8, 8)),
]


@pytest.mark.parametrize("name, n, in_hw, out_hw", SWEEP, ids=[s[0] for s in SWEEP])
def test_sweep_bit_exact_vs_pil_and_the_normalise_chain(device, name, n, in_hw, out_hw):
    (oh, ow), norm = out_hw, CUSTOM if len(name) % 2 else IMAGENET
    frames = _frames(n, *in_hw, seed=len(name) + 31 * n)
    ref_u8 = np.stack([np.asarray(Image.fromarray(f).resize((ow, oh), Image.BILINEAR)) for f in frames])
    ref = _normalise(ref_u8, *norm)
    rc, out, u8 = _call(device, frames, oh, ow, norm)
    assert rc == 0
    assert np.array_equal(u8[:-TAIL].reshape(ref_u8.shape), ref_u8) and (u8[-TAIL:] == 77).all()
    assert np.array_equal(out[:-TAIL].reshape(ref.shape).view(np.uint32), ref.view(np.uint32)) and (out[-TAIL:] == -7.0).all()


def test_sweep_uses_both_normalisations():
    assert {len(s[0]) % 2 for s in SWEEP} == {0, 1} and CUSTOM[0] != CUSTOM[1] and len(set(CUSTOM[0]) | set(CUSTOM[1])) == 6


def test_normalise_chain_is_the_oracles():
    frames = _frames(2, 30, 40, 5)
    u8 = np.stack([np.asarray(Image.fromarray(f).resize((16, 16), Image.BILINEAR)) for f in frames])
    assert np.array_equal(_normalise(u8, *IMAGENET), O.frames_to_tensor(frames, 16))


@pytest.mark.parametrize("want", [("out",), ("u8",), ("out", "u8")], ids=["out_only", "u8_only", "both"])
def test_either_output_alone_leaves_the_other_untouched(device, want):
    frames = _frames(3, 21, 34, 9)
    ref_u8 = np.stack([np.asarray(Image.fromarray(f).resize((24, 16), Image.BILINEAR)) for f in frames])
    rc, out, u8 = _call(device, frames, 16, 24, CUSTOM, want)
    assert rc == 0
    if "u8" in want:
        assert np.array_equal(u8[:-TAIL].reshape(ref_u8.shape), ref_u8)
    else:
        assert (u8 == 77).all()
    if "out" in want:
        assert np.array_equal(out[:-TAIL].reshape(3, 3, 16, 24), _normalise(ref_u8, *CUSTOM))
    else:
        assert (out == -7.0).all()


@pytest.mark.parametrize("in_hw", [(16, 249), (249, 16)], ids=["width_249_to_8", "height_249_to_8"])
def test_downscale_factor_above_31_is_refused(device, in_hw):
    rc, out, u8 = _call(device, _frames(1, *in_hw, seed=1), 8, 8)
    assert rc == N.E_UNSUPPORTED and N.lib().vcap_last_error() == b"vcap_frames_preprocess: downscale factor above 31"
    assert (out == -7.0).all() and (u8 == 77).all()
