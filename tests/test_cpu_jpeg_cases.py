"""The JPEG sweep's case table (tests/jpeg_cases.py) pinned before it judges a kernel (no GPU):
  * the oracle equals Pillow's decode of every accepted case with libjpeg-turbo's SIMD off (its plain C path),
    decoded in one fresh child that sets JSIMD_FORCENONE=1 before PIL is imported;
  * a case tagged "in" also equals Pillow's default (SIMD) decode here, a case tagged "out" differs from it;
  * every case has the property it is named for, read back from its bytes, not from the builder;
  * every arithmetic mutation of the oracle changes some case's expectation;
  * vcap_jpeg_probe / vcap_jpeg_workspace_bytes accept and refuse exactly as listed, with the listed code, and the
    damaged headers the stand-alone sanitizer run (tools/jpeg_host_check.sh) reached are refused."""
import ctypes as C
import io
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
from PIL import Image

import jpeg_cases as JC
from oracle import jpeg_oracle as J
from vcap import _native as N

ACCEPTED, REFUSED = JC.accepted(), JC.refused()
CODES = {"ARG": N.E_ARG, "UNSUPPORTED": N.E_UNSUPPORTED}
_ids = lambda cs: [c.name for c in cs]  # noqa: E731

_CHILD = """
import os, sys
assert os.environ["JSIMD_FORCENONE"] == "1" and "PIL" not in sys.modules and "torch" not in sys.modules
sys.path.insert(0, sys.argv[1])
import io
import numpy as np
from PIL import Image
import jpeg_cases as JC
np.savez(sys.argv[2], **{c.name: np.asarray(Image.open(io.BytesIO(c.data)).convert("RGB")) for c in JC.accepted()})
assert "torch" not in sys.modules
"""


def _pillow(data):
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


@pytest.fixture(scope="module")
def pillow_c_path(tmp_path_factory):
    """Pillow's decode of every accepted case on libjpeg-turbo's C path: one child process, no GPU work."""
    out = tmp_path_factory.mktemp("jsimd_none") / "decoded.npz"
    env = dict(os.environ, JSIMD_FORCENONE="1")
    subprocess.run([sys.executable, "-c", _CHILD, str(Path(__file__).resolve().parent), str(out)], env=env, check=True)
    return np.load(out)


def test_annex_k_tables_are_the_ones_pillow_writes():
    b = io.BytesIO()
    Image.fromarray(np.zeros((16, 16, 3), np.uint8)).save(b, format="JPEG")
    written = J.parse(b.getvalue())["ht"]
    for key, table in JC.STD_HUFF.items():
        assert {(ln, code): s for s, (code, ln) in JC.huff_codes(table).items()} == written[key]


def test_table_has_every_listed_row():
    names = {c.name for c in JC.cases()}
    assert len(JC.cases()) == len(names) and all(len(c.data) < 4096 for c in JC.cases())
    for c in ACCEPTED:
        assert c.tag in ("in", "out") and max(c.meta["width"], c.meta["height"]) <= 64
    assert {c.refuse for c in REFUSED} == {"ARG", "UNSUPPORTED"}
    assert len([c for c in REFUSED if c.refuse == "UNSUPPORTED"]) >= 11 and len([c for c in REFUSED if c.narrow]) == 2


@pytest.mark.parametrize("case", ACCEPTED, ids=_ids(ACCEPTED))
def test_oracle_equals_pillow_c_path(case, pillow_c_path):
    assert np.array_equal(JC.expected(case), pillow_c_path[case.name])


@pytest.mark.parametrize("case", ACCEPTED, ids=_ids(ACCEPTED))
def test_tag_in_range_equals_default_pillow_out_of_range_differs(case):
    same = np.array_equal(JC.expected(case), _pillow(case.data))
    assert same == (case.tag == "in")


@pytest.mark.parametrize("case", ACCEPTED, ids=_ids(ACCEPTED))
def test_header_is_what_the_builder_asked_for(case):
    info, m = J.parse(case.data), case.meta
    assert (info["width"], info["height"], info["restart"]) == (m["width"], m["height"], m["restart"])
    assert [(c["h"], c["v"]) for c in info["comps"]] == m["hv"] and [c["id"] for c in info["comps"]] == m["ids"]
    assert [(c["tq"], c["td"], c["ta"]) for c in info["comps"]] == m["tables"]
    assert [s[0] for s in JC.segments(case.data) if s[0] in (0xC0, 0xC1)] == [m["sof"]]


# ---------------------------------------------------------------------------------------------------------
# the property each case is named for, read from its bytes
def _coefs(name):
    return J.coefficients(J.parse(JC.case(name).data))


def _symbols(blk):
    return [s for s, _, _ in JC.block_symbols(blk[JC.ZIGZAG])]


def _decoded_code_lengths(monkeypatch, name):
    seen = []

    def huff(bits, table):
        code = 0
        for length in range(1, 17):
            code = (code << 1) | bits.bit()
            s = table.get((length, code))
            if s is not None:
                seen.append(length)
                return s
        raise J.JpegError("bad Huffman code")

    monkeypatch.setattr(J, "_huff", huff)
    J.coefficients(J.parse(JC.case(name).data))
    return seen


def _rst(name):
    scan = J.parse(JC.case(name).data)["scan"]
    return [scan[i + 1] for i in range(len(scan) - 1) if scan[i] == 0xFF and 0xD0 <= scan[i + 1] <= 0xD7]


def _q(name):
    return J.parse(JC.case(name).data)["qt"]


def test_amplitude_cases():
    co = _coefs("amp_single_coefficient_each_position")
    for c in co:                                         # 64 blocks, one nonzero each, all 64 positions
        pos = [np.nonzero(b)[0] for b in c.reshape(-1, 64)]
        assert all(len(p) == 1 for p in pos) and sorted(int(p[0]) for p in pos) == list(range(64))
    assert max(int(np.abs(c).max()) for c in _coefs("amp_dense_q1_full_scale_32x16")) >= 800
    dc = _coefs("amp_dc_chain_2047_restart")[0][:, :, 0].reshape(-1)
    diffs = [int(dc[i]) - (0 if i % 5 == 0 else int(dc[i - 1])) for i in range(len(dc))]      # DRI = 5
    assert dc.max() == 2047 and dc.min() == -2047 and 2047 in diffs and -2047 in diffs
    assert int(dc[4]) == 2047 and int(dc[5]) == -2047 and int(dc[9]) == 0 and int(dc[10]) == -2047   # across restarts
    for name, lo, hi in [("amp_ac_1023_q255", 255, 255), ("amp_ac_1023_q16bit", 300, 4000)]:
        co = _coefs(name)
        assert all(c[:, :, 1:].max() == 1023 and c[:, :, 1:].min() == -1023 for c in co)
        assert all(lo <= q[1:].max() <= hi for q in _q(name).values())
    assert all(s[1][0] >> 4 == 1 for s in JC.segments(JC.case("amp_ac_1023_q16bit").data) if s[0] == 0xDB)
    assert min(int(q[1:].min()) for q in _q("amp_q16bit_entry_above_32767").values()) < 0     # the signed multiplier
    for c in _coefs("amp_all_positions_maximal"):
        assert (np.abs(c[:, :, 1:]) == 1023).all() and set(np.abs(c[:, :, 0]).reshape(-1)) <= {0, 2047}
        assert np.abs(c[:, :, 0]).max() == 2047


def test_wrap_case_wraps():
    """The range table's wrap is observable: the same IDCT with a plain clamp gives other samples."""
    clamp = JC.mutated_oracle("range wrap -> clamp")
    for name in ("amp_range_wrap_grey", "amp_dc_chain_2047_restart", "amp_all_positions_maximal"):
        assert not np.array_equal(clamp.decode(JC.case(name).data), JC.expected(JC.case(name)))
    assert np.array_equal(JC.mutated_oracle(None).decode(JC.case("amp_range_wrap_grey").data),
                          JC.expected(JC.case("amp_range_wrap_grey")))


def test_run_size_case():
    for c in _coefs("runsize_zrl3_full_eob_r15"):
        b = [_symbols(c[0, k]) for k in range(4)]
        assert b[0] == [0xF0, 0xF0, 0xF0, (14 << 4) | 6]                     # ZRL x3, then position 63, no EOB
        assert len(b[1]) == 63 and 0x00 not in b[1] and all(s >> 4 == 0 for s in b[1])
        assert b[2] == [0x00]                                                # EOB straight after DC
        assert b[3][-1] >> 4 == 15 and b[3][-1] & 15 and 0x00 not in b[3]    # (15, s) lands on 63 by r alone
        assert c[0, 3][JC.ZIGZAG[47]] != 0 and c[0, 3][JC.ZIGZAG[63]] != 0


@pytest.mark.parametrize("name", ["huff_long_codes", "struct_long_codes_dri_3"])
def test_long_code_cases_decode_only_codes_past_the_lookahead(monkeypatch, name):
    seen = _decoded_code_lengths(monkeypatch, name)
    assert min(seen) >= 10 and max(seen) == 16 and len(set(seen)) >= 4
    assert JC.case(name).stats["lengths"] == {n: seen.count(n) for n in set(seen)}


def test_standard_table_cases_also_reach_the_slow_path(monkeypatch):
    seen = _decoded_code_lengths(monkeypatch, "amp_all_positions_maximal")
    assert seen.count(16) >= 100 and min(seen) <= 9


def test_entropy_and_structure_cases():
    scan = J.parse(JC.case("huff_stuffed_ff00").data)["scan"]
    assert scan.count(b"\xff\x00") >= 64 and scan.count(b"\xff\x00") == JC.case("huff_stuffed_ff00").stats["stuffed"]
    seg = {n: JC.segments(JC.case(n).data) for n in _ids(ACCEPTED)}
    dht = [s for s in seg["huff_ids_2_3_sof1"] if s[0] == 0xC4]
    assert sorted(s[1][0] for s in dht) == [0x02, 0x03, 0x12, 0x13] and 0xC1 in [s[0] for s in seg["huff_ids_2_3_sof1"]]
    merged = [s[0] for s in seg["struct_merged_dht_dqt"]]
    assert merged.count(0xC4) == 1 and merged.count(0xDB) == 1
    assert [s[0] for s in seg["samp_420_37x27"]].count(0xC4) == 4
    assert [s[1][0] >> 4 for s in seg["struct_dqt_16bit"] if s[0] == 0xDB] == [1, 0]
    assert max(q.max() for q in _q("struct_dqt_16bit").values()) > 255
    assert all(s[2] == 3 for s in seg["struct_fill_bytes"][1:]) and JC.case("struct_fill_bytes").data.endswith(b"\xff" * 4 + b"\xd9")
    assert not any(s[0] == 0xE0 for s in seg["struct_ids_7_9_200_no_jfif"])
    nested = [s for s in seg["struct_com_app1_with_soi_eoi"] if s[0] in (0xFE, 0xE1)]
    assert len(nested) == 3 and all(b"\xff\xd8" in s[1] and b"\xff\xd9" in s[1] and b"\xff\xda" in s[1] for s in nested)
    assert _rst("struct_dri_1") == [0xD0, 0xD1, 0xD2]                                   # 2 x 2 MCUs, one per interval
    r = _rst("struct_dri_11_intervals")
    assert r == [0xD0 + k % 8 for k in range(11)] and r[7:9] == [0xD7, 0xD0]            # 12 intervals, RST7 -> RST0
    assert _rst("struct_dri_beyond_mcu_count") == [] and JC.case("struct_dri_beyond_mcu_count").meta["restart"] == 1000
    assert len(_rst("struct_long_codes_dri_3")) == 1


SAMPLING = {   # name -> (width, height, (h, v) per component), written out independently of the builder
    "samp_444_19x13": (19, 13, JC.S444), "samp_422_35x21": (35, 21, JC.S422), "samp_420_37x27": (37, 27, JC.S420),
    "samp_cb11_cr22_29x19": (29, 19, ((2, 2), (1, 1), (2, 2))), "samp_cb11_cr21_27x11": (27, 11, ((2, 1), (1, 1), (2, 1))),
    "samp_420_w5_h9": (5, 9, JC.S420), "samp_420_w6_h2": (6, 2, JC.S420), "samp_422_w5_h17": (5, 17, JC.S422),
    "samp_422_w6_h1": (6, 1, JC.S422), "samp_420_w21_h1": (21, 1, JC.S420), "samp_420_w40_h17": (40, 17, JC.S420),
    "samp_444_w1_h9": (1, 9, JC.S444), "samp_444_w9_h2": (9, 2, JC.S444), "samp_420_64x64": (64, 64, JC.S420),
    "samp_420_64x64_b": (64, 64, JC.S420), "samp_420_64x64_c": (64, 64, JC.S420), "samp_420_64x64_d": (64, 64, JC.S420),
    "samp_grey_24x16_a": (24, 16, ((1, 1),)), "samp_grey_24x16_b": (24, 16, ((1, 1),)),
    "samp_grey_24x16_dri": (24, 16, ((1, 1),)), "samp_grey_13x17": (13, 17, ((1, 1),)), "samp_grey_8x8": (8, 8, ((1, 1),)),
}


def test_sampling_cases():
    assert {c.name for c in ACCEPTED if c.name.startswith("samp_")} == set(SAMPLING)
    for name, (w, h, hv) in SAMPLING.items():
        info = J.parse(JC.case(name).data)
        assert (info["width"], info["height"]) == (w, h) and tuple((c["h"], c["v"]) for c in info["comps"]) == hv
        assert JC.expected(JC.case(name)).shape == (h, w, 3)
    narrowest = [n for n, (w, h, hv) in SAMPLING.items() if hv[0][0] == 2 and -(-w // 2) == 3]
    assert {SAMPLING[n][2] for n in narrowest} == {JC.S420, JC.S422} and {SAMPLING[n][0] for n in narrowest} == {5, 6}
    assert {1, 2, 9, 17} <= {h for _, h, _ in SAMPLING.values()} and SAMPLING["samp_444_w1_h9"][0] == 1
    for key, size in (("b420", 6), ("bgrey", 3), ("b64", 4)):          # what one batched call needs of its members
        b = JC.batch(key)
        assert len(b) == size and len({(c.meta["width"], c.meta["height"], str(c.meta["hv"])) for c in b}) == 1
    b = JC.batch("b420")
    assert len({str(J.parse(c.data)["ht"]) for c in b}) >= 2 and len({c.meta["restart"] for c in b}) >= 3
    assert len({str(c.meta["ids"]) for c in b}) >= 3 and len({str(_q(c.name)) for c in b}) >= 3
    assert sum(any(s[0] == 0xDB and s[1][0] >> 4 for s in JC.segments(c.data)) for c in b) == 1


# ---------------------------------------------------------------------------------------------------------
_COEF = {}                     # case name -> entropy-decoded coefficients, shared by the mutations


@pytest.mark.parametrize("mutation", list(JC.MUTATIONS))
def test_every_mutation_changes_some_expectation(mutation):
    mod = JC.mutated_oracle(mutation)
    hit = []
    for c in ACCEPTED:
        info = J.parse(c.data)
        mod.parse = lambda data, info=info: info                       # entropy decoding is not what is mutated
        coef = _COEF.setdefault(c.name, J.coefficients(info))
        mod.coefficients = lambda info, coef=coef: coef
        if not np.array_equal(mod.decode(c.data), JC.expected(c)):
            hit.append(c.name)
    assert hit, f"no case notices: {mutation}"


def test_unmutated_copy_is_the_oracle():
    mod = JC.mutated_oracle(None)
    for c in ACCEPTED[:8]:
        assert np.array_equal(mod.decode(c.data), JC.expected(c))


# ---------------------------------------------------------------------------------------------------------
def _probe(data):
    lib = N.lib()
    w, h, c = C.c_int(-1), C.c_int(-1), C.c_int(-1)
    rc = lib.vcap_jpeg_probe(data, len(data), C.byref(w), C.byref(h), C.byref(c))
    return int(rc), (w.value, h.value, c.value), lib.vcap_last_error().decode()


@pytest.mark.parametrize("case", ACCEPTED, ids=_ids(ACCEPTED))
def test_probe_accepts(case):
    info = J.parse(case.data)
    assert _probe(case.data)[:2] == (0, (info["width"], info["height"], len(info["comps"])))
    assert N.lib().vcap_jpeg_workspace_bytes(case.data, len(case.data), 1) > 0
    assert N.lib().vcap_jpeg_workspace_bytes(case.data, len(case.data), 33) > N.lib().vcap_jpeg_workspace_bytes(
        case.data, len(case.data), 1)


@pytest.mark.parametrize("case", REFUSED, ids=_ids(REFUSED))
def test_probe_refuses_with_the_listed_code(case):
    assert _probe(case.data)[0] == CODES[case.refuse]
    assert N.lib().vcap_jpeg_workspace_bytes(case.data, len(case.data), 1) == 0


@pytest.mark.parametrize("name, data, code, text", JC.DAMAGED, ids=[d[0] for d in JC.DAMAGED])
def test_damaged_header_is_refused(name, data, code, text):
    rc, _, err = _probe(data)
    assert (rc, err) == (CODES[code], "vcap_jpeg_probe: " + text)
    assert N.lib().vcap_jpeg_workspace_bytes(data, len(data), 1) == 0
