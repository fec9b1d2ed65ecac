"""Frames of the seeded grammar (frame_grammar.py) through everything that decodes on the CPU.  No
GPU.  The expected PCM of every frame is the generator's own samples, known before any decoder
ran, so a reading of RFC 9639 that the verifier decoder and fg_dec.hpp share does not pass here.

Per case: (a) the verifier decoder (oracle/flac_decode.c), (b) the decode core on the host under
AddressSanitizer and UBSan (tests/cpp/decode_host_main.cpp) with the frame sizes given and with
the sizes found, (c) the host frame index and the index's shared pieces under the sanitizers
(tests/cpp/index_host_main.cpp).  tests/test_gpu_frame_grammar.py gives the GPU only these
frames, all valid, after they went through here.

Also pinned here: flac_bits.frame()'s new optional arguments left the older hand-built frames
and index streams byte for byte as they were."""
import hashlib
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "zig-flac_amd"))
sys.path.insert(0, os.path.join(HERE, "golden"))

import decode_cases as dc  # noqa: E402
import flac_bits as fb  # noqa: E402
import frame_grammar as fg  # noqa: E402
import index_cases as ic  # noqa: E402
import test_decode_host as tdh  # noqa: E402
import test_index_host as tih  # noqa: E402

CASES = fg.cases()
IDS = [c["name"] for c in CASES]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return tdh.host_program(tmp_path_factory.mktemp("grammar_dec"))


@pytest.fixture(scope="module")
def index_exe(tmp_path_factory):
    return tih.host_program(tmp_path_factory.mktemp("grammar_idx"))


def test_older_hand_built_bytes_are_unchanged():
    """sha256 taken before flac_bits.frame() grew its optional arguments."""
    h = hashlib.sha256()
    for x in dc.hand_built():
        h.update(x["name"].encode())
        h.update(x["frame"])
    assert h.hexdigest() == "78e287428e6b40c8c85c6a0f63bfa708ad668649eec1a0594166aa7b78222954"
    pins = {
        "tiny_frames": (b"".join(ic.tiny_frames()), "332b5dd55f7bf5e148d949f5f3496f2728d5b540e38a9f45d37238d388dbf297"),
        "lone_fake_header": (ic.lone_fake_header(), "704a6db8b512ed991cb2b54d2b7f886eb6a0a61baf42b010b620812715e695bc"),
        "nested_fake_frames": (ic.nested_fake_frames(), "90be28477c2174021cca8996bc012f7169dbe3257933e66df6bb7a2c622ae8b8"),
        "false_end": (ic.false_end()[0], "831757cdf750dfac4220b12e15404c15566e7a05dbe5ff436f0ea39d10cecf16"),
        "near_candidate": (ic.near_candidate()[0], "46b1ff3f6ea810fad7b3952afc2ef67b1e769900f74b168a757f370508e47cf0"),
    }
    for name, (data, want) in pins.items():
        assert hashlib.sha256(data).hexdigest() == want, name


def test_the_grammar_is_what_it_claims():
    cov = fg.coverage(CASES)
    assert [k for k, v in cov.items() if v == 0] == []
    assert 36 <= len(CASES) <= 48 and all(3 <= len(c["frames"]) <= 6 for c in CASES)
    assert sum(f["block"] >= 4095 for c in CASES for f in c["frames"]) <= 6  # the bit-list writer is slow on those
    for c in CASES:
        per = c["channels"] * (c["bits"] // 8)
        for f in c["frames"]:
            assert fb.crc16(f["frame"]) == 0
            assert len(f["pcm"]) == f["block"] * per
    # the same list twice gives the same bytes: nothing depends on anything but the seeds
    again = fg._build_case(fg._SPECS[5])
    assert fg.case_bytes(again) == fg.case_bytes(CASES[5]) and fg.case_pcm(again) == fg.case_pcm(CASES[5])


def test_the_header_arguments_write_rfc_9639_headers():
    """flac_bits.frame()'s optional arguments against header bytes worked out by hand from 9.1."""
    sub = lambda w: fb.sub_constant(w, 0, 16)  # noqa: E731
    # 4096 samples by table code 12, rate code 0, depth code 0, fixed strategy, frame 1
    fr = fb.frame(1, 4096, 0, 16, sub, table_bs=True, rate_code=0, bits_code=0)
    assert fr[:5] == bytes([0xFF, 0xF8, 0xC0, 0x00, 0x01]) and fr[5] == fb.crc8(fr[:5])
    # 192 samples (code 1), 8-bit kHz field (code 12) = 48, variable strategy, sample number 2^35:
    # the field follows the 7-byte coded number; no block-size field
    fr = fb.frame(1 << 35, 192, 1, 16, lambda w: (sub(w), sub(w)), table_bs=True, rate_code=12, rate_field=48, variable=True)
    assert fr[:4] == bytes([0xFF, 0xF9, 0x1C, 0x18])
    assert fr[4:11] == bytes([0xFE, 0xA0, 0x80, 0x80, 0x80, 0x80, 0x80]) and fr[11] == 48 and fr[12] == fb.crc8(fr[:12])
    # 100 samples (code 6, field 99), then the 16-bit rate field of code 14
    fr = fb.frame(0, 100, 0, 16, sub, table_bs=True, rate_code=14, rate_field=4410)
    assert fr[:4] == bytes([0xFF, 0xF8, 0x6E, 0x08]) and fr[4:8] == bytes([0, 99, 0x11, 0x3A]) and fr[8] == fb.crc8(fr[:8])
    assert [fb.block_size_code(b) for b in (192, 576, 1152, 2304, 4608, 256, 512, 4096, 32768, 100, 257)] == \
        [1, 2, 3, 4, 5, 8, 9, 12, 15, 6, 7]


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_verifier_decoder_returns_the_generators_samples(c):
    """(a) fdec_frames_to_pcm insists on consecutive frame numbers from first_number, which the
    variable-blocksize cases (the coded number is a sample number) do not have: every frame of
    every case is decoded alone with first_number set to its own coded number.  The verifier
    ignores the blocking-strategy bit, so this accepts those frames as they are."""
    for f in c["frames"]:
        assert dc.oracle_status(f["frame"], c["channels"], c["bits"], c["rate"], f["number"]) == 0, f["block"]
        assert dc.oracle_pcm(f["frame"], c["channels"], c["bits"], c["rate"], f["number"]) == f["pcm"], f["block"]


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_host_program_under_sanitizers(exe, tmp_path, c):
    """(b) sizes given: each frame within its own length; sizes found: one after another."""
    frames = [f["frame"] for f in c["frames"]]
    for sizes in (True, False):
        res, got = tdh.run_host(exe, tmp_path, frames, c["channels"], c["bits"], c["rate"], sizes=sizes)
        assert res["status"] == [0] * len(frames), sizes
        assert res["block"] == [f["block"] for f in c["frames"]], sizes
        assert res["number"] == [f["number"] for f in c["frames"]], sizes
        assert res["consumed"] == [len(x) for x in frames], sizes
        assert got == fg.case_pcm(c), sizes


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_index_finds_the_true_sizes(index_exe, tmp_path, c):
    """(c) the host index, and the device index's scalar pieces at three chunk geometries."""
    import flacgpu

    data = fg.case_bytes(c)
    want = [len(f["frame"]) for f in c["frames"]]
    si, first, sizes = flacgpu.flac_index(data, raw_frames=True)
    assert si is None and first == 0 and sizes == want
    for chunk, group, lead in ((7, 3, 0), (64, 256, 0), (64, 256, 9)):
        assert tih.run_host(index_exe, tmp_path, data, c["bits"], c["rate"], chunk, group, lead) == want, (chunk, group, lead)
