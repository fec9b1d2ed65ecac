"""Frames of up to 16384 samples (bigblock_cases.py) through everything that runs on the CPU, and
the decoder's geometry (fg_geom.hpp: dec_geometry; fg_dec.hpp: seg_len) on the host under
AddressSanitizer and UBSan.  No GPU.  tests/test_gpu_bigblock.py gives the GPU only these frames.

(a) the verifier decoder returns the generator's PCM: the inputs are good.
(b) the unchanged tests/cpp/decode_host_main.cpp with block = 16384, sizes given and found.
(c) tests/cpp/decgeom_host_main.cpp against tests/golden/dec_geometry.json.  The rows of blocks
    <= 4096 are what launch_dec_recon computed before dec_geometry existed, worked out by hand:
    a plane is 4096 + 4096 / 64 = 4160 elements.  8 / 16 / 24 bits: 4-byte elements, W = C waves,
    C * 4160 * 4 = C * 16640 bytes of LDS (8 channels: 133120), one pass.  32 bits: 8-byte elements,
    W = min(C, 4), W * 4160 * 8 = W * 33280 bytes (4 and more channels: 133120), two passes where
    C > 4.  Above 4096 the plane is B + B / 64 elements, B = 8192 or 16384, and W = min(C, floor(
    (163840 - 16) / plane bytes)): 33280 -> 4, 66560 -> 2, 133120 -> 1; a 32-bit context above 8192
    is refused.
(d) the DecSub bytes of every frame of frame_grammar.cases() (all <= 4096 samples) hash to
    tests/golden/decsub_sha.json, recorded with the same program against fg_dec.hpp as it was before
    segments scaled: no existing frame decodes differently.  The program writes the bytes, this
    module hashes them.
(e) the argument checks of flacgpu_open_decoder that come before any device call."""
import ctypes
import hashlib
import json
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "zig-flac_amd"))
sys.path.insert(0, os.path.join(HERE, "golden"))

import bigblock_cases as bb  # noqa: E402
import decode_cases as dc  # noqa: E402
import frame_grammar as fg  # noqa: E402
import test_decode_host as tdh  # noqa: E402

CASES = bb.cases()
IDS = [c["name"] for c in CASES]
GEOM_BLOCKS = (1, 4096, 4097, 8192, 8193, 16384, 16385)
GEOM_ARGS = [f"{ch},{bits},{blk}" for ch in range(1, 9) for bits in (8, 16, 24, 32) for blk in GEOM_BLOCKS]
SEG_BLOCKS = (1, 64, 4095, 4096, 4097, 4608, 8192, 8193, 16383, 16384)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return tdh.host_program(tmp_path_factory.mktemp("bigblock_dec"))


@pytest.fixture(scope="module")
def geom_exe(tmp_path_factory):
    path = os.path.join(str(tmp_path_factory.mktemp("decgeom")), "decgeom_host_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-Wno-unknown-pragmas",
                           os.path.join(HERE, "cpp", "decgeom_host_main.cpp"), "-o", path])
    return path


def run(exe, args):
    r = subprocess.run([exe, *args], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", f"sanitizer / program failure for {args[:3]}:\n{r.stderr[-2000:]}"
    return json.loads(r.stdout)


def _golden(name):
    with open(os.path.join(HERE, "golden", name)) as f:
        return json.load(f)


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_verifier_decoder_returns_the_generators_samples(c):
    """(a) every frame alone, first_number its own coded number (variable blocking codes samples)."""
    for f in c["frames"]:
        assert dc.oracle_status(f["frame"], c["channels"], c["bits"], c["rate"], f["number"]) == 0, f["block"]
        assert dc.oracle_pcm(f["frame"], c["channels"], c["bits"], c["rate"], f["number"]) == f["pcm"], f["block"]


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_host_program_under_sanitizers(exe, tmp_path, c):
    """(b) the program takes block = 16384 once fg::dec::kMaxBlock does."""
    frames = [f["frame"] for f in c["frames"]]
    for sizes in (True, False):
        res, got = tdh.run_host(exe, tmp_path, frames, c["channels"], c["bits"], c["rate"], block=16384, sizes=sizes)
        assert res["status"] == [0] * len(frames), sizes
        assert res["block"] == [f["block"] for f in c["frames"]], sizes
        assert res["number"] == [f["number"] for f in c["frames"]], sizes
        assert res["consumed"] == [len(x) for x in frames], sizes
        assert got == fg.case_pcm(c), sizes


def test_host_program_block_limits(exe, tmp_path):
    """A frame larger than the block argument is RANGE, and 16385 is no block argument."""
    c = bb.case("big_mono_a")
    f = c["frames"][1]  # 4608 samples
    res, got = tdh.run_host(exe, tmp_path, [f["frame"]], 1, 16, c["rate"], block=4096)
    assert res["status"] == [dc.STATUS["RANGE"]] and got == b""
    res, got = tdh.run_host(exe, tmp_path, [f["frame"]], 1, 16, c["rate"], block=4608)
    assert res["status"] == [0] and got == f["pcm"]
    r = subprocess.run([exe, "none", "1", "16", "44100", "16385", "none"], capture_output=True, text=True)
    assert r.returncode == 2


def test_geometry_matches_the_fixture(geom_exe):
    """(c)"""
    gold = _golden("dec_geometry.json")
    assert [r["args"] for r in gold["rows"]] == GEOM_ARGS
    got = run(geom_exe, ["geom", *GEOM_ARGS])
    for g, want in zip(got, gold["rows"]):
        assert g == want["out"], want["args"]
    assert run(geom_exe, ["seglen", *map(str, SEG_BLOCKS)]) == [gold["seg_len"][str(b)] for b in SEG_BLOCKS]
    # refused without a table: channel counts and depths no context has
    assert run(geom_exe, ["geom", "0,16,4096", "9,16,4096", "2,12,4096", "2,16,0"]) == [{"ok": 0}] * 4


def test_geometry_invariants(geom_exe):
    """Independent of the fixture: what a launch needs to be legal, and what the kernel assumes."""
    for arg, g in zip(GEOM_ARGS, run(geom_exe, ["geom", *GEOM_ARGS])):
        ch, bits, blk = map(int, arg.split(","))
        if not g["ok"]:
            assert blk > (8192 if bits == 32 else 16384), arg
            continue
        assert g["elem"] == (8 if bits == 32 else 4)
        assert g["lds"] == g["W"] * g["plane_words"] * g["elem"] and g["lds"] + 16 <= 160 * 1024, arg
        assert 1 <= g["W"] <= ch and g["W"] >= min(ch, 2), arg  # both planes of a stereo pair in one round
        assert g["passes"] == (2 if ch > g["W"] else 1), arg
        # the padded index of the last sample of the largest frame stays inside the plane
        top = 4096 if blk <= 4096 else 8192 if blk <= 8192 else 16384
        seg = top // 64
        assert (top - 1) + (top - 1) // seg < g["plane_words"] == top + top // 64, arg


def decsub_hashes(geom_exe, work, case):
    """sha256 of each frame's DecSub bytes (340 per subframe) as parse_frame leaves them."""
    frames = [f["frame"] for f in case["frames"]]
    blob, sz, out = (os.path.join(str(work), n) for n in ("frames.bin", "sizes.txt", "subs.bin"))
    with open(blob, "wb") as f:
        f.write(b"".join(frames))
    with open(sz, "w") as f:
        f.write("\n".join(str(len(x)) for x in frames))
    res = run(geom_exe, ["decsub", blob, sz, str(case["channels"]), str(case["bits"]), str(case["rate"]), out])
    assert res["status"] == [0] * len(frames) and res["nsub"] == [case["channels"]] * len(frames)
    raw = open(out, "rb").read()
    per = 340 * case["channels"]
    assert len(raw) == per * len(frames)
    return [hashlib.sha256(raw[i * per:(i + 1) * per]).hexdigest() for i in range(len(frames))]


def test_descriptors_up_to_4096_are_unchanged(geom_exe, tmp_path):
    """(d)"""
    gold = _golden("decsub_sha.json")
    small = fg.cases()
    assert sorted(gold) == sorted(c["name"] for c in small)
    for c in small:
        assert decsub_hashes(geom_exe, tmp_path, c) == gold[c["name"]], c["name"]


def test_descriptors_of_big_frames_use_longer_segments(geom_exe, tmp_path):
    """seg_pos of a big frame's FIXED subframe: segment s starts at sample max(L s, order), so with
    every residual of one escaped width w the positions are L * w bits apart."""
    import flac_bits as fbits

    bs, w, order = 8192, 5, 2
    x = [((i * 7) % 13) - 6 for i in range(bs)]
    res = fbits.fixed_residual(x, order)
    assert all(-16 <= r < 16 for r in res)
    fr = fbits.frame(0, bs, 0, 16, lambda wr: fbits.sub_fixed(wr, x, 16, order, 0, 0, [("esc", w)]))
    case = {"channels": 1, "bits": 16, "rate": 44100, "frames": [{"frame": fr}]}
    decsub_hashes(geom_exe, tmp_path, case)
    raw = open(os.path.join(str(tmp_path), "subs.bin"), "rb").read()
    seg_pos = [int.from_bytes(raw[12 + 4 * s:16 + 4 * s], "little") for s in range(64)]
    assert seg_pos[1] - seg_pos[0] == 4 + 5 + (128 - order) * w  # the parameter field, then 126 residuals
    assert [b - a for a, b in zip(seg_pos[1:], seg_pos[2:])] == [128 * w] * 62


def test_open_decoder_argument_checks():
    """(e)"""
    import flacgpu

    L = flacgpu.load_library()
    assert "flacgpu_open_decoder" in flacgpu.exported_symbols()
    assert "flacgpu_open_decoder" in open(os.path.join(ROOT, "include", "flacgpu.h")).read()
    assert L.flacgpu_abi_version() == 5
    h = ctypes.c_void_p()
    out = ctypes.byref(h)
    assert L.flacgpu_open_decoder(0, 44100, 2, 16, 16384, 4, None) == -2
    for rate, ch, bits, block in ((44100, 2, 16, 0), (44100, 2, 16, 16385), (44100, 2, 32, 8193), (44100, 1, 32, 16384),
                                  (44100, 0, 16, 8192), (44100, 9, 16, 8192), (44100, 2, 12, 8192), (44100, 2, 0, 8192),
                                  (1 << 20, 2, 16, 8192)):
        assert L.flacgpu_open_decoder(0, rate, ch, bits, block, 4, out) == -1, (rate, ch, bits, block)
        assert not h.value
    try:
        import torch
        has_gpu = torch.cuda.is_available()
    except ImportError:
        has_gpu = False
    if not has_gpu:  # good arguments reach the device check; there is no other path
        assert L.flacgpu_open_decoder(0, 44100, 2, 16, 16384, 4, out) == -5
        assert L.flacgpu_open_decoder(0, 44100, 2, 32, 8192, 4, out) == -5
        with pytest.raises(flacgpu.FlacGpuError) as e:
            flacgpu.Decoder(2, 16, 44100, block_size=16384)
        assert e.value.code == -5
