"""The decoder's shared core (zig-flac_amd/csrc/fg_dec.hpp) on the host, under AddressSanitizer
and UBSan, through the stand-alone program tests/cpp/decode_host_main.cpp; the host-only frame
index; and the decode entry points' argument checks.  No GPU.

The sanitizer run is what clears corrupted input for the device: tests/test_gpu_decode.py gives
the GPU only frames that went through here (host_statuses below)."""
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

import decode_cases as dc  # noqa: E402
import make_golden  # noqa: E402
import oracle_ref  # noqa: E402

_PROG = {}


def host_program(tmp_dir) -> str:
    """decode_host_main built with -fsanitize=address,undefined (once per test process)."""
    if "path" not in _PROG:
        exe = os.path.join(str(tmp_dir), "decode_host_main")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=undefined", "-Wno-unknown-pragmas",
                               os.path.join(HERE, "cpp", "decode_host_main.cpp"), "-o", exe])
        _PROG["path"] = exe
    return _PROG["path"]


def run_host(exe, work, frames, channels, bits, rate, block=4096, sizes=True):
    """Frames (a list of bytes) through the program -> (result dict, pcm bytes).  A sanitizer
    report makes the program exit non-zero with text on stderr: both are asserted absent."""
    blob = os.path.join(str(work), "frames.bin")
    with open(blob, "wb") as f:
        f.write(b"".join(frames))
    args = [exe, blob, str(channels), str(bits), str(rate), str(block), os.path.join(str(work), "out.pcm")]
    if sizes:
        sz = os.path.join(str(work), "sizes.txt")
        with open(sz, "w") as f:
            f.write("\n".join(str(len(x)) for x in frames))
        args.append(sz)
    r = subprocess.run(args, capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", f"sanitizer / program failure:\n{r.stderr[-2000:]}"
    return json.loads(r.stdout), open(os.path.join(str(work), "out.pcm"), "rb").read()


def host_statuses(exe, work, c, frames, corrupted):
    """Statuses of corrupted frames (a list of bytes) of golden / hand-built case c."""
    res, _ = run_host(exe, work, corrupted, c["channels"], c["bits"], c.get("rate", 44100), c.get("block", 4096))
    return res["status"]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return host_program(tmp_path_factory.mktemp("dechost"))


@pytest.mark.parametrize("c", dc.FRAME_CASES, ids=[c["name"] for c in dc.FRAME_CASES])
def test_goldens_decode_clean(exe, tmp_path, c):
    frames, raw = dc.golden_frames(c)
    pcm = make_golden.make_pcm(c["name"], c["channels"], c["bits"], c["rate"], c["n_samples"], c["stream_seed"])
    assert hashlib.sha256(pcm).hexdigest() == c["pcm_sha256"]
    ref, ref_sizes = oracle_ref.decode_frames(raw, c["channels"], c["bits"], c["rate"], c["n_samples"],
                                              first_number=c["first_frame"])
    assert ref == pcm
    # the frames taken one after another, each as long as it parses: the sizes are found, not given
    res, got = run_host(exe, tmp_path, [raw], c["channels"], c["bits"], c["rate"], c["block"], sizes=False)
    assert res["status"] == [0] * len(frames)
    assert res["consumed"] == c["frame_bytes"] == ref_sizes
    assert res["number"] == [c["first_frame"] + i for i in range(len(frames))]
    assert got == ref
    # and each within its own length
    res, got = run_host(exe, tmp_path, frames, c["channels"], c["bits"], c["rate"], c["block"])
    assert res["status"] == [0] * len(frames) and got == ref


def test_hand_built_frames_decode(exe, tmp_path):
    for h in dc.hand_built():
        res, got = run_host(exe, tmp_path, [h["frame"]], h["channels"], h["bits"], 44100)
        assert res["status"] == [0] and res["block"] == [h["block"]] and res["number"] == [h["number"]], h["name"]
        assert got == h["pcm"], h["name"]  # the samples the frame was written from
        assert got == dc.oracle_pcm(h["frame"], h["channels"], h["bits"], 44100, h["number"]), h["name"]


@pytest.mark.parametrize("c", dc.FRAME_CASES, ids=[c["name"] for c in dc.FRAME_CASES])
def test_corrupted_frames_are_caught(exe, tmp_path, c):
    frames, _ = dc.golden_frames(c)
    bad = []
    for f, fr in enumerate(frames):
        bad += [dc.flip(fr, b) for b in dc.edge_flips(fr)]
        bad += dc.cuts(fr)
    bad += [dc.flip(frames[f], b) for f, b in dc.random_flips(c, frames)]
    # untouched frames between the corrupted ones
    batch = []
    for i, x in enumerate(bad):
        batch.append(x)
        if i % 50 == 0:
            batch.append(frames[i % len(frames)])
    res, _ = run_host(exe, tmp_path, batch, c["channels"], c["bits"], c["rate"], c["block"])
    k = 0
    for i, x in enumerate(bad):
        assert res["status"][k] != 0, f"corrupted frame {i} of {c['name']} decoded as good"
        k += 1
        if i % 50 == 0:
            assert res["status"][k] == 0
            k += 1
    assert k == len(batch)


def test_curated_corruptions_give_the_oracle_codes(exe, tmp_path):
    b = dc.curated_base()
    cur = dc.curated(b["frame"], b["marks"])
    res, _ = run_host(exe, tmp_path, [fr for _, fr, _ in cur], b["channels"], b["bits"], 44100)
    for (name, fr, want), got in zip(cur, res["status"]):
        assert dc.oracle_status(fr, b["channels"], b["bits"], 44100, b["number"]) == dc.STATUS[want], name
        assert got == dc.STATUS[want], (name, got)
    # the same places in every golden's first frame, against the verifier decoder's own verdict
    for c in dc.FRAME_CASES:
        frames, _ = dc.golden_frames(c)
        fr = frames[0]
        n = len(fr)
        cases = [dc.flip(fr, 3), dc.flip(fr, 31), dc.flip(fr, 39), dc.flip(fr, 8 * (n - 1) + 2), dc.flip(fr, 8 * (n // 2))]
        res, _ = run_host(exe, tmp_path, cases, c["channels"], c["bits"], c["rate"], c["block"])
        want = [dc.oracle_status(x, c["channels"], c["bits"], c["rate"], c["first_frame"]) for x in cases]
        assert res["status"] == want, c["name"]


def test_flac_index():
    import flacgpu

    for c in dc.FRAME_CASES:
        _, raw = dc.golden_frames(c)
        si, first, sizes = flacgpu.flac_index(raw, raw_frames=True)
        assert si is None and first == 0 and sizes == c["frame_bytes"], c["name"]
    c = dc.FILE_CASE
    buf = open(os.path.join(dc.GOLD, c["name"] + ".flac"), "rb").read()
    si, first, sizes = flacgpu.flac_index(buf)
    assert first == 73 and sum(sizes) == len(buf) - 73
    body = buf[8:42]  # "fLaC", the block header, then the 34 STREAMINFO bytes
    assert (si.min_block_size, si.max_block_size) == (int.from_bytes(body[0:2], "big"), int.from_bytes(body[2:4], "big"))
    assert (si.min_frame_size, si.max_frame_size) == (int.from_bytes(body[4:7], "big"), int.from_bytes(body[7:10], "big"))
    v = int.from_bytes(body[10:18], "big")
    assert si.sample_rate == v >> 44 == c["rate"]
    assert si.channels == ((v >> 41) & 7) + 1 == c["channels"]
    assert si.bit_depth == ((v >> 36) & 31) + 1 == c["bits"]
    assert si.interchannel_samples == v & ((1 << 36) - 1) == c["n_samples"]
    assert bytes(si.md5) == body[18:34] and bytes(si.md5).hex() == c["md5"]
    assert max(sizes) == si.max_frame_size
    # a truncated file, and bytes that are no FLAC, are refused
    for bad in (buf[:-5], b"RIFF" + buf[4:], buf[:60]):
        with pytest.raises(flacgpu.FlacGpuError) as e:
            flacgpu.flac_index(bad)
        assert e.value.code == -2


def test_argument_checks_without_a_device():
    import flacgpu

    L = flacgpu.load_library()
    n = ctypes.c_size_t(0)
    ns = ctypes.c_uint64(0)
    buf = ctypes.create_string_buffer(64)
    assert L.flacgpu_flac_index(None, 0, None, None, None, 0, ctypes.byref(n)) == -2
    assert L.flacgpu_flac_index(buf, 64, None, None, None, 0, None) == -2
    assert L.flacgpu_decode_frames(None, buf, buf, 1, buf, 64, ctypes.byref(ns), buf) == -2
    assert L.flacgpu_decode_frames_device(None, buf, buf, buf, 1, None, None, 0, None, buf, buf, None) == -2
    assert L.flacgpu_verify_plan_device(None, None, buf, buf, buf, buf, buf, buf, None) == -2
    assert L.flacgpu_decode_file(None, buf, 64, buf, 64, ctypes.byref(ns), None) == -2
    try:
        import torch
        has_gpu = torch.cuda.is_available()
    except ImportError:
        has_gpu = False
    if has_gpu:
        # with a context: NULL buffers, and more frames than the context was opened for
        with flacgpu.Decoder(2, 16, 44100, max_frames=4) as d:
            assert L.flacgpu_decode_frames_device(d.ctx, None, buf, buf, 1, None, None, 0, None, buf, buf, None) == -2
            assert L.flacgpu_decode_frames_device(d.ctx, buf, buf, buf, 5, None, None, 0, None, buf, buf, None) == -2
            assert L.flacgpu_decode_frames(d.ctx, buf, buf, 1, buf, 64, None, buf) == -2
    else:
        with pytest.raises(flacgpu.FlacGpuError) as e:
            flacgpu.Decoder(2, 16, 44100)
        assert e.value.code == -5
