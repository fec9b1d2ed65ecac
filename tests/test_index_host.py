"""The device frame index's shared scalar pieces (zig-flac_amd/csrc/fg_index.hpp) on the host,
under AddressSanitizer and UBSan, through the stand-alone program tests/cpp/index_host_main.cpp,
against the host index flacgpu_flac_index.  No GPU.

The program runs the stages of fg_index.hip serially with the chunk size and the chunks per
"workgroup" given on the command line, so sizes of 1 and 7 bytes put a seam at every position.
The sanitizer run is what clears crafted input for the device: tests/test_gpu_index.py gives the
GPU only the streams of index_cases.cases(), all of which go through here."""
import json
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "zig-flac_amd"))

import index_cases as ic  # noqa: E402

_PROG = {}
GEOMETRY = [(c, g) for c in (1, 7, 64, 256) for g in (1, 3)]


def host_program(tmp_dir) -> str:
    """index_host_main built with -fsanitize=address,undefined (once per test process)."""
    if "path" not in _PROG:
        exe = os.path.join(str(tmp_dir), "index_host_main")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=undefined", "-Wno-unknown-pragmas",
                               os.path.join(HERE, "cpp", "index_host_main.cpp"), "-o", exe])
        _PROG["path"] = exe
    return _PROG["path"]


def run_host(exe, work, data, bits, rate, chunk, group, lead=0):
    """A bare run of frames through the program -> the list of sizes, or None where it refuses.  A
    sanitizer report makes the program exit non-zero with text on stderr: both are asserted absent."""
    blob = os.path.join(str(work), "stream.bin")
    with open(blob, "wb") as f:
        f.write(data)
    r = subprocess.run([exe, blob, str(bits), str(rate), str(chunk), str(group), str(lead)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", f"sanitizer / program failure:\n{r.stderr[-2000:]}"
    res = json.loads(r.stdout)
    assert res["status"] in (0, 1)
    if res["status"]:
        assert res["n_frames"] == 0 and res["sizes"] == []
        return None
    assert res["n_frames"] == len(res["sizes"])
    return res["sizes"]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return host_program(tmp_path_factory.mktemp("idxhost"))


CASES = ic.cases()


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_program_matches_the_host_index(exe, tmp_path, case):
    name, data, bits, rate = case
    want = ic.host_index(data)
    for chunk, group in GEOMETRY:
        assert run_host(exe, tmp_path, data, bits, rate, chunk, group) == want, (name, chunk, group)
    # the device's geometry, with the data starting inside the first chunk (an unaligned base)
    for lead in (9, 63):
        assert run_host(exe, tmp_path, data, bits, rate, 64, 256, lead) == want, (name, lead)


def test_the_crafted_streams_are_what_they_claim():
    """What the host index makes of them: the fake header and the nested frames are skipped, the
    false end is taken (the host cuts the frame there), the near candidate is skipped."""
    by = {c[0]: c for c in CASES}
    assert len(ic.host_index(by["lone_fake_header"][1])) == 3
    assert len(ic.host_index(by["nested_fake_frames"][1])) == 3
    data, cut = ic.false_end()
    sizes = ic.host_index(data)
    assert len(sizes) == 4 and sizes[0] + sizes[1] == cut
    data, hdr = ic.near_candidate()
    sizes = ic.host_index(data)
    assert len(sizes) == 3 and sizes[1] > hdr + 3
    assert len(ic.host_index(by["tiny_frames"][1])) == 3001
    assert ic.host_index(by["huge_frames"][1]) == ic.huge_frames()[1]
    for name in ("cut_1", "cut_2", "cut_5", "trailing_junk", "no_sync", "len_1", "len_5"):
        assert ic.host_index(by[name][1]) is None, name
    assert ic.host_index(by["len_0"][1]) == []


def test_goldens_index_to_their_manifest_sizes(exe, tmp_path):
    import decode_cases as dc

    for c in dc.FRAME_CASES:
        _, raw = dc.golden_frames(c)
        assert run_host(exe, tmp_path, raw, c["bits"], c["rate"], 64, 256) == c["frame_bytes"], c["name"]
