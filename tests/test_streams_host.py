"""The many-streams forms of the device index and decode on the host, under AddressSanitizer and
UBSan, through the stand-alone program tests/cpp/streams_host_main.cpp.  No GPU.

`index`: the per-stream geometry, carving and dispatch of fg_index.hpp, the scalar pieces applied
stream by stream over one concatenated buffer with odd offsets, against flacgpu_flac_index per
stream.  `segments`: the cut of all streams' frames into chunks and the per-frame PCM offsets and
folded results of fg_streams.hpp, which the program checks against plain loops; the cut itself is
checked again here."""
import json
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "zig-flac_amd"))

import index_cases as ic  # noqa: E402


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = os.path.join(str(tmp_path_factory.mktemp("streamshost")), "streams_host_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-Wno-unknown-pragmas",
                           os.path.join(HERE, "cpp", "streams_host_main.cpp"), "-o", out])
    return out


def run(exe, args):
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", f"sanitizer / program failure:\n{r.stdout[-500:]}\n{r.stderr[-2000:]}"
    return json.loads(r.stdout)


def layout(streams, gap=3):
    """The streams back to back at odd offsets in a 0xA5-filled blob -> (blob, [offset])."""
    blob, offs = bytearray(b"\xA5" * 5), []
    for data in streams:
        if len(blob) % 2 == 0:
            blob += b"\xA5"
        offs.append(len(blob))
        blob += data + b"\xA5" * gap
    return bytes(blob), offs


def index_streams():
    by = {c[0]: c for c in ic.cases()}
    names = ["c1_44k16_stereo" if "c1_44k16_stereo" in by else ic.cases()[0][0], "len_0", "tiny_frames", "cut_1",
             "hand_built", "near_candidate", "no_sync", "lone_fake_header"]
    return [by[n] for n in names]


def test_index_streams_match_the_host_index(exe, tmp_path):
    cases = index_streams()
    blob, offs = layout([c[1] for c in cases])
    assert all(o % 2 == 1 for o in offs)
    path = os.path.join(str(tmp_path), "blob.bin")
    with open(path, "wb") as f:
        f.write(blob)
    want = [ic.host_index(c[1]) for c in cases]
    assert any(w is None for w in want) and any(w == [] for w in want)
    assert max(len(c[1]) for c in cases) > 2 * 16384  # more than two groups
    caps = [len(c[1]) // 8 + 1 for c in cases]
    short = next(i for i, c in enumerate(cases) if c[0] == "hand_built")
    for too_small in (False, True):
        if too_small:
            caps[short] = len(want[short]) - 1
        args = ["index", path, len(cases)]
        for (name, data, bits, rate), off, cap in zip(cases, offs, caps):
            args += [off, len(data), bits, rate, cap]
        res = run(exe, args)
        assert res["untouched"]
        for i, (c, w, off, got) in enumerate(zip(cases, want, offs, res["streams"])):
            if w is None:
                assert (got["status"], got["n_frames"], got["sizes"]) == (1, 0, []), c[0]
            elif too_small and i == short:
                assert (got["status"], got["n_frames"], got["sizes"]) == (2, len(w), []), c[0]
            else:
                assert (got["status"], got["n_frames"]) == (0, len(w)) and got["sizes"] == w, c[0]
                at, expect = off, []
                for s in w:
                    expect.append(at)
                    at += s
                assert got["offsets"] == expect, c[0]


def plain_cut(frames, max_frames):
    segs, fill, chunk = [], 0, 0
    for s, n in enumerate(frames):
        done = 0
        while done < n:
            if fill == max_frames:
                fill, chunk = 0, chunk + 1
            k = min(n - done, max_frames - fill)
            segs.append([s, fill, k, done, chunk * max_frames + fill])
            fill += k
            done += k
    return segs


@pytest.mark.parametrize("frames", [
    [1, 3, 64, 70, 0],          # cuts inside a stream and exactly at a boundary, a chunk of three streams
    [10, 150, 0, 0, 7, 64, 1],  # starts mid-chunk, spans three chunks, ends mid-chunk; streams of 0 frames
    [0, 0], [64], [64, 64], [129],
])
def test_segments(exe, frames):
    for seed, short in ((1, None), (2, 1)):
        args = ["segments", 64, 4, seed]
        for n in frames:
            args += [n, n if short is None else max(n - short, 0)]
        res = run(exe, args)
        want = plain_cut(frames, 64)
        assert res["segments"] == want
        firsts = [i for i, s in enumerate(want) if s[1] == 0]
        assert res["chunks"] == (firsts + [len(want)] if want else [])
    if frames == [10, 150, 0, 0, 7, 64, 1]:
        of_1 = [s for s in plain_cut(frames, 64) if s[0] == 1]
        assert len(of_1) == 3 and of_1[0][1] == 10 and of_1[-1][1] + of_1[-1][2] < 64
