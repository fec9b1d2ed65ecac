"""The scalar rules of the sample-window decode (zig-flac_amd/csrc/fg_window.hpp) on the host, under
AddressSanitizer and UBSan, through the stand-alone program tests/cpp/window_host_main.cpp.  No GPU.

`positions`: the block size read at every frame's offset and the exclusive sums, over streams of
the seeded frame grammar (a different block size in every frame) laid at odd offsets of one blob,
against the block sizes the generator used.  `cover`: windows over a position slice against a
plain linear search, in the program and again here.  `copy`: the unit decomposition of the copy
against memcpy for every alignment pair and the lengths 0 to 48."""
import json
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import frame_grammar as fg  # noqa: E402

U64 = (1 << 64) - 1


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = os.path.join(str(tmp_path_factory.mktemp("windowhost")), "window_host_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-Wno-unknown-pragmas",
                           os.path.join(HERE, "cpp", "window_host_main.cpp"), "-o", out])
    return out


def run(exe, args):
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", f"sanitizer / program failure:\n{r.stdout[-500:]}\n{r.stderr[-2000:]}"
    return json.loads(r.stdout)


def test_positions_of_grammar_streams(exe, tmp_path):
    by = {c["name"]: c for c in fg.cases()}
    names = ["fixed_orders_big", "full_scale_sides_16", "seed5_1x32", "seed27_8x16", "lpc_rings_side_right_24", "seed29_1x16"]
    streams = [(by[n]["bits"], by[n]["rate"], by[n]["frames"]) for n in names]
    streams.insert(2, (16, 44100, []))  # a stream with no frames
    blocks = [[f["block"] for f in frames] for _, _, frames in streams]
    assert any(4096 in b for b in blocks) and any(1 in b for b in blocks) and [] in blocks
    assert all(len(set(b)) == len(b) for b in blocks)  # a different block size in every frame
    blob, args = bytearray(b"\xA5" * 5), []
    for bits, rate, frames in streams:
        if len(blob) % 2 == 0:
            blob += b"\xA5"
        args += [len(blob), bits, rate, len(frames)] + [len(f["frame"]) for f in frames]
        blob += b"".join(f["frame"] for f in frames)
    assert streams[-1][2] and len(streams[-1][2][-1]["frame"]) < 4096  # the blob ends with a frame, no byte after it
    path = os.path.join(str(tmp_path), "blob.bin")
    with open(path, "wb") as f:
        f.write(bytes(blob))
    res = run(exe, ["positions", path, len(streams)] + args)
    assert res["untouched"]
    for b, got in zip(blocks, res["streams"]):
        assert got["positions"] == [sum(b[:i]) for i in range(len(b))]
        assert got["total"] == sum(b)


def linear_cover(blocks, start, count):
    total = sum(blocks)
    take = min(count, max(total - start, 0))
    hit, at = [], 0
    for i, b in enumerate(blocks):
        if take and at + b > start and at < start + take:
            hit.append(i)
        at += b
    if not hit:
        return [0, 0, 0, 0, take]
    return [hit[0], len(hit), sum(blocks[i] for i in hit), start - sum(blocks[:hit[0]]), take]


@pytest.mark.parametrize("blocks", [
    [256, 256, 100],                   # a short last frame
    [4096, 1, 17, 1000, 2, 1, 576],    # the grammar's kind: every frame another size, 1-sample frames
    [5],
    [],
    list(range(1, 300)),               # more frames than one scan iteration
])
def test_cover_against_a_linear_search(exe, blocks):
    total = sum(blocks)
    bounds = [sum(blocks[:i]) for i in range(1, len(blocks))][:6]
    windows = [(0, 1), (0, total), (0, total + 1), (total, 1), (total + 1, 5), (total + 7, 0), (0, 0), (3, 0),
               (1, U64), (total - 1 if total else 0, U64), (U64, U64), (U64, 1), (0, U64)]  # start + count passes 64 bits
    for b in bounds:
        windows += [(b, 1), (b, 7), (b - 1, 1), (b - 1, 2), (b + 1, 3), (0, b), (max(b - 5, 0), min(b, 5)), (b, total)]
    assert any(s + c > U64 for s, c in windows)
    got = run(exe, ["cover", len(blocks)] + blocks + [len(windows)] + [v for w in windows for v in w])["covers"]
    for (start, count), g in zip(windows, got):
        assert g == linear_cover(blocks, start, count), (start, count)
    if total:
        assert got[windows.index((1, U64))][4] == total - 1  # clamped, not wrapped
        assert got[windows.index((total, 1))][1] == 0 and got[windows.index((0, total))][1] == len(blocks)


def test_copy_plan_against_memcpy(exe):
    assert run(exe, ["copy"])["cases"] == 16 * 16 * 49
