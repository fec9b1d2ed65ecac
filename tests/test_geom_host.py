"""The kernel geometry of an encoder context (zig-flac_amd/csrc/fg_geom.hpp: enc_geometry) on the
host, under AddressSanitizer and UBSan, through the stand-alone program
tests/cpp/geom_host_main.cpp, against tests/golden/geometry.json.  No GPU.

Which pack kernel a configuration gets, with how many threads and how much LDS, whether staging is
double-buffered, whether analysis and pack run in channel halves, and whether the configuration is
refused: flacgpu_open takes all of it from enc_geometry, so a change to it shows here as a changed
row, not as a slower benchmark.  The fixture was written by the decision block that flacgpu_open
had before enc_geometry existed, run over matrix() with the knobs in its environment; a row changes
only together with the kernel it describes."""
import json
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
LDS_LIMIT = 160 * 1024

# the bench presets: (channels, bits, prediction)
PRESETS = {"c2": (2, 16, 0), "c3": (2, 24, 8), "c4": (8, 24, 0), "c5": (2, 32, 12)}
# every geometry-changing release knob, at each value its parsing tells apart ("" : set but empty)
KNOB_VALUES = {
    "FLACGPU_PACK_DBUF": ("1", "0", ""),
    "FLACGPU_PACK4": ("0", "1"),
    "FLACGPU_PACKW": ("0", "1", "2"),
    "FLACGPU_PACKW_WPS": ("2", "4"),
    "FLACGPU_PACKW_DBUF": ("1", "0"),
    "FLACGPU_PACK_SPLIT": ("0", "1"),
    "FLACGPU_MD5_KERNEL": ("0", "1", "2"),
}
# k_packw's own knobs act only where k_packw runs: forced on, for the presets that do not take it
PACKW_ON = ("FLACGPU_PACK4=0", "FLACGPU_PACKW=1")
COMBINED = (PACKW_ON, PACKW_ON + ("FLACGPU_PACKW_WPS=2",), PACKW_ON + ("FLACGPU_PACKW_DBUF=0",))
DIAG_KNOBS = ((), ("FLACGPU_ANA1=0",), ("FLACGPU_ANA1=1",), ("FLACGPU_ANA1=2",), ("FLACGPU_FUSED=1",),
              ("FLACGPU_FUSED=0",))


def row(channels, bits, prediction, stereo=1, block=4096, knobs=()):
    return [str(channels), str(bits), str(prediction), str(stereo), str(block), *knobs]


def matrix():
    """(diag build?, program arguments) of every pinned row, in the fixture's order."""
    rows = []
    for ch in range(1, 9):
        for bits in (8, 16, 24, 32):
            for pred in (0, 8, 12):
                rows.append((False, row(ch, bits, pred)))
                if ch == 2:
                    rows.append((False, row(ch, bits, pred, stereo=0)))
    rows.append((False, row(2, 16, 0, block=1152)))
    for ch, bits, pred in PRESETS.values():
        for name, values in KNOB_VALUES.items():
            for v in values:
                rows.append((False, row(ch, bits, pred, knobs=(f"{name}={v}",))))
        for knobs in COMBINED:
            rows.append((False, row(ch, bits, pred, knobs=knobs)))
    for knobs in DIAG_KNOBS:
        rows.append((True, row(2, 16, 0, knobs=knobs)))
    return rows


MATRIX = matrix()
with open(os.path.join(HERE, "golden", "geometry.json")) as _f:
    GOLDEN = json.load(_f)["rows"]


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    """geom_host_main built with -fsanitize=address,undefined: [release, -DFG_DIAG=1]."""
    d = tmp_path_factory.mktemp("geomhost")
    exes = []
    for diag in (0, 1):
        exe = os.path.join(str(d), f"geom_host_main{diag}")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=undefined", f"-DFG_DIAG={diag}",
                               os.path.join(HERE, "cpp", "geom_host_main.cpp"), "-o", exe])
        exes.append(exe)
    return exes


def run(exe, args):
    """A sanitizer report makes the program exit non-zero with text on stderr: both are asserted absent."""
    r = subprocess.run([exe, *args], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", f"sanitizer / program failure for {args}:\n{r.stderr[-2000:]}"
    return json.loads(r.stdout)


@pytest.fixture(scope="module")
def results(programs):
    return [run(programs[diag], args) for diag, args in MATRIX]


def test_fixture_holds_exactly_the_matrix():
    assert [(g["diag"], g["args"]) for g in GOLDEN] == [(d, a) for d, a in MATRIX]


def test_geometry_matches_the_fixture(results):
    for got, want in zip(results, GOLDEN):
        assert got == want["out"], (want["diag"], want["args"])


def test_refusals():
    """The LDS check: 8 x 32-bit channels with LPC do not fit the tail analysis; 7 do, and so do 8
    without LPC.  What is refused, and nothing else, has rc = FLACGPU_ERR_INVALID_CONFIG."""
    by = {(g["diag"], *g["args"]): g["out"] for g in GOLDEN}
    refused = [k for k, v in by.items() if v["rc"] != 0]
    assert refused and all(by[k] == {"rc": -1} for k in refused)
    assert by[(False, "8", "32", "8", "1", "4096")]["rc"] == -1
    assert by[(False, "8", "32", "12", "1", "4096")]["rc"] == -1
    assert by[(False, "7", "32", "12", "1", "4096")]["rc"] == 0
    assert by[(False, "8", "32", "0", "1", "4096")]["rc"] == 0


def test_block_size_does_not_enter(results):
    by = {(d, *a): r for (d, a), r in zip(MATRIX, results)}
    assert by[(False, "2", "16", "0", "1", "1152")] == by[(False, "2", "16", "0", "1", "4096")]


def test_invariants_of_accepted_rows(results):
    """Independent of the fixture: what every launch needs to be legal on a gfx950 CU."""
    n = 0
    for (diag, args), g in zip(MATRIX, results):
        if g["rc"]:
            continue
        n += 1
        for f in ("lds", "lds_tail", "lds_pack", "lds_pack4", "lds_split", "lds_psplit", "lds_fused"):
            assert g[f] <= LDS_LIMIT, (args, f)
        for f in ("nt", "nt_pack", "nt_pack4", "nt_split", "nt_psplit"):
            assert g[f] % 64 == 0 and g[f] <= 1024, (args, f)
        assert g["nt"] and g["nt_pack"] and g["lds"] and g["lds_tail"] and g["lds_pack"], args
        assert not g["pack_split"] or g["ana_split"], args
        assert not g["nt_pack4"] or g["lds_pack4"], args
        assert bool(g["ana_split"]) == bool(g["nt_split"]) == bool(g["lds_split"]), args
        assert bool(g["pack_split"]) == bool(g["nt_psplit"]) == bool(g["lds_psplit"]), args
    assert n > 100


def test_release_program_does_not_know_the_diagnostic_knobs(programs):
    r = subprocess.run([programs[0], *row(2, 16, 0, knobs=("FLACGPU_FUSED=1",))], capture_output=True, text=True)
    assert r.returncode == 2 and "not a knob" in r.stderr
