"""The owners of HIP resources (zig-flac_amd/csrc/fg_own.hpp: DevBuf, Stream, Event, Carve, fit) on
the host, under AddressSanitizer, LeakSanitizer and UBSan, through the stand-alone program
tests/cpp/own_host_main.cpp.  No GPU: the program is built against tests/cpp/hipstub, a stand-in
<hip/hip_runtime.h> whose allocations are host memory and whose calls are counted and logged.

Every context, plan and communicator of the library holds its device memory, streams and events in
these owners and has no teardown code of its own, so what they call, in which order, and what a
failure or a move leaves behind is checked here, at 0, 1, 255, 256 and 257 elements: the program
prints one line per failed check, and a buffer it does not free, frees twice or writes past is a
sanitizer report."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_owners(tmp_path):
    exe = os.path.join(str(tmp_path), "own_host_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I", os.path.join(HERE, "cpp", "hipstub"),
                           os.path.join(HERE, "cpp", "own_host_main.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    # a sanitizer report makes the program exit non-zero with text on stderr: both are asserted absent
    assert r.stderr == "", r.stderr[-2000:]
    assert r.returncode == 0 and r.stdout == "ok\n", r.stdout[-2000:]
