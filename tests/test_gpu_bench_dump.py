"""bench.py --dump-outputs: the arrays it writes are what the timed path left after its last step.

A small Workload (the class bench.py times) runs a warm-up and three timed steps; dump_outputs()
then writes frame sizes, offsets, total, carried MD5 states and the bitstream sample, which are
compared with the CPU restatement at the last step's frame numbers.  A second workload over the same
seeded input dumps the same arrays.
"""
import argparse
import os

import numpy as np
import pytest

import bench
import oracle_ref

pytestmark = pytest.mark.gpu

S, F, CH, BITS, RATE = 24, 3, 2, 16, 44100  # 72 frames: several streams, several blocks each
FB = CH * (BITS // 8)
NAMES = {"frame_bytes", "frame_offsets", "total_bytes", "md5_h", "md5_bytes", "sample_frames", "bitstream_sample"}


def _run(path, buf):
    import torch

    import flacgpu

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    enc = flacgpu.Encoder(CH, BITS, RATE, device=0, max_frames=S * F)
    d_pcm = torch.from_numpy(buf).to(dev)
    w = bench.Workload(enc, d_pcm, S, F, FB, dev)
    bench.run_timed(w, 3, 1)
    bench.dump_outputs(w, str(path))
    return enc, w, dev


def _load(path):
    return {os.path.splitext(f)[0]: np.load(os.path.join(path, f)) for f in os.listdir(path)}


@pytest.fixture(scope="module")
def pcm():
    return bench.build_input(argparse.Namespace(streams=S, frames=S * F, channels=CH, bits=BITS, rate=RATE), 0)


def test_dump_is_the_last_steps_output(tmp_path, pcm):
    args = argparse.Namespace(channels=CH, bits=BITS, rate=RATE, lpc=0)
    enc, w, dev = _run(tmp_path / "a", pcm)
    d = _load(tmp_path / "a")
    assert set(d) == NAMES
    assert all(a.dtype in (np.float32, np.float64) for a in d.values())
    assert sum(a.nbytes for a in d.values()) <= 64 << 20
    n_per = F * 4096
    first = 3 * F  # one warm-up and three timed steps: the last step's frames start at 3 F
    ref_sizes, ref_body = [], []
    for s in range(S):
        body, sizes, _ = oracle_ref.encode_stream(bytes(pcm[s * n_per * FB:(s + 1) * n_per * FB]), CH, BITS, RATE,
                                                  first_frame=first)
        ref_sizes += sizes
        ref_body.append(body)
    ref_body = b"".join(ref_body)
    assert d["frame_bytes"].tolist() == ref_sizes
    assert d["frame_offsets"].tolist() == [0] + np.cumsum(ref_sizes)[:-1].tolist()
    assert d["total_bytes"].tolist() == [len(ref_body)]
    # fewer frames than the sample takes: every frame, in order = the whole bitstream
    assert d["sample_frames"].tolist() == list(range(S * F))
    assert d["bitstream_sample"].astype(np.uint8).tobytes() == ref_body
    assert d["md5_h"].shape == (S, 4) and d["md5_bytes"].tolist() == [4 * n_per * FB] * S
    # the carried states the dump read finalise to hashlib's digests (and the frames match once more)
    ok, _ = bench.verify(args, w, pcm, FB, S, dev)
    assert ok
    w.close()
    enc.close()


def test_dump_repeats_and_respects_its_byte_budget(tmp_path, pcm, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BYTES", 100000)
    runs = []
    for name in ("a", "b"):
        enc, w, _ = _run(tmp_path / name, pcm)
        w.close()
        enc.close()
        runs.append(_load(tmp_path / name))
    a, b = runs
    assert set(a) == set(b) == NAMES
    for k in NAMES:
        assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), k
    picks = a["sample_frames"].astype(np.int64)
    assert 0 < len(picks) < S * F and np.all(np.diff(picks) > 0)
    assert len(a["bitstream_sample"]) == int(a["frame_bytes"][picks].sum()) <= 100000
