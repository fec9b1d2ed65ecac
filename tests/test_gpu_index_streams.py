"""The many-streams device frame index (flacgpu_flac_index_streams_device) on the GPU: every
stream of index_cases.cases() in ONE call, against the host index and against the single-stream
call, the caps, the untouched entries, and the launch count."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

import decode_cases as dc  # noqa: E402
import index_cases as ic  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 5  # table entries before the first slice, between two slices and after the last
FILL64, FILL32 = 0xA5A5A5A5A5A5A5A5, 0xA5A5A5A5


def _torch():
    import torch

    return torch, torch.device("cuda", 0)


@pytest.fixture(scope="module")
def ctx():
    import flacgpu

    with flacgpu.Decoder(2, 16, 44100, device=0, max_frames=64) as d:
        yield d


@pytest.fixture(scope="module")
def streams():
    """[(name, data, bits, rate)]: the shared cases, a zero-length stream, and one of more than two
    16 KiB groups made of golden frames."""
    out = list(ic.cases())
    out.insert(3, ("empty", b"", 16, 44100))
    c = dc.FRAME_CASES[0]
    _, raw = dc.golden_frames(c)
    long = raw * (2 * 16384 // len(raw) + 2)
    assert len(long) > 2 * 16384
    out.append(("long_golden", long, c["bits"], c["rate"]))
    return out


@pytest.fixture(scope="module")
def wanted(streams):
    return [ic.host_index(s[1]) for s in streams]  # computed once, shared, never changed


def place(streams):
    """The streams back to back at odd offsets in a 0xA5-filled buffer -> (host array, [offset])."""
    blob, offs = bytearray(b"\xA5" * 3), []
    for _, data, _, _ in streams:
        if len(blob) % 2 == 0:
            blob += b"\xA5"
        offs.append(len(blob))
        blob += data
    blob += b"\xA5" * 16
    return np.frombuffer(bytes(blob), dtype=np.uint8).copy(), offs


def index_streams(d, streams, caps=None):
    """One flacgpu_flac_index_streams_device call -> ([(status, n_frames)], offsets table, sizes
    table, [first entry of each slice], caps)."""
    import flacgpu

    torch, dev = _torch()
    host, offs = place(streams)
    caps = [len(s[1]) // 8 + 1 for s in streams] if caps is None else caps
    first, at = [], GUARD
    for c in caps:
        first.append(at)
        at += c + GUARD
    d_buf = torch.from_numpy(host).to(dev)
    d_off = torch.full((8 * at,), 0xA5, dtype=torch.uint8, device=dev)
    d_fb = torch.full((4 * at,), 0xA5, dtype=torch.uint8, device=dev)
    d_res = torch.full((16 * len(streams),), 0xA5, dtype=torch.uint8, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    d.flac_index_streams_device(d_buf.data_ptr(), offs, [len(s[1]) for s in streams], first, caps, d_off.data_ptr(),
                                d_fb.data_ptr(), d_res.data_ptr(), stream_bits=[s[2] for s in streams],
                                stream_rates=[s[3] for s in streams], stream=st)
    d.sync_check(st)
    res = (flacgpu.IndexResult * len(streams)).from_buffer_copy(d_res.cpu().numpy().tobytes())
    assert all(r.reserved == 0 for r in res)
    return ([(r.status, r.n_frames) for r in res], np.frombuffer(d_off.cpu().numpy().tobytes(), dtype=np.uint64),
            np.frombuffer(d_fb.cpu().numpy().tobytes(), dtype=np.uint32), first, offs)


def check_tables(streams, wanted, got, offs_t, sizes_t, first, offs, too_small=()):
    written = np.zeros(len(offs_t), dtype=bool)
    for i, (s, want) in enumerate(zip(streams, wanted)):
        if want is None:
            assert got[i] == (1, 0), s[0]
        elif i in too_small:
            assert got[i] == (2, len(want)), s[0]
        else:
            n = len(want)
            assert got[i] == (0, n), s[0]
            assert list(sizes_t[first[i]:first[i] + n]) == want, s[0]
            assert list(offs_t[first[i]:first[i] + n]) == [offs[i] + int(v) for v in np.cumsum([0] + want)[:-1]], s[0]
            written[first[i]:first[i] + n] = True
    # invalid and too-small streams' slices, entries past each n_frames, the guard entries
    assert (offs_t[~written] == FILL64).all() and (sizes_t[~written] == FILL32).all()


def test_all_cases_in_one_call(ctx, streams, wanted):
    assert any(w is None for w in wanted) and wanted[3] == []
    got, offs_t, sizes_t, first, offs = index_streams(ctx, streams)
    assert all(o % 2 == 1 for o in offs)
    check_tables(streams, wanted, got, offs_t, sizes_t, first, offs)


def test_each_stream_equals_the_single_call(ctx, streams):
    import flacgpu

    torch, dev = _torch()
    got, offs_t, sizes_t, first, offs = index_streams(ctx, streams)
    host, _ = place(streams)
    d_buf = torch.from_numpy(host).to(dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    for i, (name, data, bits, rate) in enumerate(streams):
        cap = len(data) // 8 + 1
        d_off = torch.full((8 * cap,), 0xA5, dtype=torch.uint8, device=dev)
        d_fb = torch.full((4 * cap,), 0xA5, dtype=torch.uint8, device=dev)
        d_res = torch.full((16,), 0xA5, dtype=torch.uint8, device=dev)
        ctx.flac_index_device(d_buf.data_ptr() + offs[i], len(data), d_off.data_ptr(), d_fb.data_ptr(), cap,
                              d_res.data_ptr(), stream_bits=bits, stream_rate=rate, stream=st)
        ctx.sync_check(st)
        r = flacgpu.IndexResult.from_buffer_copy(d_res.cpu().numpy().tobytes())
        assert got[i] == (r.status, r.n_frames), name
        one_off = np.frombuffer(d_off.cpu().numpy().tobytes(), dtype=np.uint64)
        one_fb = np.frombuffer(d_fb.cpu().numpy().tobytes(), dtype=np.uint32)
        n = int(r.n_frames) if r.status == 0 else 0
        assert (sizes_t[first[i]:first[i] + cap] == one_fb).all(), name
        assert (offs_t[first[i]:first[i] + n] == one_off[:n] + np.uint64(offs[i])).all(), name
        assert (offs_t[first[i] + n:first[i] + cap] == one_off[n:]).all(), name


def test_cap_one_too_small_on_one_stream(ctx, streams, wanted):
    by = [s[0] for s in streams]
    sub = [by.index("hand_built") - 1, by.index("hand_built"), by.index("hand_built") + 1]
    some = [streams[i] for i in sub]
    want = [wanted[i] for i in sub]
    assert all(w for w in want)
    caps = [len(s[1]) // 8 + 1 for s in some]
    caps[1] = len(want[1]) - 1
    got, offs_t, sizes_t, first, offs = index_streams(ctx, some, caps)
    check_tables(some, want, got, offs_t, sizes_t, first, offs, too_small={1})
    caps[1] = len(want[1])  # exactly enough
    got, offs_t, sizes_t, first, offs = index_streams(ctx, some, caps)
    check_tables(some, want, got, offs_t, sizes_t, first, offs)


def test_one_timed_launch_whatever_the_stream_count(ctx, streams, wanted):
    import flacgpu

    nine = streams[:9]
    ctx.set_timing(True)
    try:
        ctx.reset_timing()
        got, offs_t, sizes_t, first, offs = index_streams(ctx, nine)
        launches, ms = ctx.kernel_time(flacgpu.K_INDEX)
    finally:
        ctx.set_timing(False)
    assert launches == 1 and ms > 0
    check_tables(nine, wanted[:9], got, offs_t, sizes_t, first, offs)


def test_argument_checks(ctx):
    import ctypes

    L = ctx.lib
    buf = ctypes.create_string_buffer(64)
    u64 = (ctypes.c_uint64 * 2)(0, 8)
    f = L.flacgpu_flac_index_streams_device
    assert f(ctx.ctx, None, 2, u64, u64, None, None, u64, u64, buf, buf, buf, None) == -2
    assert f(ctx.ctx, buf, 2, None, u64, None, None, u64, u64, buf, buf, buf, None) == -2
    assert f(ctx.ctx, buf, 2, u64, u64, None, None, None, u64, buf, buf, buf, None) == -2
    assert f(ctx.ctx, buf, 2, u64, u64, None, None, u64, u64, buf, buf, None, None) == -2
    big = (ctypes.c_uint64 * 2)(1 << 32, 8)
    assert f(ctx.ctx, buf, 2, u64, big, None, None, u64, u64, buf, buf, buf, None) == -2
    many = (ctypes.c_uint64 * 65536)()
    assert f(ctx.ctx, buf, 65536, many, many, None, None, many, many, buf, buf, buf, None) == -2
