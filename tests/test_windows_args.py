"""The sample-window decode's three entry points (flacgpu_flac_positions_streams_device,
flacgpu_decode_windows_device, flacgpu_decode_files_windows): the argument checks that need no
device, and their place in the binding."""
import ctypes

import flacgpu


def _arrays():
    u64 = (ctypes.c_uint64 * 2)(0, 8)
    u32 = (ctypes.c_uint32 * 2)(0, 1)
    return ctypes.create_string_buffer(64), u64, u32


def test_positions_argument_checks_without_a_device():
    L = flacgpu.load_library()
    buf, u64, _ = _arrays()
    f = L.flacgpu_flac_positions_streams_device
    assert f(None, buf, 2, u64, u64, buf, buf, buf, None, None, buf, buf, None) == -2  # no context
    assert f(None, None, 2, None, None, None, None, None, None, None, None, None, None) == -2
    assert f(None, buf, 65536, u64, u64, buf, buf, buf, None, None, buf, buf, None) == -2
    assert f(None, buf, 0, None, None, None, None, None, None, None, None, None, None) == -2


def test_decode_windows_argument_checks_without_a_device():
    L = flacgpu.load_library()
    buf, u64, u32 = _arrays()
    f = L.flacgpu_decode_windows_device
    assert f(None, buf, 2, u64, buf, buf, buf, buf, buf, 2, u32, u64, u64, buf, u64, u64, buf, None) == -2  # no context
    assert f(None, None, 2, None, None, None, None, None, None, 2, None, None, None, None, None, None, None, None) == -2
    assert f(None, buf, 2, u64, buf, buf, buf, buf, buf, 65536, u32, u64, u64, buf, u64, u64, buf, None) == -2
    assert f(None, buf, 0, None, None, None, None, None, None, 0, None, None, None, None, None, None, None, None) == -2


def test_decode_files_windows_argument_checks_without_a_device():
    L = flacgpu.load_library()
    ptrs = (ctypes.c_void_p * 1)()
    sz = (ctypes.c_size_t * 1)()
    ns = (ctypes.c_uint64 * 1)()
    st = (ctypes.c_int * 1)()
    _, u64, u32 = _arrays()
    f = L.flacgpu_decode_files_windows
    assert f(None, 1, ptrs, sz, 1, u32, u64, u64, ptrs, sz, ns, st) == -2  # no context
    assert f(None, 1, None, None, 1, None, None, None, None, None, None, None) == -2
    assert f(None, 1, ptrs, sz, 65536, u32, u64, u64, ptrs, sz, ns, st) == -2
    assert f(None, 0, None, None, 0, None, None, None, None, None, None, None) == -2


def test_binding():
    assert ctypes.sizeof(flacgpu.WindowResult) == 32
    assert (flacgpu.WINDOW_OK, flacgpu.WINDOW_BAD_INDEX, flacgpu.WINDOW_BAD_FRAME, flacgpu.WINDOW_TOO_SMALL) == (0, 1, 2, 3)
    for name in ("flacgpu_flac_positions_streams_device", "flacgpu_decode_windows_device", "flacgpu_decode_files_windows"):
        assert name in flacgpu.exported_symbols()
        assert hasattr(flacgpu.load_library(), name)
    assert flacgpu.K_INDEX == 7 and len(flacgpu.KERNEL_NAMES) == 5  # no kernel ids added
    for name in ("flac_positions_streams_device", "decode_windows_device", "decode_files_windows"):
        assert hasattr(flacgpu.Decoder, name)
    assert flacgpu.load_library().flacgpu_abi_version() == 5
