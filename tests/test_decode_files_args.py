"""The many-files decode's three entry points (flacgpu_flac_index_streams_device,
flacgpu_decode_streams_device, flacgpu_decode_files): the argument checks that need no device, and
their place in the binding."""
import ctypes

import flacgpu


def _arrays():
    u64 = (ctypes.c_uint64 * 2)(0, 8)
    return ctypes.create_string_buffer(64), u64


def test_index_streams_argument_checks_without_a_device():
    L = flacgpu.load_library()
    buf, u64 = _arrays()
    f = L.flacgpu_flac_index_streams_device
    assert f(None, buf, 2, u64, u64, None, None, u64, u64, buf, buf, buf, None) == -2  # no context
    assert f(None, None, 2, None, None, None, None, None, None, None, None, None, None) == -2
    assert f(None, buf, 0, None, None, None, None, None, None, None, None, None, None) == -2


def test_decode_streams_argument_checks_without_a_device():
    L = flacgpu.load_library()
    buf, u64 = _arrays()
    f = L.flacgpu_decode_streams_device
    assert f(None, buf, 2, u64, u64, None, None, buf, u64, u64, buf, None, None) == -2  # no context
    assert f(None, None, 2, None, None, None, None, None, None, None, None, None, None) == -2
    assert f(None, buf, 0, None, None, None, None, None, None, None, None, None, None) == -2


def test_decode_files_argument_checks_without_a_device():
    L = flacgpu.load_library()
    ptrs = (ctypes.c_void_p * 1)()
    sz = (ctypes.c_size_t * 1)()
    ns = (ctypes.c_uint64 * 1)()
    st = (ctypes.c_int * 1)()
    assert L.flacgpu_decode_files(None, 1, ptrs, sz, ptrs, sz, ns, None, st) == -2  # no context
    assert L.flacgpu_decode_files(None, 1, None, None, None, None, None, None, None) == -2
    assert L.flacgpu_decode_files(None, 0, None, None, None, None, None, None, None) == -2


def test_binding():
    assert ctypes.sizeof(flacgpu.StreamResult) == 32
    for name in ("flacgpu_flac_index_streams_device", "flacgpu_decode_streams_device", "flacgpu_decode_files"):
        assert name in flacgpu.exported_symbols()
    assert flacgpu.K_INDEX == 7 and len(flacgpu.KERNEL_NAMES) == 5  # no kernel ids added
    for name in ("flac_index_streams_device", "decode_streams_device", "decode_files"):
        assert hasattr(flacgpu.Decoder, name)
