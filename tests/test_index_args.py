"""flacgpu_flac_index_device's argument checks that need no device, and its place in the binding."""
import ctypes

import flacgpu


def test_argument_checks_without_a_device():
    L = flacgpu.load_library()
    buf = ctypes.create_string_buffer(64)
    assert L.flacgpu_flac_index_device(None, buf, 8, 16, 0, buf, buf, 1, buf, None) == -2
    assert L.flacgpu_flac_index_device(None, buf, 8, 16, 0, None, None, 1, None, None) == -2
    assert L.flacgpu_flac_index_device(None, None, 0, 16, 0, None, None, 0, None, None) == -2


def test_binding_constants():
    assert flacgpu.K_INDEX == 7 and "flacgpu_flac_index_device" in flacgpu.exported_symbols()
    assert len(flacgpu.KERNEL_NAMES) == 5  # bench.py enumerates it: the index is not one of its columns
    assert ctypes.sizeof(flacgpu.IndexResult) == 16
    assert (flacgpu.INDEX_OK, flacgpu.INDEX_INVALID, flacgpu.INDEX_TOO_SMALL) == (0, 1, 2)
