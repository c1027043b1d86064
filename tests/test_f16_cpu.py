"""CPM_F16 (IEEE binary16 voxels, include/cpm/cpm.h) on the host side -- no GPU:

  * the binding knows the code and maps numpy float16 to it; cpm_volume_desc_default takes it;
  * cpm_sequence_delta_encode on a float16 sequence (+-0, subnormals, +-inf and NaN bit patterns) decodes back to the exact bytes, and the
    comparison is bytewise (-0 against +0, one NaN against another are changes);
  * the host layer's Volume stores 2 bytes per FLOAT16 voxel."""
import ctypes as C

import numpy as np
import pytest

from test_sequence_delta_cpu import _apply, _check_format


def _specials():
    """One of every binary16 class: +-0, the smallest / largest subnormal, the smallest normal, the largest finite, +-inf, quiet and
    signalling NaNs of both signs."""
    bits = [0x0000, 0x8000, 0x0001, 0x8001, 0x03FF, 0x83FF, 0x0400, 0x8400, 0x7BFF, 0xFBFF, 0x7C00, 0xFC00, 0x7E00, 0xFE00, 0x7C01,
            0xFD55, 0x3C00, 0xBC00]
    return np.array(bits, np.uint16).view(np.float16)


def test_the_code_and_its_mappings(cpm):
    B = cpm.binding
    assert B.CPM_F16 == 3
    assert B._np_dtype_code(np.float16) == B.CPM_F16
    assert [B._np_dtype_code(t) for t in (np.uint8, np.uint16, np.float32)] == [B.CPM_U8, B.CPM_U16, B.CPM_F32]
    d = B.default_volume_desc((33, 20, 17), B.CPM_F16)
    assert int(d.dtype) == 3 and tuple(d.dims) == (33, 20, 17)
    assert int(B._volume_desc_like(np.zeros((17, 20, 33), np.float16)).dtype) == B.CPM_F16


def test_torch_float16_maps_to_f16_and_int16_stays_u16(cpm):
    torch = pytest.importorskip("torch")
    B = cpm.binding
    assert B._dtype_code(torch.zeros(2, dtype=torch.float16)) == B.CPM_F16
    assert B._dtype_code(torch.zeros(2, dtype=torch.int16)) == B.CPM_U16


@pytest.mark.parametrize("dims", [(33, 20, 17), (24, 24, 24), (37, 5, 3)])
def test_f16_delta_decodes_to_the_exact_bytes(cpm, dims):
    B = cpm.binding
    rng = np.random.default_rng(sum(dims))
    shape = dims[::-1]
    a = rng.standard_normal(shape).astype(np.float16)
    sp = _specials()
    a.reshape(-1)[:sp.size] = sp
    b = a.copy()
    flat = b.reshape(-1)
    for _ in range(5):
        at = int(rng.integers(0, flat.size - 40))
        flat[at:at + 40] = rng.standard_normal(40).astype(np.float16) * np.float16(100)
    k = flat.size // 2
    flat[k:k + sp.size] = sp[::-1]
    flat[-1] = np.float16(7.5)
    runs, payload = B.sequence_delta_encode(a, b)
    assert len(runs) > 0
    _check_format(runs, payload, a, b)
    assert np.array_equal(_apply(a, runs, payload).view(np.uint16), b.view(np.uint16))
    runs, payload = B.sequence_delta_encode(a, a.copy())
    assert runs.shape == (0, 3) and payload == b""


def test_f16_steps_are_compared_bytewise(cpm):
    B = cpm.binding
    a = np.zeros((16, 16, 16), np.float16)
    a.reshape(-1)[100:200] = np.nan
    b = a.copy()
    b.reshape(-1)[5] = np.float16(-0.0)                                          # -0 == +0 as numbers, not as bytes
    b.reshape(-1)[150] = np.array([0x7E01], np.uint16).view(np.float16)[0]       # another NaN
    b.reshape(-1)[1000] = np.array([0x0001], np.uint16).view(np.float16)[0]      # the smallest subnormal
    runs, payload = B.sequence_delta_encode(a, b)
    _check_format(runs, payload, a, b)
    assert [r[0] for r in runs.tolist()] == [5 * 2 // 16, 150 * 2 // 16, 1000 * 2 // 16]
    assert _apply(a, runs, payload).view(np.uint16).reshape(-1)[150] == 0x7E01


def test_host_volume_has_2_byte_float16_elements(cpm):
    cpm.build.build_host_library()
    lib = C.CDLL(str(cpm.binding.LIB_PATH.parent / "libcpm_host.so"))
    lib.cpmh_volume_element_size.argtypes = [C.c_int]
    lib.cpmh_volume_format.restype, lib.cpmh_volume_format.argtypes = C.c_char_p, [C.c_int]
    B = cpm.binding
    assert lib.cpmh_volume_element_size(B.CPM_F16) == 2
    assert lib.cpmh_volume_format(B.CPM_F16) == b"FLOAT16"
    assert [lib.cpmh_volume_element_size(d) for d in (B.CPM_U8, B.CPM_U16, B.CPM_F32)] == [1, 2, 4]
    assert [lib.cpmh_volume_format(d) for d in (B.CPM_U8, B.CPM_U16, B.CPM_F32)] == [b"UINT8", b"UINT16", b"FLOAT32"]
