"""CPM_I16 (two's-complement 16-bit voxels read as SNORM, include/cpm/cpm.h) on the host side -- no GPU:

  * the binding knows the code and maps numpy int16 to it; a torch int16 tensor stays u16 unless dtype=CPM_I16 says otherwise;
  * cpm_volume_desc_default maps the type's range onto [0, 1] (format_offset 1, format_scaling 0.5) and leaves the other types alone;
  * the value rule w(v) and the write conversion of cpm_volume_mix, stated in numpy over all 65536 codes (what the GPU tests compare the
    device with): w(+-32767) = +-1 exactly, the conversion inverts w on every code but -32768, and ties go to the even integer;
  * 2 bytes per voxel in the binding's table, the delta encoder and the host layer's Volume."""
import ctypes as C

import numpy as np
import pytest

try:
    import torch  # noqa: F401  (first: a process that goes on to GPU tests must have loaded ONE HIP runtime -- torch's -- before libcpm_hip binds one)
except ImportError:
    pass

from test_sequence_delta_cpu import _apply, _check_format

F32 = np.float32
SPECIALS = np.array([-32768, -32767, -1, 0, 1, 32767], np.int16)


def widen(v):
    """w(v): the F32 volume an I16 volume is held to, as the issue states it"""
    return np.maximum(v, -32767).astype(np.float32) * np.float32(1 / 32767)


def snorm_write(m):
    """cpm_volume_mix's write conversion of an f32 mix m: (int16) rint(clamp(m, -1, 1) * 32767), ties to even"""
    m = np.asarray(m, F32)
    return np.rint(np.clip(m, F32(-1), F32(1)) * F32(32767)).astype(np.int16)


def test_the_code_and_its_mappings(cpm):
    B = cpm.binding
    assert B.CPM_I16 == 4
    assert B._np_dtype_code(np.int16) == 4
    assert [B._np_dtype_code(t) for t in (np.uint8, np.uint16, np.float32, np.float16)] == [B.CPM_U8, B.CPM_U16, B.CPM_F32, B.CPM_F16]
    assert int(B._volume_desc_like(np.zeros((11, 9, 7), np.int16)).dtype) == B.CPM_I16


def test_torch_int16_stays_u16_without_the_keyword(cpm):
    torch = pytest.importorskip("torch")
    B = cpm.binding
    t = torch.zeros(2, dtype=torch.int16)
    assert B._dtype_code(t) == 1 == B.CPM_U16
    assert B._dtype_code(t, None) == B.CPM_U16 and B._dtype_code(t, B.CPM_U16) == B.CPM_U16
    assert B._dtype_code(t, B.CPM_I16) == B.CPM_I16
    assert B._dtype_code(torch.zeros(2, dtype=torch.float32), B.CPM_F32) == B.CPM_F32
    for other in (torch.uint8, torch.float16, torch.float32):
        with pytest.raises(ValueError):
            B._dtype_code(torch.zeros(2, dtype=other), B.CPM_I16)


def test_default_desc_maps_the_range_onto_0_1(cpm):
    B = cpm.binding
    d = B.default_volume_desc((7, 9, 11), B.CPM_I16)
    assert int(d.dtype) == 4 and tuple(d.dims) == (7, 9, 11)
    assert d.format_offset == 1.0 and d.format_scaling == 0.5
    lo, hi = [(float(w) + d.format_offset) * (1.0 - d.format_scaling) for w in widen(np.array([-32768, 32767], np.int16))]
    assert (lo, hi) == (0.0, 1.0)
    for code in (B.CPM_U8, B.CPM_U16, B.CPM_F32, B.CPM_F16):
        e = B.default_volume_desc((7, 9, 11), code)
        assert e.format_offset == 0.0 and e.format_scaling == 0.0


def test_value_rule_and_write_conversion_over_every_code():
    v = np.arange(-32768, 32768, dtype=np.int32).astype(np.int16)
    w = widen(v)
    k = F32(1 / 32767)
    assert float(k).hex() == "0x1.0002000000000p-15" and k == F32(1) / F32(32767)
    assert w.dtype == np.float32 and w[0] == w[1] == F32(-1) and w[-1] == F32(1) and w[32768] == 0
    assert np.all(np.diff(w[1:]) > 0)                                    # strictly increasing from -32767 on
    back = snorm_write(w)
    assert back.dtype == np.int16 and np.array_equal(back, np.maximum(v, -32767))
    # clamping, and ties to even: products that are exactly k + 0.5 in f32
    assert snorm_write([-7.0, -1.0000001, 1.5, np.inf, -np.inf]).tolist() == [-32767, -32767, 32767, 32767, -32767]
    halves = (np.arange(-2000, 2000, dtype=np.float32) + F32(0.5))
    m = (halves / F32(32767)).astype(F32)
    p = m * F32(32767)
    tie = p == halves
    assert tie.sum() > 100
    got = snorm_write(m[tie]).astype(np.int64)
    lo = np.floor(halves[tie]).astype(np.int64)
    assert np.array_equal(got, np.where(lo % 2 == 0, lo, lo + 1))
    near = snorm_write(m[~tie]).astype(np.int64)                          # the others: the nearest integer of the f32 product
    assert np.array_equal(near, np.floor(p[~tie].astype(np.float64) + 0.5).astype(np.int64))


def test_element_sizes(cpm):
    B = cpm.binding
    assert B.DTYPE_SIZE == {B.CPM_U8: 1, B.CPM_U16: 2, B.CPM_F32: 4, B.CPM_F16: 2, B.CPM_I16: 2}
    for code, dt in ((B.CPM_U8, np.uint8), (B.CPM_U16, np.uint16), (B.CPM_F32, np.float32), (B.CPM_F16, np.float16), (B.CPM_I16, np.int16)):
        assert np.dtype(dt).itemsize == B.DTYPE_SIZE[code] and B._np_dtype_code(dt) == code
    cpm.build.build_host_library()
    lib = C.CDLL(str(B.LIB_PATH.parent / "libcpm_host.so"))
    lib.cpmh_volume_element_size.argtypes = [C.c_int]
    lib.cpmh_volume_format.restype, lib.cpmh_volume_format.argtypes = C.c_char_p, [C.c_int]
    assert lib.cpmh_volume_element_size(B.CPM_I16) == 2 and lib.cpmh_volume_format(B.CPM_I16) == b"INT16"
    assert [lib.cpmh_volume_element_size(d) for d in (B.CPM_U8, B.CPM_U16, B.CPM_F32, B.CPM_F16)] == [1, 2, 4, 2]


def test_the_bindings_one_table_agrees_with_numpy_and_the_host_layer(cpm):
    """binding.VOXEL_TYPES (what DTYPE_SIZE and the dtype maps are derived from) against numpy's item sizes and cpm_dtype_size as the
    host layer's Volume reports it"""
    B = cpm.binding
    assert [row[0] for row in B.VOXEL_TYPES] == [B.CPM_U8, B.CPM_U16, B.CPM_F32, B.CPM_F16, B.CPM_I16] == list(B.DTYPE_SIZE)
    cpm.build.build_host_library()
    lib = C.CDLL(str(B.LIB_PATH.parent / "libcpm_host.so"))
    lib.cpmh_volume_element_size.argtypes = [C.c_int]
    for code, np_name, torch_name, size in B.VOXEL_TYPES:
        assert size == B.DTYPE_SIZE[code] == np.dtype(np_name).itemsize == lib.cpmh_volume_element_size(code)
        assert B._np_dtype_code(np_name) == code and torch_name in (np_name, None)


@pytest.mark.parametrize("dims", [(7, 9, 11), (24, 24, 24)])
def test_i16_delta_decodes_to_the_exact_bytes(cpm, dims):
    """the delta encoder counts 2 bytes per I16 voxel: its runs rebuild the next step byte for byte"""
    B = cpm.binding
    rng = np.random.default_rng(sum(dims))
    a = rng.integers(-32768, 32768, dims[::-1]).astype(np.int16)
    a.reshape(-1)[:SPECIALS.size] = SPECIALS
    b = a.copy()
    flat = b.reshape(-1)
    for _ in range(4):
        at = int(rng.integers(0, flat.size - 40))
        flat[at:at + 40] = rng.integers(-32768, 32768, 40).astype(np.int16)
    flat[-SPECIALS.size:] = SPECIALS[::-1]
    runs, payload = B.sequence_delta_encode(a, b)
    assert len(runs) > 0
    _check_format(runs, payload, a, b)
    assert np.array_equal(_apply(a, runs, payload), b)
    runs, payload = B.sequence_delta_encode(a, a.copy())
    assert runs.shape == (0, 3) and payload == b""
