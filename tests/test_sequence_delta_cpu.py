"""cpm_sequence_delta_encode (include/cpm/cpm_ext.h, "delta uploads"): the format a streamed sequence sends instead of whole steps, decoded
here with numpy -- pure host code, no GPU.

  * applying the runs to `from` gives `to` byte for byte (u8 / u16 / f32, row lengths that are not multiples of 16 bytes, a short last piece);
  * runs are maximal, sorted and disjoint, payload_piece_offset is the prefix sum of their lengths;
  * the comparison is bytewise: -0.0 against +0.0 and NaNs with other payloads are changes;
  * identical steps give no runs, a step that differs everywhere is more than 3/4 of a step;
  * on BASELINE config 5's sequence the dirty pieces are numpy's count."""
import numpy as np
import pytest

PIECE = 16


def _pieces_changed(a, b):
    """bool per 16-byte piece of the flat blocks (the last piece may be short)."""
    x, y = a.reshape(-1).view(np.uint8), b.reshape(-1).view(np.uint8)
    n = (x.size + PIECE - 1) // PIECE
    pad = n * PIECE - x.size
    d = np.concatenate([x != y, np.zeros(pad, bool)]).reshape(n, PIECE)
    return d.any(axis=1)


def _apply(a, runs, payload):
    out = a.reshape(-1).view(np.uint8).copy()
    pay = np.frombuffer(payload, np.uint8)
    for first, n, off in runs.tolist():
        lo, hi = first * PIECE, min((first + n) * PIECE, out.size)
        out[lo:hi] = pay[off * PIECE: off * PIECE + (hi - lo)]
    return out.view(a.dtype).reshape(a.shape)


def _check_format(runs, payload, a, b):
    changed = _pieces_changed(a, b)
    assert runs.dtype == np.uint32 and runs.ndim == 2 and runs.shape[1] == 3
    covered = np.zeros(changed.size, bool)
    offset = 0
    for i, (first, n, off) in enumerate(runs.tolist()):
        assert n > 0 and off == offset
        if i:
            prev_end = runs[i - 1, 0] + runs[i - 1, 1]
            assert first > prev_end, "runs must be sorted, disjoint and maximal (no two touching)"
        covered[first:first + n] = True
        offset += n
    assert np.array_equal(covered, changed)
    nbytes = a.nbytes
    want = sum(min((f + n) * PIECE, nbytes) - f * PIECE for f, n, _ in runs.tolist())
    assert len(payload) == want
    assert np.array_equal(_apply(a, runs, payload).view(np.uint8), b.view(np.uint8))


def _clustered_change(rng, a, n_blobs=5):
    b = a.copy()
    flat = b.reshape(-1)
    for _ in range(n_blobs):
        at = int(rng.integers(0, flat.size))
        n = int(rng.integers(1, 40))
        if a.dtype == np.float32:
            flat[at:at + n] = rng.random(len(flat[at:at + n]), dtype=np.float32) + 2.0
        else:
            flat[at:at + n] ^= np.asarray(int(rng.integers(1, 200)), a.dtype)
    return b


@pytest.mark.parametrize("dtype,dims", [(np.uint8, (37, 20, 11)), (np.uint16, (33, 17, 9)), (np.float32, (24, 24, 24))])
def test_runs_applied_to_from_give_to(cpm, dtype, dims):
    B = cpm.binding
    rng = np.random.default_rng(sum(dims))
    shape = dims[::-1]
    if dtype == np.float32:
        a = rng.random(shape, dtype=np.float32)
    else:
        a = rng.integers(0, np.iinfo(dtype).max, shape, dtype=dtype, endpoint=True)
    b = _clustered_change(rng, a)
    b.reshape(-1)[-1] = a.reshape(-1)[-1] + 1 if dtype != np.float32 else 5.0   # the (possibly short) last piece
    runs, payload = B.sequence_delta_encode(a, b)
    assert 0 < len(runs) <= 6
    _check_format(runs, payload, a, b)
    # identical steps: nothing to send
    runs, payload = B.sequence_delta_encode(a, a.copy())
    assert runs.shape == (0, 3) and payload == b""
    # a step that differs everywhere: every piece, one run, and more than 3/4 of a step (what cpm_sequence_delta_create stores as "full")
    c = (a.view(np.uint8) ^ 0x5A).view(dtype)
    runs, payload = B.sequence_delta_encode(a, c)
    _check_format(runs, payload, a, c)
    assert runs.tolist() == [[0, (a.nbytes + 15) // 16, 0]]
    assert ((12 * len(runs) + 15) // 16) * 16 + len(payload) > 3 * a.nbytes / 4


def test_float_steps_are_compared_bytewise(cpm):
    B = cpm.binding
    a = np.zeros((24, 24, 24), np.float32)
    a.reshape(-1)[100:200] = np.nan
    b = a.copy()
    b.reshape(-1)[5] = -0.0                                                  # -0.0 == +0.0 as floats, not as bytes
    b.reshape(-1)[150] = np.frombuffer(np.uint32(0x7FC00001).tobytes(), np.float32)[0]   # another NaN
    b.reshape(-1)[1000] = np.float32(1e-30)
    runs, payload = B.sequence_delta_encode(a, b)
    _check_format(runs, payload, a, b)
    assert [r[0] for r in runs.tolist()] == [5 * 4 // 16, 150 * 4 // 16, 1000 * 4 // 16]
    assert _apply(a, runs, payload).view(np.uint32)[0, 6, 6] == 0x7FC00001


def test_bad_arguments_are_refused(cpm):
    B = cpm.binding
    with pytest.raises(ValueError):
        B.sequence_delta_encode(np.zeros((4, 4, 4), np.uint8), np.zeros((4, 4, 5), np.uint8))
    lib = B.load_library()
    import ctypes as C
    desc = B.default_volume_desc((4, 4, 4), B.CPM_U8)
    a = np.zeros(64, np.uint8)
    b = a.copy(); b[3] = 1
    n, pay = C.c_uint32(), C.c_size_t()
    runs = np.zeros((1, 3), np.uint32)
    payload = np.zeros(16, np.uint8)
    assert lib.cpm_sequence_delta_encode(C.byref(desc), a.ctypes.data, b.ctypes.data, runs.ctypes.data, payload.ctypes.data, 8,
                                         C.byref(n), C.byref(pay)) != 0          # payload capacity too small
    assert lib.cpm_sequence_delta_encode(C.byref(desc), None, b.ctypes.data, None, None, 0, C.byref(n), C.byref(pay)) != 0


@pytest.mark.parametrize("t", [0, 15])
def test_config5_transitions_match_numpy(cpm, t):
    """BASELINE config 5 (the 32-step 256^3 u8 sequence): the dirty 16-byte pieces of transitions 0 -> 1 and 15 -> 16 are numpy's count, and
    a transition is a fraction of a step."""
    B, S = cpm.binding, cpm.synthetic
    a = S.heterogeneous_volume(256, S.sequence_blob_center(t, 32))
    b = S.heterogeneous_volume(256, S.sequence_blob_center(t + 1, 32))
    runs, payload = B.sequence_delta_encode(a, b)
    changed = _pieces_changed(a, b)
    assert int(runs[:, 1].sum()) == int(changed.sum())
    assert len(payload) == 16 * int(changed.sum())
    assert np.array_equal(_apply(a, runs, payload), b)
    block = ((12 * len(runs) + 15) // 16) * 16 + len(payload)
    assert 0 < block < a.nbytes / 4
