"""INT16 volumes through the C++ processors (host/, cpmh_* facade): an INT16 network and its FLOAT32 twin, which holds w(v) under the
INT16 default mapping (formatOffset 1, formatScaling 0.5), show the same light volume and photons after a full frame and the same
photons after a TF edit; an INT16 VolumeSequencePlayer shows the same volumes, min/max grids and difference grids whether the sequence is
kept on the device or streamed from host memory (whole steps, or changes only)."""
import ctypes as C

import numpy as np
import pytest

from test_host_layer_gpu import host  # noqa: F401  (fixture: build and load libcpm_host after torch's HIP runtime)
from test_timevarying_host_gpu import seqlib  # noqa: F401
from test_i16_cpu import SPECIALS, widen

pytestmark = pytest.mark.gpu
TFP = [(0.0, 1, 1, 1, 0.0), (0.55, 1, 0.5, 0.2, 0.0), (0.7, 0.6, 0.3, 0.1, 0.3), (1.0, 0.1, 0.6, 0.7, 0.6)]
TFP_EDIT = [(0.0, 1, 1, 1, 0.0), (0.5, 1, 0.5, 0.2, 0.0), (0.75, 0.6, 0.3, 0.1, 0.5), (1.0, 0.1, 0.6, 0.7, 0.6)]


def _field(cpm, dim, t, steps):
    S = cpm.synthetic
    u8 = S.heterogeneous_volume(dim, S.sequence_blob_center(t, steps))
    rng = np.random.default_rng(100 + t)
    v = (u8.astype(np.float64) / 255.0 * 2.0 - 1.0) * 32000.0 + rng.integers(-60, 61, u8.shape)
    v = np.clip(np.rint(v), -32768, 32767).astype(np.int16)
    v.reshape(-1)[rng.choice(v.size, 2 * SPECIALS.size, replace=False)] = np.tile(SPECIALS, 2)
    return v


def _light_volume(lib, h):
    dims, ch = (C.c_int * 3)(), C.c_int()
    lib.cpmh_light_volume_dims(h, C.byref(dims), C.byref(ch))
    out = np.zeros(dims[0] * dims[1] * dims[2] * ch.value, np.float32)
    assert lib.cpmh_download_light_volume(h, out.ctypes.data) == 0
    return out


def _photons(lib, h):
    out = np.zeros((lib.cpmh_n_photons(h), 8), np.float32)
    assert lib.cpmh_download_photons(h, out.ctypes.data) == 0
    return out


def test_int16_network_matches_its_float32_twin(host, cpm):
    B = cpm.binding
    host.cpmh_set_volume_format_mapping.restype = C.c_int
    host.cpmh_set_volume_format_mapping.argtypes = [C.c_void_p, C.c_float, C.c_float]
    v16 = _field(cpm, 32, 3, 8)
    nets = []
    for vol, code in ((v16, B.CPM_I16), (widen(v16), B.CPM_F32)):
        vol = np.ascontiguousarray(vol)
        pts = np.ascontiguousarray(np.asarray(TFP, np.float32))
        h = host.cpmh_create(vol.ctypes.data, code, vol.shape[2], vol.shape[1], vol.shape[0], 96, 96,
                             C.byref((C.c_float * 3)(0.3, 0.5, 2.0)), C.byref((C.c_float * 3)(-0.3, -0.5, -1.0)), pts.ctypes.data,
                             pts.shape[0], 2, 1, 1)
        assert h
        nets.append(h)
    assert host.cpmh_set_volume_format_mapping(nets[1], 1.0, 0.5) == 0          # the twin: INT16's default pair on FLOAT32 data
    try:
        for h in nets:
            assert host.cpmh_evaluate(h, 1) == 0
        lv = [_light_volume(host, h) for h in nets]
        assert lv[0].sum() > 0 and np.array_equal(lv[0].view(np.uint32), lv[1].view(np.uint32))
        ph = [_photons(host, h) for h in nets]
        assert (ph[0][:, 0] < 1e30).any() and np.array_equal(ph[0].view(np.uint32), ph[1].view(np.uint32))
        pts = np.ascontiguousarray(np.asarray(TFP_EDIT, np.float32))
        for h in nets:
            host.cpmh_set_transfer_function(h, pts.ctypes.data, pts.shape[0])
            assert host.cpmh_evaluate(h, 0) == 0
        assert host.cpmh_n_recomputed(nets[0]) == host.cpmh_n_recomputed(nets[1]) > 0
        assert np.array_equal(_photons(host, nets[0]).view(np.uint32), _photons(host, nets[1]).view(np.uint32))
    finally:
        for h in nets:
            host.cpmh_destroy(h)


def test_int16_player_shows_the_same_volumes_on_the_device_and_from_host_memory(seqlib, ctx, cpm):
    B = cpm.binding
    dim, steps, region = 32, 4, 8
    vols = np.stack([_field(cpm, dim, t, steps) for t in range(steps)])
    for name, res, args in [("cpmh_sequence_keep_on_device", None, [C.c_void_p, C.c_int]),
                            ("cpmh_sequence_upload_changes_only", None, [C.c_void_p, C.c_int])]:
        f = getattr(seqlib, name)
        f.restype, f.argtypes = res, args
    players = [seqlib.cpmh_sequence_create(vols.ctypes.data, B.CPM_I16, dim, dim, dim, steps, region) for _ in range(3)]
    assert all(players)
    resident, streamed, changes = players
    seqlib.cpmh_sequence_keep_on_device(streamed, 0)
    seqlib.cpmh_sequence_keep_on_device(changes, 0)
    seqlib.cpmh_sequence_upload_changes_only(changes, 1)
    try:
        for time in [0.0, 1.0, 1.5, 2.0, 3.0, 0.0, 2.25]:
            for h in players:
                seqlib.cpmh_sequence_evaluate(h)
                seqlib.cpmh_sequence_set_time(h, time)
                assert seqlib.cpmh_sequence_evaluate(h) == 0
            got = [np.empty_like(vols[0]) for _ in players]
            for h, g in zip(players, got):
                assert seqlib.cpmh_sequence_download(h, 0, g.ctypes.data) == 0
            assert np.array_equal(got[0], got[1]) and np.array_equal(got[0], got[2]), time
            if time == int(time):   # the player's output is a cpm_volume_mix at weight 0: w(-32768) = -1 is written as -32767
                assert np.array_equal(got[0], np.maximum(vols[int(time)], -32767)), time
            else:
                assert not any(np.array_equal(got[0], v) for v in vols), time
            for kind, dt, shape in ((1, np.uint16, ((dim // region) ** 3, 2)), (2, np.float32, ((dim // region) ** 3,))):
                gs = [np.empty(shape, dt) for _ in players]
                for h, g in zip(players, gs):
                    assert seqlib.cpmh_sequence_download(h, kind, g.ctypes.data) == 0
                assert np.array_equal(gs[0].view(np.uint8), gs[1].view(np.uint8)) and np.array_equal(gs[0].view(np.uint8), gs[2].view(np.uint8))
    finally:
        for h in players:
            seqlib.cpmh_sequence_destroy(h)
