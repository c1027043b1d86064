"""VolumeSequencePlayer's uploadChangesOnly (this build's property, like keepSequenceOnDevice): a sequence kept in host memory is compared
once and an element whose predecessor is in the player's ring crosses PCIe as the pieces that changed (cpm_sequence_delta).  Three players
of one sequence -- resident, streamed, streamed with changes only -- show the same volume, min/max grid and difference grid, bit for bit,
at every displayed time forth and back across the wrap."""
import ctypes as C

import numpy as np
import pytest

from test_host_layer_gpu import host, host_extras  # noqa: F401  (fixtures: build and load libcpm_host after torch's HIP runtime)
from test_timevarying_host_gpu import _sequence, seqlib  # noqa: F401

pytestmark = pytest.mark.gpu


def test_a_sequence_uploading_changes_only_plays_the_same_volumes(seqlib, ctx, cpm):
    dim, steps, region = 32, 6, 8
    vols = _sequence(cpm, dim, steps)
    for name, res, args in [("cpmh_sequence_keep_on_device", None, [C.c_void_p, C.c_int]),
                            ("cpmh_sequence_upload_changes_only", None, [C.c_void_p, C.c_int]),
                            ("cpmh_sequence_stream_stats", C.c_int, [C.c_void_p, C.c_void_p]),
                            ("cpmh_sequence_delta_stats", C.c_int, [C.c_void_p, C.c_void_p])]:
        f = getattr(seqlib, name)
        f.restype, f.argtypes = res, args
    players = [seqlib.cpmh_sequence_create(vols.ctypes.data, 0, dim, dim, dim, steps, region) for _ in range(3)]
    resident, streamed, changes = players
    seqlib.cpmh_sequence_keep_on_device(streamed, 0)
    seqlib.cpmh_sequence_keep_on_device(changes, 0)
    seqlib.cpmh_sequence_upload_changes_only(changes, 1)
    stats = (C.c_double * 4)()
    assert seqlib.cpmh_sequence_delta_stats(resident, stats) == -1
    times = [0.0, 0.25, 0.5, 1.0, 1.75, 2.0, 2.5, 3.0, 3.5, 4.0, 4.9, 5.0, 5.5, 0.0, 0.5, 1.0, 0.0, 5.0, 4.5, 3.25, 2.0, 1.0, 0.0]
    for time in times:
        for h in players:
            seqlib.cpmh_sequence_evaluate(h)
            seqlib.cpmh_sequence_set_time(h, time)
            assert seqlib.cpmh_sequence_evaluate(h) == 0
        got = [np.empty_like(vols[0]) for _ in players]
        for h, g in zip(players, got):
            assert seqlib.cpmh_sequence_download(h, 0, g.ctypes.data) == 0
        assert np.array_equal(got[0], got[1]) and np.array_equal(got[0], got[2]), time
        for kind, dt, shape in ((1, np.uint16, ((dim // region) ** 3, 2)), (2, np.float32, ((dim // region) ** 3,))):
            gs = [np.empty(shape, dt) for _ in players]
            for h, g in zip(players, gs):
                assert seqlib.cpmh_sequence_download(h, kind, g.ctypes.data) == 0
            assert np.array_equal(gs[0].view(np.uint8), gs[1].view(np.uint8)) and np.array_equal(gs[0].view(np.uint8), gs[2].view(np.uint8)), (time, kind)
    ctx.torch.cuda.synchronize()
    assert seqlib.cpmh_sequence_delta_stats(streamed, stats) == -1        # streamed in full: no delta in use
    assert seqlib.cpmh_sequence_delta_stats(changes, stats) == 0
    delta_uploads, full_uploads, delta_bytes, analysis_ms = int(stats[0]), int(stats[1]), int(stats[2]), float(stats[3])
    assert delta_uploads > 0 and full_uploads >= 2 and analysis_ms > 0
    assert 0 < delta_bytes < delta_uploads * dim ** 3 * 3 // 4
    s_full, s_changes = (C.c_double * 4)(), (C.c_double * 4)()
    assert seqlib.cpmh_sequence_stream_stats(streamed, s_full) == 0 and seqlib.cpmh_sequence_stream_stats(changes, s_changes) == 0
    assert int(s_changes[0]) == delta_uploads + full_uploads          # every upload of the changes-only player, timed
    for h in players:
        seqlib.cpmh_sequence_destroy(h)
