"""Delta uploads of a streamed sequence (include/cpm/cpm_ext.h, cpm_sequence_delta + cpm_volume_stream_use_delta): a step whose predecessor
is resident in the ring crosses PCIe as the pieces that changed, patched on the device into a copy of the predecessor.

  * small sequences (u8 / u16 / f32, rows that are not a multiple of 16 bytes, sparse clustered changes, an identical transition and one that
    changes everything): every acquired slot holds its step and the tracer's footprint copy of it (photons bit for bit those of a
    cpm_volume_create'd volume); the first step and the fully changed transition upload in full, every other one as a delta; the bytes
    that crossed PCIe are the transitions' blocks plus the full steps;
  * the fallbacks -- backwards, a jump, an evicted step again, a 2-slot ring -- give the same bits as full uploads;
  * BASELINE config 5 at full size, delta-streamed against resident over all 31 transitions and the wrap 31 -> 0: the same re-traced
    indices, importance grid and photons, the light volume within the add-remove splat's tolerance after an update and the same bits
    after a full frame; every step after the first is a delta."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
LIGHT_DIR = (0.3, 0.5, -1.0)


def _n(t, dtype=None):
    a = t.detach().cpu().numpy()
    return a.view(dtype) if dtype is not None else a


def _sequence(dtype, dims, n=8, seed=0):
    """steps[t + 1] = steps[t] with a few clustered changes, except: 2 -> 3 identical, 5 -> 6 everything new."""
    rng = np.random.default_rng(seed + dims[0])
    shape = dims[::-1]

    def fresh():
        if dtype == np.float32:
            return rng.random(shape, dtype=np.float32)
        return rng.integers(0, np.iinfo(dtype).max, shape, dtype=dtype, endpoint=True)
    steps = [fresh()]
    for t in range(1, n):
        if t == 3:
            steps.append(steps[-1].copy())
            continue
        if t == 6:
            steps.append(fresh())
            continue
        b = steps[-1].copy()
        flat = b.reshape(-1)
        for _ in range(4):
            at = int(rng.integers(0, flat.size - 64))
            k = int(rng.integers(1, 64))
            flat[at:at + k] = fresh().reshape(-1)[:k] if dtype != np.float32 else rng.random(k, dtype=np.float32) + 1.0
        steps.append(b)
    return steps


def _photons(ctx, cpm, vol):
    P, S = cpm.pipeline, cpm.synthetic
    fr = P.PhotonFrame(ctx, vol, S.workspace_tf(), 64, (16, 16, 16), light_travel_direction=LIGHT_DIR)
    fr.trace()
    ctx.torch.cuda.synchronize()
    return _n(fr.photons).copy().view(np.uint32)


@pytest.mark.parametrize("dtype,dims", [(np.uint8, (37, 20, 11)), (np.uint16, (33, 17, 9)), (np.float32, (23, 24, 24))])
def test_forward_walk_uploads_the_changes(ctx, cpm, dtype, dims):
    B = cpm.binding
    steps = _sequence(dtype, dims)
    n = len(steps)
    seq = B.PinnedSequence(ctx, steps)
    delta = B.SequenceDelta(ctx, seq, wrap=True)
    info = delta.info()
    assert (info.n_steps, info.n_transitions, info.wrap, info.step_bytes) == (n, n, 1, steps[0].nbytes)
    assert delta.transition(2, 3) == (0, 0)                       # identical: nothing to send, still a delta
    assert delta.transition(5, 6) == (0, steps[0].nbytes)         # everything changed: full
    assert delta.transition(n - 1, 0) == (0, steps[0].nbytes)     # the wrap lands on an unrelated step
    with pytest.raises(B.CpmError):
        delta.transition(3, 2)                                    # forward deltas only
    full = {t for t in range(n) if delta.transition(t, (t + 1) % n) == (0, steps[0].nbytes)}
    assert full == {5, n - 1}
    assert info.n_delta_transitions == n - 2 and 0 < info.dirty_fraction < 1 and info.analysis_ms > 0
    for t in range(n):
        if t not in full and t != 2:
            r, nb = delta.transition(t, t + 1)
            assert r > 0 and 0 < nb < steps[0].nbytes * 3 // 4
    walk = list(range(n)) + [0, 1]                                # across the wrap: 7 -> 0 in full, 0 -> 1 as a delta again
    sent = steps[0].nbytes + sum(delta.transition(a, b)[1] for a, b in zip(walk, walk[1:]))
    vs = B.VolumeStream(ctx, steps[0], n_slots=3)
    vs.use_delta(delta)
    delta.close()                                                 # the stream keeps its own reference
    vs.prefetch(walk[0], seq.steps[walk[0]])
    for i, t in enumerate(walk):
        if i + 1 < len(walk):
            vs.prefetch(walk[i + 1], seq.steps[walk[i + 1]])
        v = vs.acquire(t)
        assert np.array_equal(v.download(), steps[t]), (i, t)
        if dtype != np.float32 or i < 3 or t == 4:
            assert np.array_equal(_photons(ctx, cpm, v), _photons(ctx, cpm, ctx.volume_create(steps[t]))), (i, t)
    ctx.torch.cuda.synchronize()
    st, ds = vs.stats(), vs.delta_stats()
    # full: the first step, 5 -> 6, 7 -> 0; every other step a delta
    assert (ds.full_uploads, ds.delta_uploads) == (3, len(walk) - 3)
    assert st.uploads == len(walk) and st.hits == len(walk) and st.uploads_at_acquire == 0
    assert ds.delta_bytes + ds.full_bytes == st.bytes_uploaded == sent
    assert ds.full_bytes == 3 * steps[0].nbytes
    assert ds.delta_uploads_timed == ds.delta_uploads and ds.delta_h2d_ms_total >= 0 and st.uploads_timed == len(walk)
    vs.close(); seq.close()


@pytest.mark.parametrize("dtype,dims", [(np.uint8, (37, 20, 11)), (np.float32, (23, 24, 24))])
def test_fallbacks_give_the_bits_of_full_uploads(ctx, cpm, dtype, dims):
    B = cpm.binding
    steps = _sequence(dtype, dims, n=10, seed=1)
    n = len(steps)
    seq = B.PinnedSequence(ctx, steps)
    delta = B.SequenceDelta(ctx, seq, wrap=False)

    def ring(n_slots):
        vs = B.VolumeStream(ctx, steps[0], n_slots=n_slots)
        vs.use_delta(delta)
        return vs

    def check(v, t, photons=False):
        assert np.array_equal(v.download(), steps[t]), t
        if photons:
            assert np.array_equal(_photons(ctx, cpm, v), _photons(ctx, cpm, ctx.volume_create(steps[t]))), t

    # backwards: no reverse deltas -- every step in full
    vs = ring(3)
    vs.prefetch(n - 1, seq.steps[n - 1])
    for t in range(n - 1, -1, -1):
        if t > 0:
            vs.prefetch(t - 1, seq.steps[t - 1])
        check(vs.acquire(t), t, photons=t in (n - 1, 4))
    ds = vs.delta_stats()
    assert (ds.delta_uploads, ds.full_uploads) == (0, n)
    vs.close()

    # a jump (0 -> 5: step 4 is not resident), an evicted step again, then the walk goes on from it with deltas
    vs = ring(3)
    check(vs.acquire(0, seq.steps[0]), 0)
    check(vs.acquire(5, seq.steps[5]), 5, photons=True)
    assert vs.delta_stats().delta_uploads == 0
    check(vs.acquire(1, seq.steps[1]), 1, photons=True)      # base 0 still resident: a delta
    check(vs.acquire(8, seq.steps[8]), 8)                     # jump: full; evicts step 0
    check(vs.acquire(0, seq.steps[0]), 0, photons=True)      # evicted, and the first step: full
    check(vs.acquire(1), 1)                                   # (still resident)
    check(vs.acquire(2, seq.steps[2]), 2, photons=True)      # 1 -> 2: a delta
    ds = vs.delta_stats()
    assert (ds.delta_uploads, ds.full_uploads) == (2, 4) and vs.stats().hits == 1
    vs.close()

    # a 2-slot ring: prefetching t + 1 before acquiring t leaves only the base as the victim -- full uploads; acquiring one step after the
    # other, the victim is the step before the base -- deltas (5 -> 6 changes everything: full)
    vs = ring(2)
    vs.prefetch(0, seq.steps[0])
    for t in range(n):
        if t + 1 < n:
            vs.prefetch(t + 1, seq.steps[t + 1])
        check(vs.acquire(t, seq.steps[t]), t, photons=t in (2, 7))
    vs.close()
    vs = ring(2)
    for t in range(n):
        check(vs.acquire(t, seq.steps[t]), t, photons=t in (2, 7))
    ds = vs.delta_stats()
    assert (ds.full_uploads, ds.delta_uploads) == (2, n - 2)
    vs.close()
    # a stream that has uploaded already, or of another shape, refuses the delta
    vs = B.VolumeStream(ctx, steps[0], n_slots=3)
    vs.acquire(0, seq.steps[0])
    with pytest.raises(B.CpmError):
        vs.use_delta(delta)
    vs.close()
    other = B.VolumeStream(ctx, np.zeros((4, 4, 4), steps[0].dtype), n_slots=3)
    with pytest.raises(B.CpmError):
        other.use_delta(delta)
    other.close(); delta.close(); seq.close()


@pytest.mark.parametrize("steps", [list(range(0, 12)), list(range(11, 22)), list(range(21, 32)) + [0]])   # 31 transitions and the wrap
def test_config5_delta_streamed_equals_resident(ctx, cpm, steps):
    B, S, P = cpm.binding, cpm.synthetic, cpm.pipeline
    torch = ctx.torch
    vdim, gdim, n_side, region = 256, 128, 1024, 8
    tfp = list(S.WORKSPACE_TF_POINTS)
    vols = [S.heterogeneous_volume(vdim, S.sequence_blob_center(t, 32)) for t in steps]
    resident = [ctx.volume_create(v) for v in vols]
    seq = B.PinnedSequence(ctx, vols)
    delta = B.SequenceDelta(ctx, seq, wrap=False)     # (tags: positions in this list; its last transition is 31 -> 0 for the third part)
    assert delta.info().n_delta_transitions == len(steps) - 1
    vs = B.VolumeStream(ctx, vols[0], n_slots=3)
    vs.use_delta(delta)

    def mapper():
        cm = P.CorrelatedPhotonMapper(ctx, vols[0], S.tf_from_points(tfp), n_side, (gdim,) * 3, light_travel_direction=LIGHT_DIR,
                                      tf_points=tfp, incremental_threshold_percent=100.0, region=region)
        cm.full_frame()
        return cm
    a, b = mapper(), mapper()
    vs.prefetch(0, seq.steps[0])
    vs.prefetch(1, seq.steps[1])
    for t in range(1, len(steps)):
        if t + 1 < len(steps):
            vs.prefetch(t + 1, seq.steps[t + 1])      # crosses PCIe (as a delta) while step t is computed
        b.set_volume(vs.acquire(t))
        nb = b.correlated_update()
        a.set_volume(resident[t])
        na = a.correlated_update()
        torch.cuda.synchronize()
        assert na == nb and 0 < na < a.n
        assert np.array_equal(np.sort(_n(a.indices, np.uint32)[:na]), np.sort(_n(b.indices, np.uint32)[:nb])), t
        assert np.array_equal(_n(a.photons, np.uint32), _n(b.photons, np.uint32)), t
        assert np.array_equal(_n(a.importance_grid, np.uint32), _n(b.importance_grid, np.uint32)), t
        # the add-remove splat's float atomics add in arrival order: its stated tolerance after an update ...
        la, lb = _n(a.light_volume), _n(b.light_volume)
        assert np.allclose(la, lb, rtol=1e-3, atol=2e-5 * float(la.max())), t
        if t % 4 == 0 or t == len(steps) - 1:
            # ... and the same bits after a full frame on the current volumes (every photon through the slot's footprint copy)
            a.full_frame(); b.full_frame()
            torch.cuda.synchronize()
            assert np.array_equal(_n(a.photons, np.uint32), _n(b.photons, np.uint32)), t
            assert np.array_equal(_n(a.light_volume, np.uint32), _n(b.light_volume, np.uint32)), t
    ds = vs.delta_stats()
    assert (ds.full_uploads, ds.delta_uploads) == (1, len(steps) - 1)
    assert ds.delta_bytes < (len(steps) - 1) * vols[0].nbytes // 4
    assert vs.stats().uploads_at_acquire == 0
    vs.close(); delta.close(); seq.close()
