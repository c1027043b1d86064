"""CPM_F16 volumes (include/cpm/cpm.h): every operation on a binary16 volume gives the bits the same operation gives on the F32 volume that
holds the widened values -- where the result is itself a volume (cpm_volume_mix), the f32 result rounded to nearest even.

  * create -> download returns every 16-bit pattern (host and device sources, cpm_volume_update);
  * photons and RNG state of cpm_trace (I = 1 and 4, Henyey-Greenstein, progressive, two-plane records), cpm_trace_lights,
    cpm_trace_emitted, on a shape whose x is not a multiple of 8 and on BASELINE config 2's full shape; the fast-path light volume;
  * min/max, difference and one-pass step bricks at regions 4, 8, 16 and 32 with NaN and +-inf voxels present (NaN compared as NaN);
  * a TF edit and the 31 transitions of a reduced config-5 sequence (importance, selection, re-traced photons; fused and cpm_trace_selected);
  * cpm_volume_mix, then a re-trace through the mixed volume's linear block;
  * resident, streamed and delta-streamed F16 sequences agree."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
LIGHT_DIR = (0.3, 0.5, -1.0)
TFP = [(0.0, 1, 1, 1, 0.0), (0.55, 1, 0.5, 0.2, 0.0), (0.7, 0.6, 0.3, 0.1, 0.3), (1.0, 0.1, 0.6, 0.7, 0.6)]
TFP_EDIT = [(0.0, 1, 1, 1, 0.0), (0.5, 1, 0.5, 0.2, 0.0), (0.75, 0.6, 0.3, 0.1, 0.5), (1.0, 0.1, 0.6, 0.7, 0.6)]


def _n(t):
    return t.detach().cpu().numpy()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _same_or_both_nan(a, b):
    a, b = np.asarray(a), np.asarray(b)
    nan = np.isnan(a)
    return np.array_equal(nan, np.isnan(b)) and np.array_equal(_bits(a[~nan]), _bits(b[~nan]))


def _field(cpm, dims, t=None):
    """A float field in binary16: config-5's blob volume over [0, 1] plus a small ripple, so that the values are not u8 / 255."""
    S = cpm.synthetic
    u8 = S.heterogeneous_volume(dims) if t is None else S.heterogeneous_volume(dims, S.sequence_blob_center(t, 32))
    z, y, x = np.meshgrid(*[np.arange(s, dtype=np.float32) for s in u8.shape], indexing="ij")
    f = u8.astype(np.float32) / np.float32(255.0) + np.float32(0.003) * np.sin(np.float32(0.37) * x + np.float32(0.21) * y + z)
    return np.clip(f, 0, 1).astype(np.float16)


def _wide(h):
    return h.astype(np.float32)


def test_round_trip_of_every_bit_pattern(ctx, cpm):
    h = np.arange(1 << 16, dtype=np.uint32).astype(np.uint16).view(np.float16).reshape(16, 64, 64)
    v = ctx.volume_create(h)
    assert int(v.desc.dtype) == cpm.binding.CPM_F16
    assert np.array_equal(v.download().view(np.uint16), h.view(np.uint16))
    d = ctx.volume_create(ctx.torch.from_numpy(h.copy()).to(ctx.device))       # a device source: copy + footprint in one launch
    assert d.download().dtype == np.float16 and np.array_equal(d.download().view(np.uint16), h.view(np.uint16))
    r = h[:, :, ::-1].copy()
    v.update(r)
    assert np.array_equal(v.download().view(np.uint16), r.view(np.uint16))


@pytest.mark.parametrize("dims,n_side,inter,planar", [((33, 20, 17), 64, 1, False), ((33, 20, 17), 64, 4, False), ((33, 20, 17), 48, 4, True),
                                                     ((48, 40, 32), 100, 1, True)])
def test_trace_photons_and_rng_match_the_widened_f32_volume(ctx, cpm, dims, n_side, inter, planar):
    S, P = cpm.synthetic, cpm.pipeline
    h = _field(cpm, dims)
    out = []
    for vol in (h, _wide(h)):
        fr = P.PhotonFrame(ctx, vol, S.workspace_tf(), n_side, (16, 16, 16), light_travel_direction=LIGHT_DIR, max_interactions=inter,
                           material=(0.3, 0, 0, 0))
        if planar:
            fr.set_planar_records(True)
        fr.trace()
        ctx.torch.cuda.synchronize()
        out.append((_n(fr.photons).copy(), _n(fr.rng).copy()))
    assert _same(out[0][0], out[1][0]) and _same(out[0][1], out[1][1])
    assert (out[0][0][:, 0] < 1e30).any()


def test_progressive_iterations_match(ctx, cpm):
    S, P = cpm.synthetic, cpm.pipeline
    h = _field(cpm, (33, 20, 17))
    res = []
    for vol in (h, _wide(h)):
        pm = P.ProgressivePhotonMapper(ctx, vol, S.workspace_tf(), 64, (16, 16, 16), light_travel_direction=LIGHT_DIR, max_interactions=2,
                                       material=(0.5, 0, 0, 0))
        for _ in range(3):
            pm.iterate()
        ctx.torch.cuda.synchronize()
        res.append((_n(pm.photons).copy(), _n(pm.rng).copy(), _n(pm.light_volume).copy()))
    for a, b in zip(*res):
        assert _same(a, b)


def test_trace_lights_and_emitted_match(ctx, cpm):
    import ctypes as C
    S, P, B = cpm.synthetic, cpm.pipeline, cpm.binding
    torch = ctx.torch
    h = _field(cpm, (33, 20, 17))
    got = []
    for arr in (h, _wide(h)):
        vol = ctx.volume_create(arr)
        tf = ctx.tf_create(S.workspace_tf())
        frames = [P.PhotonFrame(ctx, vol, tf, s, (16, 16, 16), light_travel_direction=d, max_interactions=2, material=(0.3, 0, 0, 0), seed=k)
                  for k, (s, d) in enumerate([(48, (0.3, 0.5, -1.0)), (37, (-0.4, 0.2, -1.0))])]
        ns = [f.n for f in frames]
        spans = ctx.light_spans([(f.light_samples, f.isect, n, off) for f, n, off in zip(frames, ns, [0, ns[0]])])
        rng = torch.cat([f.rng_initial for f in frames]).contiguous()
        params = B.TraceParams()
        C.memmove(C.byref(params), C.byref(frames[0].params), C.sizeof(params))
        params.total_photons = sum(ns)
        ph = torch.full((sum(ns) * 2, 8), -7.0, dtype=torch.float32, device=ctx.device)
        ctx.trace_lights(vol, tf, frames[0].aabb, params, spans, rng, ph)
        em = P.PhotonFrame(ctx, vol, tf, 64, (16, 16, 16), light_travel_direction=LIGHT_DIR, max_interactions=2, emit_in_tracer=True)
        em.trace()
        torch.cuda.synchronize()
        got.append([_n(ph).copy(), _n(rng).copy(), _n(em.photons).copy(), _n(em.rng).copy()])
    for a, b in zip(*got):
        assert _same(a, b)


def test_config2_full_shape_trace_and_fast_light_volume(ctx, cpm):
    """BASELINE config 2: 256^3, 1 048 576 photons, a 128^3 light volume through the brick bin + tile gather."""
    S, P = cpm.synthetic, cpm.pipeline
    h = _field(cpm, 256)
    res = []
    for vol in (h, _wide(h)):
        fr = P.PhotonFrame(ctx, vol, S.workspace_tf(), 1024, (128, 128, 128), light_travel_direction=LIGHT_DIR)
        lv = fr.frame_fast()
        ctx.torch.cuda.synchronize()
        res.append((_n(fr.photons).copy(), _n(fr.rng).copy(), _n(lv).copy()))
        del fr
    for a, b in zip(*res):
        assert _same(a, b)
    assert res[0][2].sum() > 0


def _specials_in(rng, h):
    """h with NaN, +-inf, -0 and subnormal voxels sprinkled in (one brick column of NaNs only)."""
    h = h.copy()
    flat = h.reshape(-1)
    pats = np.array([0x7E00, 0xFE00, 0x7C01, 0x7C00, 0xFC00, 0x8000, 0x0001, 0x83FF], np.uint16).view(np.float16)
    at = rng.choice(flat.size, 60, replace=False)
    flat[at] = pats[np.arange(60) % pats.size]
    h[:4, :4, :4] = np.float16(np.nan)
    return h


@pytest.mark.parametrize("dims", [(64, 48, 40), (33, 20, 17)])
@pytest.mark.parametrize("region", [4, 8, 16, 32])
def test_brick_minmax_difference_and_step(ctx, cpm, dims, region):
    """dx % 8 == 0 takes the streaming kernels (region <= 16: the one-pass step), 33 the per-brick fallback; the F32 reference is the
    per-brick form (minmax_kernel ignores NaN voxels; the difference's double sum), and F16 finite data also matches F32's default path."""
    torch = ctx.torch
    rng = np.random.default_rng(region + dims[0])
    a = _field(cpm, dims)
    b = (a.astype(np.float32) * np.float32(0.9) + np.float32(0.05) * rng.random(a.shape, dtype=np.float32)).astype(np.float16)
    a_s, b_s = _specials_in(rng, a), _specials_in(rng, b)
    a_s[-8:, -8:, -8:], b_s[-8:, -8:, -8:] = a[-8:, -8:, -8:], b[-8:, -8:, -8:]
    b_s[-1, -1, -1] = np.float16(np.inf)                 # (region <= 8: the last brick's only non-finite term -> an inf brick)
    nb = int(np.prod([(d + region - 1) // region for d in dims]))

    def run(x, y, streaming):
        ctx.lib.cpm_debug_set_brick_streaming(ctx.h, int(streaming))
        try:
            vx, vy = ctx.volume_create(x), ctx.volume_create(y)
            mm = torch.zeros((nb, 2), dtype=torch.int16, device=ctx.device)
            diff = torch.zeros(nb, dtype=torch.float32, device=ctx.device)
            smm = torch.zeros((nb, 2), dtype=torch.int16, device=ctx.device)
            sdiff = torch.zeros(nb, dtype=torch.float32, device=ctx.device)
            ctx.volume_minmax(vx, region, mm)
            ctx.volume_difference(vx, vy, region, diff)
            ctx.volume_step(vx, vy, region, sdiff, smm)
            torch.cuda.synchronize()
            return [_n(mm).copy(), _n(diff).copy(), _n(sdiff).copy(), _n(smm).copy()]
        finally:
            ctx.lib.cpm_debug_set_brick_streaming(ctx.h, 1)

    for x, y in ((a, b), (a_s, b_s)):
        f16 = run(x, y, True)
        ref = run(_wide(x), _wide(y), False)
        per_brick = run(x, y, False)
        for got in (f16, per_brick):
            assert _same(got[0], ref[0]) and _same(got[3], ref[3])
            assert _same_or_both_nan(got[1], ref[1]) and _same_or_both_nan(got[2], ref[2])
        if x is a_s:
            assert np.isnan(f16[1]).any() and (region > 8 or np.isinf(f16[1]).any())
        else:
            default = run(_wide(x), _wide(y), True)
            assert all(_same(g, d) for g, d in zip(f16, default))


def _mappers(ctx, cpm, h, n_side=128, grid=(32, 32, 32), **kw):
    S, P = cpm.synthetic, cpm.pipeline
    out = []
    for vol in (h, _wide(h)):
        cm = P.CorrelatedPhotonMapper(ctx, vol, S.tf_from_points(TFP), n_side, grid, light_travel_direction=LIGHT_DIR, tf_points=TFP,
                                      incremental_threshold_percent=100.0, **kw)
        cm.full_frame()
        out.append(cm)
    return out


def _state(cm, n):
    return [_n(cm.importance_grid).copy(), np.sort(_n(cm.indices)[:n]), _n(cm.photons).copy(), _n(cm.rng).copy()]


@pytest.mark.parametrize("fused", [True, False])
def test_tf_edit_matches(ctx, cpm, fused):
    """BASELINE config 3 at reduced size: a TF edit's importance, selection and re-traced photons (fused: importance_retrace_kernel;
    otherwise cpm_trace_selected)."""
    S = cpm.synthetic
    pair = _mappers(ctx, cpm, _field(cpm, 64))
    res = []
    for cm in pair:
        cm.fused = fused
        cm.set_transfer_function(TFP_EDIT)
        n = cm.correlated_update()
        ctx.torch.cuda.synchronize()
        res.append((n, _state(cm, n)))
    assert res[0][0] == res[1][0] > 0
    for a, b in zip(res[0][1], res[1][1]):
        assert _same(a, b)


def test_sequence_transitions_match(ctx, cpm):
    """BASELINE config 5 reduced to 64^3: all 31 transitions of the 32-step moving blob."""
    steps = [_field(cpm, 64, t) for t in range(32)]
    pair = _mappers(ctx, cpm, steps[0])
    total = 0
    for t in range(1, 32):
        res = []
        for cm, wide in zip(pair, (False, True)):
            cm.set_volume(_wide(steps[t]) if wide else steps[t])
            n = cm.correlated_update()
            ctx.torch.cuda.synchronize()
            res.append((n, _state(cm, n)))
        assert res[0][0] == res[1][0], t
        total += res[0][0]
        for a, b in zip(res[0][1], res[1][1]):
            assert _same(a, b), t
    assert total > 0


def test_mix_rounds_the_f32_mix_and_retraces_through_it(ctx, cpm):
    a, b = _field(cpm, 64, 0), _field(cpm, 64, 9)
    mixed = []
    for x, y in ((a, b), (_wide(a), _wide(b))):
        out = ctx.volume_create(np.zeros_like(x))
        ctx.volume_mix(ctx.volume_create(x), ctx.volume_create(y), 0.37, out)
        mixed.append(out)
    m16, m32 = mixed[0].download(), mixed[1].download()
    assert m16.dtype == np.float16 and np.array_equal(m16.view(np.uint16), m32.astype(np.float16).view(np.uint16))
    # the F16 mix's footprint copy is stale: its correlated re-trace reads the linear block (LinearLoad<CPM_F16>); the twin is the F32
    # volume of the rounded mix's widened values
    pair = _mappers(ctx, cpm, a)
    res = []
    for cm, vol in zip(pair, (mixed[0], ctx.volume_create(_wide(m16)))):
        cm.set_volume(vol)
        n = cm.correlated_update()
        ctx.torch.cuda.synchronize()
        res.append((n, _state(cm, n)))
    assert res[0][0] == res[1][0] > 0
    for x, y in zip(res[0][1], res[1][1]):
        assert _same(x, y)


def test_resident_streamed_and_delta_streamed_sequences_agree(ctx, cpm):
    B, P, S = cpm.binding, cpm.pipeline, cpm.synthetic
    steps = [_field(cpm, (40, 24, 24), t * 3) for t in range(8)]
    steps[5] = _specials_in(np.random.default_rng(5), steps[5])
    seq = B.PinnedSequence(ctx, steps)

    def photons(v):
        fr = P.PhotonFrame(ctx, v, S.workspace_tf(), 48, (16, 16, 16), light_travel_direction=LIGHT_DIR)
        fr.trace()
        ctx.torch.cuda.synchronize()
        return _n(fr.photons).copy()

    resident = [ctx.volume_create(s) for s in steps]
    full, changes = B.VolumeStream(ctx, steps[0], n_slots=3), B.VolumeStream(ctx, steps[0], n_slots=3)
    delta = B.SequenceDelta(ctx, seq, wrap=True)
    changes.use_delta(delta)
    walk = list(range(8)) + [0, 1]
    for i, t in enumerate(walk):
        for vs in (full, changes):
            vs.prefetch(t, seq.steps[t])
        got = [vs.acquire(t) for vs in (full, changes)]
        for v in got:
            assert np.array_equal(v.download().view(np.uint16), steps[t].view(np.uint16)), (i, t)
        if t != 5:
            want = photons(resident[t])
            for v in got:
                assert _same(photons(v), want), (i, t)
    ctx.torch.cuda.synchronize()
    assert changes.delta_stats().delta_uploads > 0
