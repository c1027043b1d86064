"""CPM_I16 volumes (include/cpm/cpm.h): every operation on an int16 (SNORM) volume gives the bits the same operation gives on the F32
volume that holds w(v) = max(v, -32767) * fl32(1 / 32767) under the same format_offset / format_scaling -- where the result is itself a
volume (cpm_volume_mix), the f32 mix converted by (int16) rint(clamp(m, -1, 1) * 32767).  Every comparison is on bits but one.

  * create -> download returns all 65536 codes (host and device sources, cpm_volume_update);
  * photons and RNG states of cpm_trace (I = 1 and 3, AoS and two-plane records), cpm_trace_lights, cpm_trace_emitted (directional and
    point), progressive iterations -- under the default mapping and a CT-style offset / scaling pair;
  * min/max, difference and step bricks (with and without the streaming kernels the other types take);
  * a TF edit (fused: importance_retrace_kernel; unfused: cpm_trace_selected) and a 3-step sequence: importance grids, selections,
    photons; the light volume after a full frame;
  * cpm_volume_mix at four weights, then a re-trace through the mixed volume's linear block;
  * resident, streamed and delta-streamed sequences; the raycaster, plain, with an accel and shaded; the refusals.

The one tolerance: the light volume after an INCREMENTAL update is a sum of atomic - old / + new splats whose order differs from run to
run.  tests/test_f16_volume_gpu.py does not compare that light volume and so holds no constant for it; the constant used here is the
suite's own for that step (tests/test_correlated_gpu.py, test_correlated_fused_gpu.py: rtol 1e-3, atol 2e-5 max)."""
import numpy as np
import pytest

from test_i16_cpu import SPECIALS, snorm_write, widen
from test_render_gpu import light_volume, matrix

pytestmark = pytest.mark.gpu
F32 = np.float32
LIGHT_DIR = (0.3, 0.5, -1.0)
TFP = [(0.0, 1, 1, 1, 0.0), (0.55, 1, 0.5, 0.2, 0.0), (0.7, 0.6, 0.3, 0.1, 0.3), (1.0, 0.1, 0.6, 0.7, 0.6)]
TFP_EDIT = [(0.0, 1, 1, 1, 0.0), (0.5, 1, 0.5, 0.2, 0.0), (0.75, 0.6, 0.3, 0.1, 0.5), (1.0, 0.1, 0.6, 0.7, 0.6)]
# (format_offset, format_scaling): cpm_volume_desc_default's pair, and CT's -1024..3071 onto [0, 1]
MAPPINGS = {"default": (1.0, 0.5), "ct": (1024.0 / 32767.0, 1.0 - 32767.0 / 4095.0)}
SPLAT_TOL = dict(rtol=1e-3)   # + atol 2e-5 * max (see the module docstring)


def _n(t):
    return t.detach().cpu().numpy()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _field(cpm, dims, t=None, mapping="default", seed=0):
    """config 5's blob volume (step t of 32) as int16 -- over the whole range, or over CT's -1024..3071 -- plus seeded noise, with
    -32768, -32767, -1, 0, 1 and 32767 planted at seeded places"""
    S = cpm.synthetic
    u8 = S.heterogeneous_volume(dims) if t is None else S.heterogeneous_volume(dims, S.sequence_blob_center(t, 32))
    noise = np.random.default_rng(1000 * seed + sum(u8.shape))           # (the same at every step: a sequence changes where the blob moves)
    rng = np.random.default_rng(1000 * seed + (0 if t is None else t + 1) + sum(u8.shape))
    f = u8.astype(np.float64) / 255.0
    if mapping == "ct":
        v = f * 4095.0 - 1024.0 + noise.integers(-3, 4, u8.shape)
    else:
        v = (f * 2.0 - 1.0) * 32000.0 + noise.integers(-60, 61, u8.shape)
    v = np.clip(np.rint(v), -32768, 32767).astype(np.int16)
    flat = v.reshape(-1)
    at = rng.choice(flat.size, 4 * SPECIALS.size, replace=False)
    flat[at] = np.tile(SPECIALS, 4)
    assert set(SPECIALS.tolist()) <= set(flat.tolist())
    return v


def _volumes(ctx, cpm, v, mapping="default"):
    """(the I16 volume of v, the F32 volume of w(v)) under one format_offset / format_scaling"""
    B = cpm.binding
    out = []
    for arr, code in ((v, B.CPM_I16), (widen(v), B.CPM_F32)):
        d = B.default_volume_desc(arr.shape[::-1], code)
        d.format_offset, d.format_scaling = MAPPINGS[mapping]
        out.append(ctx.volume_create(arr, d))
    assert int(out[0].desc.dtype) == B.CPM_I16 and int(out[1].desc.dtype) == B.CPM_F32
    return out


def test_round_trip_of_every_code(ctx, cpm):
    B = cpm.binding
    dims = (40, 41, 40)
    h = np.zeros(dims[::-1], np.int16)
    h.reshape(-1)[:1 << 16] = np.arange(-32768, 32768, dtype=np.int32).astype(np.int16)
    v = ctx.volume_create(h)
    assert int(v.desc.dtype) == B.CPM_I16 and v.desc.format_offset == 1.0 and v.desc.format_scaling == 0.5
    got = v.download()
    assert got.dtype == np.int16 and np.array_equal(got, h)
    t = ctx.torch.from_numpy(h.copy()).to(ctx.device)
    d = ctx.volume_create(t, dtype=B.CPM_I16)                 # a device source: copy + footprint in one launch
    assert int(d.desc.dtype) == B.CPM_I16 and d.download().dtype == np.int16 and np.array_equal(d.download(), h)
    u = ctx.volume_create(t)                                  # without the keyword a torch int16 tensor is u16, as before
    assert int(u.desc.dtype) == B.CPM_U16 and u.desc.format_offset == 0.0 and u.download().dtype == np.uint16
    assert np.array_equal(u.download(), h.view(np.uint16))
    with pytest.raises(ValueError):
        ctx.volume_create(t.to(ctx.torch.float32), dtype=B.CPM_I16)
    r = h[:, :, ::-1].copy()
    v.update(r)
    assert np.array_equal(v.download(), r)


@pytest.mark.parametrize("mapping", ["default", "ct"])
@pytest.mark.parametrize("planar", [False, True])
@pytest.mark.parametrize("dims", [(7, 9, 11), (32, 32, 32)])
def test_trace_photons_and_rng_match_the_widened_f32_volume(ctx, cpm, dims, planar, mapping):
    S, P = cpm.synthetic, cpm.pipeline
    pair = _volumes(ctx, cpm, _field(cpm, dims, mapping=mapping), mapping)
    tf = ctx.tf_create(S.workspace_tf())
    for n_side in (32, 64):
        for inter in (1, 3):
            out = []
            for vol in pair:
                fr = P.PhotonFrame(ctx, vol, tf, n_side, (16, 16, 16), light_travel_direction=LIGHT_DIR, max_interactions=inter,
                                   material=(0.3, 0, 0, 0))
                if planar:
                    fr.set_planar_records(True)
                fr.trace()
                ctx.torch.cuda.synchronize()
                out.append((_n(fr.photons).copy(), _n(fr.rng).copy()))
            assert _same(out[0][0], out[1][0]) and _same(out[0][1], out[1][1]), (n_side, inter)
            assert (out[0][0][:, 0] < 1e30).any(), (n_side, inter)


def test_progressive_iterations_match(ctx, cpm):
    S, P = cpm.synthetic, cpm.pipeline
    res = []
    for vol in _volumes(ctx, cpm, _field(cpm, (32, 32, 32))):
        pm = P.ProgressivePhotonMapper(ctx, vol, S.workspace_tf(), 64, (16, 16, 16), light_travel_direction=LIGHT_DIR, max_interactions=2,
                                       material=(0.5, 0, 0, 0))
        for _ in range(2):
            pm.iterate()
        ctx.torch.cuda.synchronize()
        res.append((_n(pm.photons).copy(), _n(pm.rng).copy(), _n(pm.light_volume).copy()))
    for a, b in zip(*res):
        assert _same(a, b)
    assert res[0][2].sum() > 0


@pytest.mark.parametrize("mapping", ["default", "ct"])
def test_trace_lights_and_emitted_match(ctx, cpm, mapping):
    import ctypes as C
    S, P, B = cpm.synthetic, cpm.pipeline, cpm.binding
    torch = ctx.torch
    got = []
    tf = ctx.tf_create(S.workspace_tf())
    for vol in _volumes(ctx, cpm, _field(cpm, (33, 20, 17), mapping=mapping), mapping):
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
        res = [_n(ph).copy(), _n(rng).copy()]
        for kw in (dict(), dict(point_light_position=(0.4, 0.6, 2.5))):     # directional, point
            em = P.PhotonFrame(ctx, vol, tf, 64, (16, 16, 16), light_travel_direction=LIGHT_DIR, max_interactions=2, emit_in_tracer=True, **kw)
            em.trace()
            torch.cuda.synchronize()
            res += [_n(em.photons).copy(), _n(em.rng).copy()]
            assert (res[-2][:, 0] < 1e30).any()
        got.append(res)
    for a, b in zip(*got):
        assert _same(a, b)


@pytest.mark.parametrize("mapping", ["default", "ct"])
@pytest.mark.parametrize("dims,region", [((16, 20, 24), 8), ((7, 9, 11), 4), ((32, 32, 32), 16)])
def test_brick_minmax_difference_and_step(ctx, cpm, dims, region, mapping):
    """I16 takes the per-brick kernels whatever the streaming switch says; the F32 twin is run through its per-brick form and through
    its default path (min/max by the row kernel where rows are 16-byte aligned)."""
    torch = ctx.torch
    a, b = _field(cpm, dims, 3, mapping), _field(cpm, dims, 9, mapping)
    nb = int(np.prod([(d + region - 1) // region for d in dims]))

    def run(x, y, streaming):
        ctx.lib.cpm_debug_set_brick_streaming(ctx.h, int(streaming))
        try:
            mm = torch.zeros((nb, 2), dtype=torch.int16, device=ctx.device)
            diff = torch.zeros(nb, dtype=torch.float32, device=ctx.device)
            smm = torch.zeros((nb, 2), dtype=torch.int16, device=ctx.device)
            sdiff = torch.zeros(nb, dtype=torch.float32, device=ctx.device)
            ctx.volume_minmax(x, region, mm)
            ctx.volume_difference(x, y, region, diff)
            ctx.volume_step(x, y, region, sdiff, smm)
            torch.cuda.synchronize()
            return [_n(mm).copy(), _n(diff).copy(), _n(sdiff).copy(), _n(smm).copy()]
        finally:
            ctx.lib.cpm_debug_set_brick_streaming(ctx.h, 1)

    (xa, fa), (xb, fb) = _volumes(ctx, cpm, a, mapping), _volumes(ctx, cpm, b, mapping)
    ref = run(fa, fb, False)
    assert ref[1].max() > 0 and len({int(m) for m in ref[0].reshape(-1).view(np.uint16)}) > 2
    for streaming in (True, False):
        got, twin = run(xa, xb, streaming), run(fa, fb, streaming)
        for g, r, t in zip(got, ref, twin):
            assert _same(g, r) and _same(g, t), streaming
    assert _same(got[1], got[2]) and _same(run(xb, xa, True)[3], got[0])     # the step is the difference + the next volume's min/max


def _mappers(ctx, cpm, v, n_side=96, grid=(16, 16, 16), **kw):
    """(a mapper over the int16 array itself -- the pipeline passes the type through --, its twin over the F32 volume of w(v))"""
    S, P = cpm.synthetic, cpm.pipeline
    out = []
    for vol in (v, _volumes(ctx, cpm, v)[1]):
        cm = P.CorrelatedPhotonMapper(ctx, vol, S.tf_from_points(TFP), n_side, grid, light_travel_direction=LIGHT_DIR, tf_points=TFP,
                                      incremental_threshold_percent=100.0, **kw)
        cm.full_frame()
        out.append(cm)
    assert int(out[0].vol.desc.dtype) == cpm.binding.CPM_I16
    ctx.torch.cuda.synchronize()
    lv = [_n(cm.light_volume).copy() for cm in out]
    assert lv[0].sum() > 0 and _same(lv[0], lv[1])                               # after a full frame: the bits
    assert _same(_n(out[0].photons), _n(out[1].photons))
    return out


def _state(cm, n):
    return [_n(cm.importance_grid).copy(), np.sort(_n(cm.indices)[:n]), _n(cm.photons).copy(), _n(cm.rng).copy()]


def _assert_light_volumes_close(pair):
    a, b = [_n(cm.light_volume) for cm in pair]
    np.testing.assert_allclose(a, b, atol=2e-5 * float(b.max()), **SPLAT_TOL)


@pytest.mark.parametrize("fused", [True, False])
def test_tf_edit_matches(ctx, cpm, fused):
    pair = _mappers(ctx, cpm, _field(cpm, (32, 32, 32)))
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
    _assert_light_volumes_close(pair)


def test_sequence_of_three_steps_matches(ctx, cpm):
    """set_volume with int16 arrays (the mapper keeps the type and the mapping) against adopted F32 volumes of w(v)"""
    steps = [_field(cpm, (32, 32, 32), t) for t in (0, 6, 12, 18)]
    pair = _mappers(ctx, cpm, steps[0])
    total = 0
    for t in range(1, 4):
        res = []
        for cm, nxt in zip(pair, (steps[t], _volumes(ctx, cpm, steps[t])[1])):
            cm.set_volume(nxt)
            n = cm.correlated_update()
            ctx.torch.cuda.synchronize()
            res.append((n, _state(cm, n)))
        assert int(pair[0].vol.desc.dtype) == cpm.binding.CPM_I16 and pair[0].vol.desc.format_offset == 1.0
        assert res[0][0] == res[1][0], t
        total += res[0][0]
        for a, b in zip(res[0][1], res[1][1]):
            assert _same(a, b), t
        _assert_light_volumes_close(pair)
    assert total > 0


def test_mix_converts_the_f32_mix_and_retraces_through_it(ctx, cpm):
    a, b = _field(cpm, (32, 32, 32), 0), _field(cpm, (32, 32, 32), 9)
    (xa, fa), (xb, fb) = _volumes(ctx, cpm, a), _volumes(ctx, cpm, b)
    out16, out32 = _volumes(ctx, cpm, np.zeros_like(a))
    for weight in (0.0, 0.25, 0.5, 1.0):
        ctx.volume_mix(xa, xb, weight, out16)
        ctx.volume_mix(fa, fb, weight, out32)
        m16, m32 = out16.download(), out32.download()
        assert m16.dtype == np.int16 and np.array_equal(m16, snorm_write(m32)), weight
        if weight in (0.0, 1.0):
            assert np.array_equal(m16, np.maximum(a if weight == 0.0 else b, -32767))
    ctx.volume_mix(xa, xb, 0.25, out16)
    m16 = out16.download()
    # the mixed volume's footprint copy is stale: its correlated re-trace reads the linear block (LinearLoad<CPM_I16>); the twin is an
    # I16 volume uploaded with those values (its footprint copy is current)
    res = []
    pair = [_mappers(ctx, cpm, a)[0] for _ in range(2)]
    for cm, vol in zip(pair, (out16, ctx.volume_create(m16))):
        cm.set_volume(vol)
        n = cm.correlated_update()
        ctx.torch.cuda.synchronize()
        res.append((n, _state(cm, n)))
    assert res[0][0] == res[1][0] > 0
    for x, y in zip(res[0][1], res[1][1]):
        assert _same(x, y)


def test_resident_streamed_and_delta_streamed_sequences_agree(ctx, cpm):
    B, P, S = cpm.binding, cpm.pipeline, cpm.synthetic
    steps = [_field(cpm, (32, 32, 32), t * 5) for t in range(4)]
    seq = B.PinnedSequence(ctx, steps)
    tf = ctx.tf_create(S.workspace_tf())

    def photons(v):
        fr = P.PhotonFrame(ctx, v, tf, 48, (16, 16, 16), light_travel_direction=LIGHT_DIR)
        fr.trace()
        ctx.torch.cuda.synchronize()
        return _n(fr.photons).copy()

    resident = [ctx.volume_create(s) for s in steps]
    full, changes = B.VolumeStream(ctx, steps[0], n_slots=3), B.VolumeStream(ctx, steps[0], n_slots=3)
    assert int(full.desc.dtype) == B.CPM_I16
    delta = B.SequenceDelta(ctx, seq, wrap=True)
    changes.use_delta(delta)
    for i, t in enumerate([0, 1, 2, 3, 0, 1]):
        for vs in (full, changes):
            vs.prefetch(t, seq.steps[t])
        got = [vs.acquire(t) for vs in (full, changes)]
        want = photons(resident[t])
        for v in got:
            assert v.download().dtype == np.int16 and np.array_equal(v.download(), steps[t]), (i, t)
            assert _same(photons(v), want), (i, t)
    ctx.torch.cuda.synchronize()
    assert changes.delta_stats().delta_uploads > 0


def _threshold_tf(width=256):
    x = (np.arange(width) + 0.5) / width
    rgb = np.stack([0.6 + 0.4 * np.sin(7 * x), 0.5 + 0.5 * np.cos(5 * x), 0.3 + 0.2 * np.sin(11 * x + 1)], 1)
    return np.concatenate([rgb, np.where(x < 0.6, 0.0, 0.05)[:, None]], 1).astype(F32)


@pytest.mark.parametrize("mapping", ["default", "ct"])
def test_render_plain_skipping_and_shaded_match(ctx, cpm, mapping):
    import torch
    B, S = cpm.binding, cpm.synthetic
    W, H, ldims = 48, 40, (11, 9, 7)
    v = _field(cpm, (37, 20, 19), mapping=mapping)
    v[:8, :8, :16] = v.min()                      # bricks below the threshold TF's first non-zero alpha: something to skip
    pair = _volumes(ctx, cpm, v, mapping)
    lv = torch.from_numpy(light_volume(np.random.default_rng(3), ldims, 4)).to(ctx.device)
    g = B.default_grid_desc(ldims, 4)
    m = matrix(cpm, "diagonal", W, H)
    sh = dict(mode="blinn_phong", texture_to_world=B.texture_to_world(), light_position=(2.0, 3.0, 2.5), shininess=12.0)
    assert B.SHADE_MODES["blinn_phong"] == B.SHADE_BLINN_PHONG
    skipped = 0
    for lut in (S.workspace_tf(256), _threshold_tf()):
        res = []
        for vol in pair:
            tf = ctx.tf_create(lut)
            imgs, infos = [ctx.render(vol, tf, lv, g, W, H, ndc_to_texture=m, sampling_rate=1.5)], []
            imgs.append(ctx.render(vol, tf, lv, g, W, H, ndc_to_texture=m, sampling_rate=1.5, shading=sh))
            for brick in (4, 8):
                accel = ctx.render_accel(vol, brick)
                accel.update(vol, tf)
                st = torch.zeros(2, dtype=torch.int32, device=ctx.device)
                imgs.append(ctx.render(vol, tf, lv, g, W, H, ndc_to_texture=m, sampling_rate=1.5, accel=accel, stats=st))
                imgs.append(ctx.render(vol, tf, lv, g, W, H, ndc_to_texture=m, sampling_rate=1.5, accel=accel, shading=sh))
                torch.cuda.synchronize()
                infos.append((accel.info(), [int(x) & 0xffffffff for x in st.cpu().tolist()]))
                accel.close()
            res.append(([_n(i).copy() for i in imgs], infos))
        for a, b in zip(res[0][0], res[1][0]):
            assert _same(a, b)
        assert res[0][1] == res[1][1]                                        # bricks, n_empty and the (evaluated, skipped) pair
        imgs = res[0][0]
        assert imgs[0][..., 3].max() > 0 and not _same(imgs[0], imgs[1])
        assert _same(imgs[0], imgs[2]) and _same(imgs[0], imgs[4]) and _same(imgs[1], imgs[3]) and _same(imgs[1], imgs[5])
        skipped += sum(st[1] for _, st in res[0][1])
    assert skipped > 0


def test_refusals_still_fire(ctx, cpm):
    import torch
    B, S = cpm.binding, cpm.synthetic
    W, H, ldims = 48, 40, (8, 8, 8)
    v = _field(cpm, (16, 20, 24))
    x16, f32 = _volumes(ctx, cpm, v)
    tf = ctx.tf_create(S.workspace_tf(256))
    lv = torch.from_numpy(light_volume(np.random.default_rng(4), ldims, 1)).to(ctx.device)
    g = B.default_grid_desc(ldims, 1)
    m = matrix(cpm, "face-on", W, H)
    for other in (f32, ctx.volume_create(v.view(np.uint16))):                # an accel made for another type (same dims, even same bytes)
        accel = ctx.render_accel(other, 8)
        with pytest.raises(B.CpmError):
            accel.update(x16, tf)
        accel.update(other, tf)
        with pytest.raises(Exception):
            ctx.render(x16, tf, lv, g, W, H, ndc_to_texture=m, accel=accel)
        accel.close()
    buf = torch.full((W * H * 4 + 1,), -7.0, dtype=torch.float32, device=ctx.device)
    with pytest.raises(B.CpmError):
        ctx.render(x16, tf, lv, g, W, H, ndc_to_texture=m, out=buf[1:])      # 4 bytes off a 16-byte boundary
    torch.cuda.synchronize()
    assert (buf == -7.0).all()
    with pytest.raises(B.CpmError):                                           # volumes of two types do not mix or step
        ctx.volume_mix(x16, f32, 0.5, x16)
    with pytest.raises(B.CpmError):
        ctx.volume_difference(x16, f32, 8, torch.zeros(2 * 3 * 3, dtype=torch.float32, device=ctx.device))
