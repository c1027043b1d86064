"""cpm_render_shaded on the device (include/cpm/cpm_ext.h; DESIGN.md "Gradient shading"): mode NONE is cpm_render_ex bit for bit; every
mode x voxel type x light layout x ray mode against the numpy restatement (tests/render_shaded_reference.py) on the inputs of
tests/render_shaded_cases.py; skipping leaves a shaded image's bits alone; closed forms of a constant medium and of a ramp; repeatability;
the refusals; a PhotonFrame end to end.

Tolerance of the comparison with the restatement (float64 shading from float32 gradients): the shading formulas evaluated in numpy
float32 on the same samples need rtol 6.8e-7 at atol 1e-6 (measured on the CPU by test_render_shaded_cpu, which asserts <= 7e-7); four
times that, 2.8e-6, is below the project's own rtol 1e-5 / atol 1e-6, which therefore stands.  Pixels the restatement marks ambiguous
(early termination one sample apart) are excluded: at most 0.5 % of the live pixels, which the CPU test asserts on the same inputs."""
import ctypes as C

import numpy as np
import pytest

import render_reference as R
import render_shaded_cases as K
import render_shaded_reference as RS
from test_render_gpu import H, W, const_case, light_volume, matrix, random_tf, random_volume

pytestmark = pytest.mark.gpu
F32 = np.float32
UNIT_BOX = (0.0, 0.0, 0.0, 1.0, 1.0, 1.0, 1.0, 1.0)


def bits(t):
    return t.cpu().numpy().view(np.uint32)


def device(ctx, cpm, vol, lut, lv, ldims, channels):
    import torch
    return (ctx.volume_create(vol), ctx.tf_create(lut), torch.from_numpy(lv).to(ctx.device), cpm.binding.default_grid_desc(ldims, channels))


def rays_on_device(ctx, kw):
    import torch
    if "entry" in kw:
        return dict(entry=torch.from_numpy(kw["entry"]).to(ctx.device), exit=torch.from_numpy(kw["exit"]).to(ctx.device),
                    ndc_to_texture=np.zeros(16, F32))
    return dict(kw)


def assert_matches(got, want, amb, what):
    ok = np.isclose(got, want, rtol=K.RTOL, atol=K.ATOL).all(-1) | amb
    print(what, "needs rtol", RS.needed_rtol(got[~amb], want[~amb], K.ATOL), "excluded", int(amb.sum()))
    assert ok.all(), (what, np.argwhere(~ok)[:5], got[~ok][:3], want[~ok][:3])


def test_mode_none_and_null_are_cpm_render_ex(ctx, cpm):
    """(a) shading = NULL and mode NONE: the kernels and the bits of cpm_render_ex, with and without accel / clip / stats"""
    import torch
    B = cpm.binding
    rng = np.random.default_rng(5)
    vol, lut, lv = random_volume(rng, np.uint8), random_tf(rng), light_volume(rng, (9, 9, 9), 4)
    v, t, lvt, g = device(ctx, cpm, vol, lut, lv, (9, 9, 9), 4)
    acc = ctx.render_accel(v, 4)
    acc.update(v, t)
    m = matrix(cpm, "diagonal")
    clip = (0.1, 0.0, 0.2, 1.0, 0.9, 1.0, 0.8, 1.0)
    none = B.Shading(mode="none", light_position=(float("nan"),) * 3)   # NONE looks at nothing else
    for kw in (dict(), dict(clip=clip), dict(accel=acc), dict(accel=acc, clip=clip)):
        for with_stats in (False, True):
            st = [torch.zeros(2, dtype=torch.int32, device=ctx.device) for _ in range(2)]
            a = ctx.render(v, t, lvt, g, W, H, ndc_to_texture=m, stats=st[0] if with_stats else None, **(kw or dict(clip=UNIT_BOX)))
            b = ctx.render(v, t, lvt, g, W, H, ndc_to_texture=m, stats=st[1] if with_stats else None, shading=none, **kw)
            assert np.array_equal(bits(a), bits(b)) and (a[..., 3] > 0).any(), kw
            assert torch.equal(st[0], st[1]) and (not with_stats or int(st[0][0]) > 0)
    # a NULL shading and NULL options through the entry point itself: the bits of cpm_render
    d = B.RenderDesc()
    d.width, d.height, d.sampling_rate, d.colored_light = W, H, 1.0, 1
    d.ndc_to_texture[:] = m.tolist()
    out = torch.empty((H, W, 4), dtype=torch.float32, device=ctx.device)
    assert ctx.lib.cpm_render_shaded(ctx.h, v.h, t.h, C.c_void_p(lvt.data_ptr()), C.byref(g), C.byref(d), None, None,
                                     C.c_void_p(out.data_ptr()), ctx._stream()) == 0
    assert np.array_equal(bits(out), bits(ctx.render(v, t, lvt, g, W, H, ndc_to_texture=m)))
    # ... and a shaded image is another image
    assert not np.array_equal(bits(out), bits(ctx.render(v, t, lvt, g, W, H, ndc_to_texture=m, shading=K.shading("phong"))))


@pytest.mark.parametrize("rays", K.RAYS)
@pytest.mark.parametrize("channels", K.CHANNELS)
@pytest.mark.parametrize("dtype", K.DTYPES)
def test_matches_the_reference(ctx, cpm, dtype, channels, rays):
    """(b) every mode against the restatement"""
    vol, lut, lv, kw = K.inputs(cpm, dtype, channels, rays)
    v, t, lvt, g = device(ctx, cpm, vol, lut, lv, K.LIGHT_DIMS, channels)
    dev_kw = rays_on_device(ctx, kw)
    seen = []
    for mode in K.MODE_NAMES:
        got = ctx.render(v, t, lvt, g, W, H, sampling_rate=K.RATE, shading=K.shading(mode), **dev_kw).cpu().numpy()
        want, amb = K.reference(vol, lut, lv, channels, kw, mode)
        live = want[..., 3] > 0
        assert live.sum() > 1000 and amb.sum() <= K.MAX_AMBIGUOUS * live.sum()
        assert_matches(got, want, amb, (np.dtype(dtype).name, channels, rays, mode))
        assert all(not np.array_equal(got, s) for s in seen)
        seen.append(got)


def test_skipping_keeps_the_shaded_bits(ctx, cpm):
    """(c) with an accel the shaded image has the bits of the shaded image without one; evaluated + skipped = the plain sample count"""
    import torch
    rng = np.random.default_rng(8)
    vol = random_volume(rng, np.uint8, (40, 36, 33))
    vol[:, :, :20] //= 4   # values below 0.25: empty under random_tf (alpha 0 below 0.3)
    vol[:18] //= 4
    lut, lv = random_tf(rng), light_volume(rng, (9, 9, 9), 1)
    v, t, lvt, g = device(ctx, cpm, vol, lut, lv, (9, 9, 9), 1)
    acc = ctx.render_accel(v, 4)
    acc.update(v, t)
    assert acc.info()[1] > 0
    m = matrix(cpm, "diagonal")
    for mode in ("diffuse", "phong"):
        sh = K.shading(mode)
        st0, st1 = (torch.zeros(2, dtype=torch.int32, device=ctx.device) for _ in range(2))
        plain = ctx.render(v, t, lvt, g, W, H, ndc_to_texture=m, shading=sh, stats=st0)
        fast = ctx.render(v, t, lvt, g, W, H, ndc_to_texture=m, shading=sh, stats=st1, accel=acc)
        bare = ctx.render(v, t, lvt, g, W, H, ndc_to_texture=m, shading=sh, accel=acc)
        assert np.array_equal(bits(plain), bits(fast)) and np.array_equal(bits(plain), bits(bare)) and (plain[..., 3] > 0).any()
        assert int(st0[1]) == 0 and int(st1[1]) > 0 and int(st1[0]) + int(st1[1]) == int(st0[0])


def test_constant_medium_is_ambient_times_the_closed_form(ctx, cpm):
    """(d) a constant volume has g = 0 exactly: every mode is ka (.) the unshaded closed form"""
    w, h = 33, 29
    m = matrix(cpm, "face-on", w, h)
    ent, ext, hit = R.camera_rays(m, w, h)
    n, t_incr, _, live = R.sample_counts(ent, ext, hit, (16, 16, 16), 1.0)
    expo = (t_incr * F32(150)).astype(F32).astype(np.float64)
    want_a = 1.0 - (1.0 - (1.0 - (1.0 - float(F32(0.02))) ** expo)) ** n
    c = np.array([0.8, 0.5, 0.25], F32)
    vol, lut, lv = const_case(0.02, 0.5)
    v, t, lvt, g = device(ctx, cpm, vol, lut, lv, (16, 16, 16), 1)
    for mode in K.MODE_NAMES:
        sh = K.shading(mode)
        img = ctx.render(v, t, lvt, g, w, h, ndc_to_texture=m, shading=sh).cpu().numpy()
        ka = np.array(sh["ambient"], F32)
        assert (img[~live] == 0).all() and live.sum() > 100
        assert np.allclose(img[live, 3], want_a[live], rtol=1e-5, atol=0), mode
        assert np.allclose(img[live, :3], (ka * c * F32(0.5))[None, :] * want_a[live, None], rtol=1e-5, atol=0), mode


def test_ramp_diffuse_closed_form(ctx, cpm):
    """(e) a ramp along z seen along z with the light far away on the z axis: DIFFUSE = (ka + kd |N.L|) (.) the unshaded closed form,
    |N.L| in float64 at every sample position from the restatement's gradient"""
    import torch
    dims = (16, 16, 16)
    vol = np.broadcast_to((np.arange(16, dtype=np.uint16) * np.uint16(4000)).reshape(16, 1, 1), (16, 16, 16)).copy()
    lut = np.tile(np.array([0.8, 0.5, 0.25, 0.02], F32), (64, 1))
    lv = np.full(16 ** 3, 0.5, F32)
    w, h = 12, 10
    y, x = np.meshgrid(np.linspace(0.1, 0.9, h, dtype=F32), np.linspace(0.1, 0.9, w, dtype=F32), indexing="ij")
    e = np.stack([x, y, np.zeros_like(x), np.ones_like(x)], -1).astype(F32)
    xx = np.stack([x, y, np.ones_like(x), np.ones_like(x)], -1).astype(F32)
    light = np.array([0.5, 0.5, 1000.0])
    sh = dict(mode="diffuse", texture_to_world=None, light_position=light, ambient=(0.2, 0.15, 0.1), diffuse=(0.6, 0.7, 0.5),
              specular=(0.0,) * 3, shininess=1.0)
    n, t_incr, d, live = R.sample_counts(e[..., :3], xx[..., :3], np.ones((h, w), bool), dims, 1.0)
    assert (n == 16).all() and live.all()
    k = np.arange(16, dtype=F32)
    tt = ((k + F32(0.5))[None, None, :] * t_incr[..., None]).astype(F32)
    p = (e[..., None, :3] + tt[..., None] * d[..., None, :]).astype(F32)          # [h, w, 16, 3]
    gr = RS.gradient(vol, p.reshape(-1, 3)).astype(np.float64)
    assert (np.abs(gr[:, 2]) > 0).all()
    N = gr / np.linalg.norm(gr, axis=-1, keepdims=True)
    L = light - p.reshape(-1, 3).astype(np.float64)
    L /= np.linalg.norm(L, axis=-1, keepdims=True)
    nl = np.abs((N * L).sum(-1)).reshape(h, w, 16)
    assert nl.min() > 1 - 1e-6 and nl.max() <= 1 + 1e-12   # the same factor at every sample of a ray, to 1e-6
    factor = np.array(sh["ambient"], F32)[None, None, :] + np.array(sh["diffuse"], F32)[None, None, :] * nl.mean(-1)[..., None]
    expo = (t_incr * F32(150)).astype(F32).astype(np.float64)
    want_a = 1.0 - (1.0 - (1.0 - (1.0 - float(F32(0.02))) ** expo)) ** n
    v, t, lvt, g = device(ctx, cpm, vol, lut, lv, dims, 1)
    dev = dict(entry=torch.from_numpy(e).to(ctx.device), exit=torch.from_numpy(xx).to(ctx.device), ndc_to_texture=np.zeros(16, F32))
    img = ctx.render(v, t, lvt, g, w, h, shading=sh, **dev).cpu().numpy()
    plain = ctx.render(v, t, lvt, g, w, h, **dev).cpu().numpy()
    c = np.array([0.8, 0.5, 0.25], F32) * F32(0.5)
    assert np.allclose(plain[..., :3], c[None, None, :] * want_a[..., None], rtol=1e-5, atol=0)
    assert np.allclose(img[..., 3], want_a, rtol=1e-5, atol=0)
    assert np.allclose(img[..., :3], factor * c[None, None, :] * want_a[..., None], rtol=1e-5, atol=0)


def test_two_runs_give_the_same_bits(ctx, cpm):
    """(f)"""
    vol, lut, lv, kw = K.inputs(cpm, np.float16, 4, "camera")
    v, t, lvt, g = device(ctx, cpm, vol, lut, lv, K.LIGHT_DIMS, 4)
    for mode in ("blinn_phong", "phong"):
        a = ctx.render(v, t, lvt, g, W, H, sampling_rate=2.0, shading=K.shading(mode), **kw)
        b = ctx.render(v, t, lvt, g, W, H, sampling_rate=2.0, shading=K.shading(mode), **kw)
        assert np.array_equal(bits(a), bits(b)) and (a[..., 3] > 0).any()


def test_refusals_write_nothing(ctx, cpm):
    """(g) every refusal leaves a poisoned output untouched"""
    import torch
    B = cpm.binding
    rng = np.random.default_rng(2)
    v, t = ctx.volume_create(random_volume(rng, np.uint8)), ctx.tf_create(random_tf(rng))
    lv = torch.ones(8 * 8 * 8 * 4, dtype=torch.float32, device=ctx.device)
    out = torch.full((16, 16, 4), -7.0, dtype=torch.float32, device=ctx.device)
    s = ctx._stream()
    nan, inf = float("nan"), float("inf")
    eye = np.eye(4, dtype=F32)

    def call(channels=1, clip=None, rate=1.0, **sh):
        g = B.default_grid_desc((8, 8, 8), 1)
        g.channels = channels
        d = B.RenderDesc()
        d.width, d.height, d.sampling_rate, d.colored_light = 16, 16, rate, 1
        d.ndc_to_texture[:] = matrix(cpm, "face-on", 16, 16).tolist()
        o = B.RenderOptions()
        if clip is not None:
            box = (C.c_float * 8)(*clip)
            o.clip_aabb = C.cast(box, C.POINTER(C.c_float))
        h = B.Shading(**{**dict(mode="phong", light_position=(1.0, 2.0, 3.0), shininess=10.0), **sh}).struct()
        return ctx.lib.cpm_render_shaded(ctx.h, v.h, t.h, C.c_void_p(lv.data_ptr()), C.byref(g), C.byref(d), C.byref(o), C.byref(h),
                                         C.c_void_p(out.data_ptr()), s)

    assert call() == 0   # the arguments below differ from a good call in one place each
    torch.cuda.synchronize()
    assert (out != -7.0).any()
    out.fill_(-7.0)

    def mat(**cells):
        m = eye.copy()
        for k, val in cells.items():
            m[int(k[1]), int(k[2])] = val   # m<row><col>
        return m.T.reshape(16)

    bad = [dict(mode=6), dict(mode=-1), dict(mode=1 << 20),
           dict(light_position=(nan, 0.0, 0.0)), dict(light_position=(0.0, inf, 0.0)), dict(ambient=(0.1, nan, 0.1)), dict(diffuse=(-inf, 0.0, 0.0)),
           dict(specular=(0.0, 0.0, nan)), dict(shininess=0.0), dict(shininess=-2.0), dict(shininess=nan), dict(shininess=inf),
           dict(texture_to_world=mat(m01=nan)), dict(texture_to_world=mat(m13=inf)), dict(texture_to_world=mat(m30=0.5)),
           dict(texture_to_world=mat(m32=-1.0)), dict(texture_to_world=mat(m33=2.0)), dict(texture_to_world=mat(m33=0.0)),
           dict(texture_to_world=mat(m11=0.0)), dict(texture_to_world=mat(m00=1.0, m01=2.0, m10=2.0, m11=4.0)),
           # ... and what cpm_render_ex refuses
           dict(channels=2), dict(rate=0.0), dict(clip=(0.5, 0.0, 0.0, 1.0, 0.5, 1.0, 1.0, 1.0)), dict(clip=(nan, 0.0, 0.0, 1.0, 1.0, 1.0, 1.0, 1.0))]
    for kw in bad:
        assert call(**kw) == -1, kw
    torch.cuda.synchronize()
    assert (out == -7.0).all()
    # an accel that saw another TF is refused with shading as without
    acc = ctx.render_accel(v, 8)
    acc.update(v, t)
    other = ctx.tf_create(random_tf(rng))
    with pytest.raises(Exception):
        ctx.render(v, other, lv, B.default_grid_desc((8, 8, 8), 4), 16, 16, ndc_to_texture=matrix(cpm, "face-on", 16, 16), accel=acc,
                   shading=K.shading("phong"), out=out)
    torch.cuda.synchronize()
    assert (out == -7.0).all()
    with pytest.raises(ValueError):
        B.Shading(mode="gooch").struct()


def test_photon_frame_end_to_end(ctx, cpm):
    """(h) a traced and gathered frame, rendered with shading= (and with skipping: the same bits)"""
    import torch
    S, P = cpm.synthetic, cpm.pipeline
    vol, tf = S.heterogeneous_volume(32), S.workspace_tf()
    fr = P.PhotonFrame(ctx, vol, tf, 128, (16, 16, 16), light_travel_direction=(0.3, 0.5, -1.0))
    fr.frame_fast()
    m = matrix(cpm, "diagonal", 80, 64)
    sh = dict(mode="blinn_phong", texture_to_world=cpm.binding.texture_to_world(), light_position=(2.0, 3.0, 2.5), ambient=0.15, diffuse=0.6,
              specular=0.4, shininess=12.0)
    img = fr.render(80, 64, ndc_to_texture=m, sampling_rate=1.5, shading=sh)
    fast = fr.render(80, 64, ndc_to_texture=m, sampling_rate=1.5, shading=sh, skip_empty=True)
    assert np.array_equal(bits(img), bits(fast))
    assert not np.array_equal(bits(img), bits(fr.render(80, 64, ndc_to_texture=m, sampling_rate=1.5)))
    torch.cuda.synchronize()
    lv = fr.light_volume.cpu().numpy()
    ref_sh = dict(sh, ambient=(0.15,) * 3, diffuse=(0.6,) * 3, specular=(0.4,) * 3)
    want, amb = RS.render(vol, tf, lv, (16, 16, 16), 1, 80, 64, shading=ref_sh, ndc_to_texture=m, sampling_rate=1.5)
    live = want[..., 3] > 0
    print("photon frame: ambiguous", int(amb.sum()), "of", int(live.sum()), "live pixels")
    assert live.mean() > 0.2 and want[..., :3].max() > 0 and amb.sum() <= K.MAX_AMBIGUOUS * live.sum()
    assert_matches(img.cpu().numpy(), want, amb, "photon frame")
