"""cpm_render_ex on the device (include/cpm/cpm_ext.h): empty-space skipping gives the bits of cpm_render over a fixed sweep, really
skips, counts its samples as the plain loop does, follows edits of the TF and of the voxels once the accel is updated, honours the clip
box, and refuses what the header says it refuses.  The rule itself is held to the oracle in tests/test_render_skip_cpu.py; its numpy
restatement there also gives the empty-brick counts the device's bits are compared with."""
import ctypes as C

import numpy as np
import pytest

import render_reference as R
import test_render_skip_cpu as SK
from test_render_gpu import CAMERAS, W, H, matrix, light_volume, const_case

pytestmark = pytest.mark.gpu
F32 = np.float32
RAGGED = (37, 20, 9)
RATES = (0.5, 1.0, 2.7)
BRICKS = (4, 8, 16)
DTYPES = (np.uint8, np.uint16, np.float16, np.float32)
LDIMS = (11, 9, 7)


def as_dtype(u8, dtype):
    """a u8 volume in another voxel type, the same normalised values up to that type's precision"""
    if np.dtype(dtype) == np.uint8:
        return u8
    if np.dtype(dtype) == np.uint16:
        return u8.astype(np.uint16) * np.uint16(257)
    return (u8.astype(F32) / F32(255)).astype(dtype)


def volume(cpm, kind, dtype):
    S = cpm.synthetic
    rng = np.random.default_rng(41)
    if kind == "config2":
        return as_dtype(S.heterogeneous_volume(256), dtype)
    if kind == "blob":
        return as_dtype(S.blob_volume((96, 80, 64), (0.45, 0.5, 0.55)), dtype)
    if kind == "noise":
        return as_dtype(rng.integers(0, 256, (24, 40, 56), dtype=np.uint8), dtype)
    if kind == "ragged":
        return as_dtype(SK.smooth_volume(RAGGED, np.uint8, 7), dtype)
    if kind == "thin":
        return as_dtype(SK.smooth_volume((16, 1, 23), np.uint8, 9), dtype)
    raise KeyError(kind)


def tfs(cpm):
    return SK.skip_tfs(256, with_workspace=cpm.synthetic.workspace_tf(256))


class Scene:
    def __init__(self, ctx, cpm, vol_np, lut, channels=1, ldims=LDIMS, seed=5):
        import torch
        self.ctx, self.cpm, self.torch = ctx, cpm, torch
        self.vol_np = vol_np
        self.v, self.t = ctx.volume_create(vol_np), ctx.tf_create(lut)
        self.lv = {}
        for ch in (1, 4):
            lv = light_volume(np.random.default_rng(seed + ch), ldims, ch)
            self.lv[ch] = (torch.from_numpy(lv).to(ctx.device), cpm.binding.default_grid_desc(ldims, ch), lv)
        self.ldims = ldims

    def render(self, channels=1, w=W, h=H, **kw):
        lv, g, _ = self.lv[channels]
        return self.ctx.render(self.v, self.t, lv, g, w, h, **kw)

    def stats(self):
        return self.torch.zeros(2, dtype=self.torch.int32, device=self.ctx.device)


def counts(st):
    return [int(x) & 0xffffffff for x in st.cpu().tolist()]


def outside_buffers(cpm, cam, w=W, h=H, scale=1.35):
    """the camera's entry / exit points pushed away from the volume's centre: partly outside [0,1]^3 (the sampler clamps there)"""
    e, x = R.camera_buffers(matrix(cpm, cam, w, h), w, h)
    for b in (e, x):
        b[..., :3] = (F32(0.5) + (b[..., :3] - F32(0.5)) * F32(scale)).astype(F32)
    pts = np.concatenate([e[e[..., 3] != 0][:, :3], x[e[..., 3] != 0][:, :3]])
    outside = ((pts < 0) | (pts > 1)).any(-1)
    assert outside.sum() > 100   # (the points between them are inside: the rays still cross the volume)
    return e, x


# ------------------------------------------------------------------------------------------------------------------- bit equality

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", ["config2", "blob", "noise", "ragged", "thin"])
def test_skipping_gives_the_bits_of_the_plain_render(ctx, cpm, kind, dtype):
    """every TF x brick size x channels / colored light x camera x rate, and the buffer mode: torch.equal with cpm_render; and in every
    case evaluated + skipped samples = the samples the plain loop evaluates, counted by the same code"""
    import torch
    vol = volume(cpm, kind, dtype)
    luts = tfs(cpm)
    sc = Scene(ctx, cpm, vol, luts["threshold"])
    cases = skipped_somewhere = 0
    bufs = {cam: tuple(torch.from_numpy(b).to(ctx.device) for b in outside_buffers(cpm, cam)) for cam in ("diagonal", "inside")}
    for brick in BRICKS:
        accel = ctx.render_accel(sc.v, brick)
        for name, lut in luts.items():
            sc.t.update(lut)
            accel.update(sc.v, sc.t)
            if kind in ("ragged", "thin"):   # the device's bits against the numpy restatement
                dims = vol.shape[::-1]
                want = SK.empty_bricks(*SK.range_grid(vol, brick), lut[:, 3])
                nb, n_empty = accel.info()
                assert nb == tuple(-(-d // brick) for d in dims) and n_empty == int(want.sum()), (name, brick, n_empty, int(want.sum()))
            for channels, colored in ((1, True), (4, True), (4, False)):
                rays = [dict(ndc_to_texture=matrix(cpm, cam)) for cam in CAMERAS]
                rays += [dict(entry=e, exit=x, ndc_to_texture=np.zeros(16, F32)) for e, x in bufs.values()]
                for ray in rays:
                    for rate in RATES:
                        kw = dict(channels=channels, colored_light=colored, sampling_rate=rate, **ray)
                        plain = sc.render(**kw)
                        s_plain, s_skip = sc.stats(), sc.stats()
                        counted = sc.render(stats=s_plain, **kw)
                        fast = sc.render(accel=accel, **kw)
                        fast_counted = sc.render(accel=accel, stats=s_skip, **kw)
                        where = (kind, np.dtype(dtype).name, brick, name, channels, colored, rate, "buffers" if "entry" in ray else "camera")
                        assert torch.equal(plain.view(torch.int32), fast.view(torch.int32)), where
                        assert torch.equal(plain.view(torch.int32), counted.view(torch.int32)), where
                        assert torch.equal(plain.view(torch.int32), fast_counted.view(torch.int32)), where
                        a, b = counts(s_plain), counts(s_skip)
                        assert a[1] == 0 and a[0] > 0 and b[0] + b[1] == a[0], (where, a, b)
                        if name == "all-zero":
                            assert b[0] == 0 and not plain.any(), where
                        if kind == "noise" and name == "all-non-zero":
                            assert b[1] == 0, where
                        skipped_somewhere += b[1] > 0
                        cases += 1
        accel.close()
    # noise has nothing to skip but under the all-zero TF (one TF in nine)
    assert cases == len(BRICKS) * len(luts) * 3 * 5 * len(RATES) and skipped_somewhere > (cases // 10 if kind == "noise" else cases // 4)


# ------------------------------------------------------------------------------------------------------------------ really skips

def test_an_empty_volume_costs_at_most_a_sample_per_brick_crossed(ctx, cpm):
    luts = tfs(cpm)
    for kind in ("config2", "ragged"):
        vol = volume(cpm, kind, np.uint8)
        sc = Scene(ctx, cpm, vol, luts["all-zero"])
        for brick in BRICKS:
            accel = ctx.render_accel(sc.v, brick)
            accel.update(sc.v, sc.t)
            nb, n_empty = accel.info()
            assert n_empty == nb[0] * nb[1] * nb[2]
            for cam in CAMERAS:
                st = sc.stats()
                img = sc.render(accel=accel, stats=st, ndc_to_texture=matrix(cpm, cam))
                ev, sk = counts(st)
                print(kind, brick, cam, "evaluated", ev, "skipped", sk)
                assert ev <= W * H * (sum(nb) + 3) and sk > 0 and not img.any()


def test_noise_under_an_opaque_tf_skips_nothing(ctx, cpm):
    sc = Scene(ctx, cpm, volume(cpm, "noise", np.uint8), tfs(cpm)["all-non-zero"])
    accel = ctx.render_accel(sc.v, 8)
    accel.update(sc.v, sc.t)
    assert accel.info()[1] == 0
    st = sc.stats()
    sc.render(accel=accel, stats=st, ndc_to_texture=matrix(cpm, "diagonal"))
    assert counts(st)[1] == 0 and counts(st)[0] > 0


def test_the_plain_count_is_the_restatements(ctx, cpm):
    """64 x 64, whole image: the samples cpm_render_ex counts without an accel are the samples render_reference takes; the camera and the TF
    leave no pixel whose termination the restatement cannot decide"""
    vol = volume(cpm, "ragged", np.uint16)
    lut = tfs(cpm)["threshold"].copy()
    lut[:, 3] *= F32(0.04)   # alpha 0.002 per reference step: no ray comes near the 0.99 of early termination
    sc = Scene(ctx, cpm, vol, lut)
    m = matrix(cpm, "diagonal", 64, 64)
    _, _, lv = sc.lv[1]
    want, amb, (taken, fetched) = R.render(vol, lut, lv, sc.ldims, 1, 64, 64, ndc_to_texture=m, stats=True)
    assert not amb.any() and want[..., 3].max() < 0.9 and taken > 10000 and 0 < fetched < taken
    st, st2 = sc.stats(), sc.stats()
    sc.render(w=64, h=64, stats=st, ndc_to_texture=m)
    print("plain count", counts(st), "restatement", taken)
    assert counts(st) == [taken, 0]
    accel = ctx.render_accel(sc.v, 4)
    accel.update(sc.v, sc.t)
    sc.render(w=64, h=64, stats=st2, accel=accel, ndc_to_texture=m)
    ev, sk = counts(st2)
    assert ev + sk == taken and sk > 0 and ev >= fetched   # every sample with alpha is evaluated


# --------------------------------------------------------------------------------------------------------------------- freshness

def raw_render_ex(ctx, cpm, sc, accel_h, out, clip=None, channels=1, w=16, h=16):
    """cpm_render_ex through ctypes alone (no Python-side tracking) -> status"""
    B = cpm.binding
    lv, g, _ = sc.lv[channels]
    d = B.RenderDesc()
    d.width, d.height, d.sampling_rate, d.colored_light = w, h, 1.0, 1
    d.ndc_to_texture[:] = matrix(cpm, "diagonal", w, h).tolist()
    o = B.RenderOptions()
    o.accel = accel_h.value if accel_h is not None else None
    if clip is not None:
        box = (C.c_float * 8)(*clip)
        o.clip_aabb = C.cast(box, C.POINTER(C.c_float))
    return ctx.lib.cpm_render_ex(ctx.h, sc.v.h, sc.t.h, C.c_void_p(lv.data_ptr()), C.byref(g), C.byref(d), C.byref(o), C.c_void_p(out.data_ptr()),
                                 ctx._stream())


def test_the_accel_follows_edits_once_it_is_updated(ctx, cpm):
    import torch
    S, B = cpm.synthetic, cpm.binding
    m = matrix(cpm, "diagonal")
    vol0 = S.blob_volume(64, (0.4, 0.5, 0.5))
    vol1 = S.blob_volume(64, (0.6, 0.45, 0.5))
    sc = Scene(ctx, cpm, vol0, S.workspace_tf(1024))
    accel = ctx.render_accel(sc.v, 8)
    accel.update(sc.v, sc.t)

    def check(what):
        plain, fast = sc.render(ndc_to_texture=m), sc.render(accel=accel, ndc_to_texture=m)
        assert torch.equal(plain.view(torch.int32), fast.view(torch.int32)) and plain.any(), what
        return plain

    first = check("first")
    # a TF edit (config 3's: point 4 moves from 0.2218 to 0.26); the binding notices that the accel is behind
    sc.t.update(S.workspace_tf(1024, moved_point4=0.26))
    with pytest.raises(ValueError):
        sc.render(accel=accel, ndc_to_texture=m)
    accel.update(tf=sc.t)
    assert not torch.equal(check("tf edit"), first)
    # cpm_volume_update
    sc.v.update(vol1)
    with pytest.raises(ValueError):
        sc.render(accel=accel, ndc_to_texture=m)
    accel.update(vol=sc.v)
    second = check("volume update")
    assert not torch.equal(second, first)
    # cpm_volume_mix into the rendered volume: its footprint copy is stale when the accel reads the linear block
    a, b = ctx.volume_create(vol0), ctx.volume_create(vol1)
    ctx.volume_mix(a, b, 0.5, sc.v)
    with pytest.raises(ValueError):
        sc.render(accel=accel, ndc_to_texture=m)
    accel.update(vol=sc.v)
    fast = sc.render(accel=accel, ndc_to_texture=m)          # (the render rebuilds the copy)
    plain = sc.render(ndc_to_texture=m)
    assert torch.equal(plain.view(torch.int32), fast.view(torch.int32)) and not torch.equal(plain, second)
    # a streamed acquire: another cpm_volume object each step -- without an update the ABI refuses and writes nothing
    seq = B.PinnedSequence(ctx, [vol0, vol1])
    stream = B.VolumeStream(ctx, vol0, n_slots=3)
    own = sc.v
    sc.v = stream.acquire(0, seq.steps[0])
    accel.update(vol=sc.v)
    check("acquire 0")
    sc.v = stream.acquire(1, seq.steps[1])
    out = torch.full((16, 16, 4), -7.0, dtype=torch.float32, device=ctx.device)
    assert raw_render_ex(ctx, cpm, sc, accel.h, out) == -1
    torch.cuda.synchronize()
    assert (out == -7.0).all()
    with pytest.raises(ValueError):
        sc.render(accel=accel, ndc_to_texture=m)
    accel.update(vol=sc.v)
    assert raw_render_ex(ctx, cpm, sc, accel.h, out) == 0
    assert torch.equal(check("acquire 1"), second)
    sc.v = own
    accel.close()
    stream.close()
    seq.close()


# ---------------------------------------------------------------------------------------------------------------------- clip box

def clip_segment_box(o, f, lo, hi):
    """render_reference.clip_segment against the box (lo, hi) instead of [0,1]^3: the kernel's slab test, operation by operation"""
    d = [f[a] - o[a] for a in range(3)]
    s0, s1 = np.zeros_like(d[0]), np.ones_like(d[0])
    with np.errstate(all="ignore"):
        for a in range(3):
            inv = F32(1) / d[a]
            ta, tb = (F32(lo[a]) - o[a]) * inv, (F32(hi[a]) - o[a]) * inv
            s0 = np.fmax(s0, np.fmin(ta, tb))
            s1 = np.fmin(s1, np.fmax(ta, tb))
        hit = s0 < s1
        entry = np.stack([o[a] + s0 * d[a] for a in range(3)], axis=-1).astype(F32)
        exit_ = np.stack([o[a] + s1 * d[a] for a in range(3)], axis=-1).astype(F32)
    return entry, exit_, hit


def camera_segments(m, w, h):
    j, i = np.meshgrid(np.arange(h, dtype=F32), np.arange(w, dtype=F32), indexing="ij")
    nx = F32(2) * (i + F32(0.5)) / F32(w) - F32(1)
    ny = F32(2) * (j + F32(0.5)) / F32(h) - F32(1)
    return R.unproject(m, nx, ny, F32(-1)), R.unproject(m, nx, ny, F32(1))


def test_the_clip_box(ctx, cpm):
    import torch
    unit = (0, 0, 0, 1, 1, 1, 1, 1)
    box = (0.2, 0.1, 0.25, 1.0, 0.7, 0.9, 0.75, 1.0)
    lo, hi = box[0:3], box[4:7]
    sc = Scene(ctx, cpm, volume(cpm, "ragged", np.uint8), tfs(cpm)["band"])
    accel = ctx.render_accel(sc.v, 4)
    accel.update(sc.v, sc.t)
    for cam in CAMERAS:
        m = matrix(cpm, cam)
        plain = sc.render(ndc_to_texture=m)
        # the unit box is no box
        for kw in (dict(clip=unit), dict(clip=unit, accel=accel)):
            assert torch.equal(plain.view(torch.int32), sc.render(ndc_to_texture=m, **kw).view(torch.int32)), (cam, kw.keys())
        # camera mode with a box = buffer mode fed the numpy slab test's entry / exit points (and skipping changes neither)
        o, f = camera_segments(m, W, H)
        ent, ext, hit = clip_segment_box(o, f, lo, hi)
        wcol = hit.astype(F32)[..., None]
        e4 = torch.from_numpy(np.concatenate([ent, wcol], -1)).to(ctx.device)
        x4 = torch.from_numpy(np.concatenate([ext, wcol], -1)).to(ctx.device)
        clipped = sc.render(ndc_to_texture=m, clip=box)
        buffers = sc.render(entry=e4, exit=x4, ndc_to_texture=np.zeros(16, F32))
        assert np.allclose(clipped.cpu().numpy(), buffers.cpu().numpy(), rtol=1e-5, atol=1e-6), cam
        assert torch.equal(clipped.view(torch.int32), sc.render(ndc_to_texture=m, clip=box, accel=accel).view(torch.int32)), cam
        # buffer mode ignores the box
        assert torch.equal(buffers.view(torch.int32), sc.render(entry=e4, exit=x4, ndc_to_texture=np.zeros(16, F32), clip=unit).view(torch.int32))
        assert torch.equal(buffers.view(torch.int32), sc.render(entry=e4, exit=x4, ndc_to_texture=np.zeros(16, F32), clip=box).view(torch.int32))
        # a ray that misses the box gives (0, 0, 0, 0)
        got = clipped.cpu().numpy()
        if cam != "inside":
            assert (~hit).sum() > 100
        assert (got[~hit] == 0).all() and (got[hit][:, 3] > 0).any()
    # a homogeneous medium: alpha = 1 - (1 - a)^(150 L), L = the ray's length inside the box
    w, h = 33, 29
    m = matrix(cpm, "face-on", w, h)
    vol, lut, lv = const_case(0.02, 0.5)
    hs = Scene(ctx, cpm, vol, lut, ldims=(16, 16, 16))
    o, f = camera_segments(m, w, h)
    ent, ext, hit = clip_segment_box(o, f, lo, hi)
    n, t_incr, _, live = R.sample_counts(ent, ext, hit, (16, 16, 16), 1.0)
    assert live.sum() > 100 and (~live).sum() > 100
    L = np.linalg.norm((ext - ent).astype(np.float64), axis=-1)
    assert live[h // 2, w // 2] and abs(L[h // 2, w // 2] - 0.5) < 1e-3   # the centre ray runs along z: the slab is 0.5 thick there
    img = hs.render(w=w, h=h, ndc_to_texture=m, clip=box).cpu().numpy()
    want_a = 1.0 - (1.0 - float(F32(0.02))) ** (150.0 * L)
    assert (img[~live] == 0).all()
    assert np.allclose(img[live, 3], want_a[live], rtol=1e-5, atol=0)


# ---------------------------------------------------------------------------------------------------------------------- refusals

def test_refusals_write_nothing(ctx, cpm):
    import torch
    sc = Scene(ctx, cpm, volume(cpm, "ragged", np.uint8), tfs(cpm)["band"])
    out = torch.full((16, 16, 4), -7.0, dtype=torch.float32, device=ctx.device)
    good = ctx.render_accel(sc.v, 8)
    good.update(sc.v, sc.t)
    assert raw_render_ex(ctx, cpm, sc, good.h, out) == 0
    assert raw_render_ex(ctx, cpm, sc, None, out, clip=(0.1, 0.1, 0.1, 1, 0.9, 0.9, 0.9, 1)) == 0
    torch.cuda.synchronize()
    out.fill_(-7.0)
    # an accel that was never updated, or only by half (the first update needs both)
    never = ctx.render_accel(sc.v, 8)
    assert raw_render_ex(ctx, cpm, sc, never.h, out) == -1
    assert ctx.lib.cpm_render_accel_update(ctx.h, never.h, sc.v.h, None, ctx._stream()) == -1
    assert ctx.lib.cpm_render_accel_update(ctx.h, never.h, None, sc.t.h, ctx._stream()) == -1
    assert raw_render_ex(ctx, cpm, sc, never.h, out) == -1
    # an accel that saw another volume object (same voxels), another TF object (same texels), other dims, another voxel type
    twin_v, twin_t = ctx.volume_create(sc.vol_np), ctx.tf_create(tfs(cpm)["band"])
    for v, t in ((twin_v, sc.t), (sc.v, twin_t)):
        other = ctx.render_accel(v, 8)
        other.update(v, t)
        assert raw_render_ex(ctx, cpm, sc, other.h, out) == -1
    for vol_np in (volume(cpm, "thin", np.uint8), volume(cpm, "ragged", np.uint16)):
        v = ctx.volume_create(vol_np)
        other = ctx.render_accel(v, 8)
        other.update(v, sc.t)
        assert raw_render_ex(ctx, cpm, sc, other.h, out) == -1
        assert ctx.lib.cpm_render_accel_update(ctx.h, other.h, sc.v.h, None, ctx._stream()) == -1   # nor can it be updated with that volume
    # a TF of another width than the accel saw is another object
    wide = ctx.tf_create(cpm.synthetic.workspace_tf(512))
    other = ctx.render_accel(sc.v, 8)
    other.update(sc.v, wide)
    assert raw_render_ex(ctx, cpm, sc, other.h, out) == -1
    # clip boxes: min >= max on an axis, not finite
    nan, inf = float("nan"), float("inf")
    for clip in ((0.5, 0, 0, 1, 0.5, 1, 1, 1), (0, 0.8, 0, 1, 1, 0.2, 1, 1), (0, 0, nan, 1, 1, 1, 1, 1), (0, 0, 0, 1, 1, inf, 1, 1),
                 (-inf, 0, 0, 1, 1, 1, 1, 1), (0, 0, 0, 1, 1, 1, nan, 1)):
        assert raw_render_ex(ctx, cpm, sc, None, out, clip=clip) == -1, clip
        assert raw_render_ex(ctx, cpm, sc, good.h, out, clip=clip) == -1, clip
    # brick sizes
    h = C.c_void_p()
    for brick in (3, 5, 12, 32):
        assert ctx.lib.cpm_render_accel_create(ctx.h, C.byref(sc.v.desc), brick, C.byref(h)) == -1 and not h.value
    torch.cuda.synchronize()
    assert (out == -7.0).all()
