"""The shaded raycaster's numpy restatement (tests/render_shaded_reference.py) without a GPU: its gradient sampler held to the oracle,
mode NONE against the unshaded restatement, the closed forms of a ramp and of a constant volume, and what the GPU comparison rests on --
the exclusion cap and the float32 deviation of the shading formulas on that test's own inputs (tests/render_shaded_cases.py)."""
import numpy as np
import pytest

import render_reference as R
import render_shaded_cases as K
import render_shaded_reference as RS

F32 = np.float32


def ramp_volume(axis, dims=(16, 12, 10), slope=3):
    """uint16 voxels slope * index along `axis` (0 = x): the normalised value rises by slope / 65535 per voxel"""
    idx = np.arange(dims[axis], dtype=np.uint16) * np.uint16(slope)
    shape = [1, 1, 1]
    shape[2 - axis] = dims[axis]
    return np.broadcast_to(idx.reshape(shape), dims[::-1]).copy()


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.float16, np.float32])
def test_gradient_is_six_oracle_samples(oracle, dtype):
    rng = np.random.default_rng(23)
    shape = (7, 9, 11)
    vol = rng.integers(0, np.iinfo(dtype).max + 1, shape, dtype=dtype) if np.dtype(dtype).kind == "u" else rng.random(shape, dtype=F32).astype(dtype)
    ov = oracle.volume(vol.astype(F32) if dtype == np.float16 else vol)   # binary16 voxels are widened first: the F32 volume's bits
    p = rng.uniform(-0.05, 1.05, (300, 3)).astype(F32)
    g = RS.gradient(vol, p)
    dims = shape[::-1]
    for a in range(3):
        h = F32(1) / F32(dims[a])
        want = []
        for q in p:
            hi, lo = q.copy(), q.copy()
            hi[a], lo[a] = q[a] + h, q[a] - h   # float32: one add
            d = F32(oracle.lib.cpmo_sample_volume(ov, *map(float, hi))) - F32(oracle.lib.cpmo_sample_volume(ov, *map(float, lo)))
            want.append(F32(d) * (F32(0.5) * F32(dims[a])))
        assert np.array_equal(g[:, a].view(np.uint32), np.array(want, F32).view(np.uint32)), a


def test_mode_none_is_the_unshaded_restatement(cpm):
    vol, lut, lv, kw = K.inputs(cpm, np.uint8, 4, "camera")
    want, amb = R.render(vol, lut, lv, K.LIGHT_DIMS, 4, K.W, K.H, **kw)
    for sh in (None, K.shading("none")):
        got, amb2 = RS.render(vol, lut, lv, K.LIGHT_DIMS, 4, K.W, K.H, shading=sh, **kw)
        assert np.array_equal(got, want) and np.array_equal(amb, amb2) and (got[..., 3] > 0).any()


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_ramp_gradient_is_the_slope(axis):
    dims = (16, 12, 10)
    vol = ramp_volume(axis, dims)
    rng = np.random.default_rng(4)
    # interior: both offset samples keep a full footprint, p +- 1 / dim within [1 / (2 dim), 1 - 1 / (2 dim)]
    lo = 1.5 / np.array(dims) + 1e-3
    p = (lo + rng.random((500, 3)) * (1.0 - 2 * lo)).astype(F32)
    g = RS.gradient(vol, p)
    slope = 3.0 / 65535.0 * dims[axis]   # per unit of texture space
    assert np.allclose(g[:, axis], slope, rtol=2e-4, atol=0)   # float32 differences of values near 7e-4: a few 1e-5 relative
    for other in set(range(3)) - {axis}:
        assert (g[:, other] == 0).all()
    # at the outermost voxel centre the sampler clamps the outer sample: one-sided, half the magnitude
    e = p.copy()
    e[:, axis] = F32(0.5 / dims[axis])
    assert np.allclose(RS.gradient(vol, e)[:, axis], 0.5 * slope, rtol=2e-4, atol=0)


def test_constant_volume_is_ambient_in_every_mode():
    vol = np.full((10, 12, 14), 100, np.uint8)
    lut = np.tile(np.array([0.8, 0.5, 0.25, 0.03], F32), (64, 1))
    lv = np.full(8 ** 3, 0.5, F32)
    m = np.eye(4, dtype=F32).reshape(16)
    e = np.zeros((3, 5, 4), F32)
    x = np.zeros((3, 5, 4), F32)
    e[...] = (0.3, 0.4, 0.0, 1.0)
    x[...] = (0.6, 0.5, 1.0, 1.0)
    rng = np.random.default_rng(0)
    assert (RS.gradient(vol, rng.uniform(-0.1, 1.1, (200, 3)).astype(F32)) == 0).all()
    want, _ = RS.render(vol, lut, lv, (8, 8, 8), 1, 5, 3, shading=K.shading("ambient"), entry=e, exit=x, ndc_to_texture=m)
    plain, _ = R.render(vol, lut, lv, (8, 8, 8), 1, 5, 3, entry=e, exit=x)
    assert np.allclose(want[..., :3], plain[..., :3] * np.array(K.shading("ambient")["ambient"], F32), rtol=1e-6, atol=0)
    for mode in K.MODE_NAMES:
        got, _ = RS.render(vol, lut, lv, (8, 8, 8), 1, 5, 3, shading=K.shading(mode), entry=e, exit=x, ndc_to_texture=m)
        assert np.array_equal(got, want) and (got[..., :3] > 0).all(), mode


def test_shading_terms_on_hand_built_vectors():
    """N, L, V chosen by hand: the five modes' sums, two-sidedness, and the zero gradient"""
    sh = dict(mode="phong", texture_to_world=None, light_position=(0.5, 0.5, 10.5), ambient=(0.1,) * 3, diffuse=(0.5,) * 3,
              specular=(0.25,) * 3, shininess=8.0)
    c = np.array([[1.0, 0.5, 0.25]], F32)
    p = np.array([[0.5, 0.5, 0.5]], F32)
    d = np.array([[0.0, 0.0, -1.0]], F32)            # V = +z = L
    c60 = np.array([[0.0, np.sqrt(3.0) / 2, 0.5]], F32)   # N 60 degrees off L: N.L = 1/2, R.V = 2 (1/4) - 1 < 0, N.H = 1/2
    want = {"ambient": 0.1 * c, "diffuse": 0.1 * c + 0.5 * c * 0.5, "specular": 0.1 * c + 0.0,
            "blinn_phong": 0.1 * c + 0.5 * c * 0.5 + 0.25 * 0.5 ** 8, "phong": 0.1 * c + 0.5 * c * 0.5}
    for mode, w in want.items():
        for g in (c60, -c60, 1e-30 * c60, 1e30 * c60):
            assert np.allclose(RS.shade(c, g.astype(F32), p, d, dict(sh, mode=mode)), w, rtol=1e-6, atol=1e-9), mode
        assert np.allclose(RS.shade(c, np.zeros((1, 3), F32), p, d, dict(sh, mode=mode)), 0.1 * c, rtol=1e-7), mode
    head_on = np.array([[0.0, 0.0, 2.0]], F32)
    assert np.allclose(RS.shade(c, head_on, p, d, sh), 0.1 * c + 0.5 * c + 0.25, rtol=1e-6)


def test_gpu_inputs_meet_the_exclusion_cap_and_the_measured_tolerance(cpm):
    """On the GPU test's own inputs, from the restatement alone: the pixels whose early termination is ambiguous stay under the cap, and
    the shading formulas in float32 deviate from float64 by no more than the figure the GPU tolerance is derived from."""
    worst = 0.0
    for dtype in K.DTYPES:
        for channels in K.CHANNELS:
            for rays in K.RAYS:
                vol, lut, lv, kw = K.inputs(cpm, dtype, channels, rays)
                for mode in K.MODE_NAMES:
                    w64, amb = K.reference(vol, lut, lv, channels, kw, mode)
                    live = w64[..., 3] > 0
                    assert live.sum() > 1000 and amb.sum() <= K.MAX_AMBIGUOUS * live.sum(), (dtype, channels, rays, mode, amb.sum(), live.sum())
                    w32, _ = K.reference(vol, lut, lv, channels, kw, mode, np.float32)
                    worst = max(worst, RS.needed_rtol(w32[~amb], w64[~amb], K.ATOL))
    print("float32 shading needs rtol", worst, "at atol", K.ATOL)
    assert worst <= K.MEASURED_F32_RTOL
    assert K.RTOL == max(1e-5, 4 * K.MEASURED_F32_RTOL) and K.ATOL == 1e-6
