"""The numpy restatement of the brick analysis and the volume mix (tests/brick_reference.py) on hand-worked cases, and the oracle held
to it over the whole voxel value domain of u8, u16 and f32 volumes: negatives, values above 1, +-inf, NaN of either sign, -0,
subnormals, +-FLT_MAX, unorm16 rounding ties, under the default and four other format mappings.  No GPU."""
import numpy as np
import pytest

import brick_reference as R

F32 = np.float32
NAN_NEG = np.array([0xFFC00000], np.uint32).view(np.float32)[0]
MAPPINGS = [(0.0, 0.0), (1.0 - 65535.0 / 4095.0, 0.0), (0.0, 0.25), (0.0, -0.125), (1.5, 0.0), (1.5, -0.25), (1.0, 0.0)]


def _brick(vals):
    return np.asarray(vals).reshape(1, 1, -1)


@pytest.mark.parametrize("nan", [F32(np.nan), NAN_NEG])
def test_minmax_skips_nan_of_either_sign(nan):
    assert np.signbit(nan) == (nan is NAN_NEG)
    got = R.volume_minmax(_brick(np.array([0.2, 0.9, nan], F32)), 4)
    assert got.tolist() == [[13107, 58982]]
    assert R.volume_minmax(_brick(np.array([nan, nan], F32)), 2).tolist() == [[65535, 0]]  # nothing taken: (FLT_MAX, 0)


def test_minmax_mappings_by_hand():
    b = _brick(np.array([-0.5, 0.25, 0.75, 2.0], F32))
    assert R.volume_minmax(b, 4).tolist() == [[0, 65535]]
    assert R.volume_minmax(b, 4, 0.0, 0.25).tolist() == [[0, 65535]]
    assert R.volume_minmax(_brick(np.array([0.25, 0.5], F32)), 2, 0.0, 0.25).tolist() == [[32768, 49151]]  # 32767.5 -> even
    # scaling > 1 reverses the mapping: (v + 0) * -0.5 -> the largest voxel gives the minimum
    assert R.volume_minmax(_brick(np.array([-1.0, -0.5], F32)), 2, 1.5).tolist() == [[16384, 32768]]  # 16383.75, 32767.5
    # scaling 1: every finite voxel maps to +-0, an infinite one to NaN (skipped)
    inf = F32(np.inf)
    assert R.volume_minmax(_brick(np.array([-inf, 0.5, inf], F32)), 4, 1.0).tolist() == [[0, 0]]
    assert R.volume_minmax(_brick(np.array([-inf, inf], F32)), 2, 1.0).tolist() == [[65535, 0]]
    # u8 / u16 normalise first: 255 * (1 / 255) and 65535 * (1 / 65535) in float32
    assert R.volume_minmax(_brick(np.array([0, 128, 255], np.uint8)), 4).tolist() == [[0, 65535]]
    assert R.volume_minmax(_brick(np.array([0, 4095], np.uint16) * 16), 2, 1.0 - 65535.0 / 4095.0).tolist() == [[0, 65535]]


def test_minmax_clipped_border_bricks_take_only_their_voxels():
    v = np.full((3, 3, 5), 0.5, F32)
    v[:, :, 4] = 0.25  # the x border brick of region 4 holds only these
    got = R.volume_minmax(v, 4)
    assert got.tolist() == [[32768, 32768], [16384, 16384]]


def test_unorm16_ties_go_to_even():
    t = R.unorm16_ties(R.f32_tie_candidates(4000))
    assert t.size > 1000
    p = t * F32(65535)
    assert np.all(p - np.floor(p) == F32(0.5))
    assert np.array_equal(R.to_unorm16(t).astype(np.int64) % 2, np.zeros(t.size, np.int64))
    assert R.unorm16_ties(np.array([0.5], np.float16)).size == 1  # 0.5 * 65535 = 32767.5 exactly
    assert R.unorm16_ties(np.arange(65536, dtype=np.uint16)).size == 0  # u16 / 65535 * 65535 never lands on a tie ...
    assert R.unorm16_ties(np.arange(65536, dtype=np.uint16), 0.0, 0.5 / 65535).size > 0  # ... an offset of half a step does


def test_difference_by_hand():
    a = np.zeros((64, 64, 64), np.uint8)
    assert R.volume_difference(a, a + 255, 64).tolist() == [1.0]
    assert R.volume_difference(a.astype(np.uint16), a.astype(np.uint16) + 65535, 64).tolist() == [1.0]
    # clipped bricks divide by region^3 too
    assert R.volume_difference(np.zeros((1, 1, 3), np.uint8), np.full((1, 1, 3), 255, np.uint8), 2).tolist() == [0.25, 0.125]
    # f16 extremes over a 16^3 brick: 4096 terms of 131008, summed exactly just below 2^53
    h = np.full((16, 16, 16), -65504, np.float16)
    assert R.volume_difference(h, -h, 16).tolist() == [131008.0]
    assert R.volume_difference(h.astype(F32), -h.astype(F32), 16).tolist() == [131008.0]
    # non-finite terms: NaN wins over inf, inf - inf is NaN
    inf = F32(np.inf)
    assert np.isinf(R.volume_difference(_brick(np.array([0, 1], F32)), _brick(np.array([inf, 1], F32)), 2)[0])
    assert np.isnan(R.volume_difference(_brick(np.array([inf, 0], F32)), _brick(np.array([inf, np.nan], F32)), 2)[0])
    assert np.isnan(R.volume_difference(_brick(np.array([inf], F32)), _brick(np.array([inf], F32)), 1)[0])
    assert R.volume_difference(_brick(np.array([inf], F32)), _brick(np.array([-inf], F32)), 1)[0] == inf


def test_difference_is_the_sequential_double_sum():
    rng = np.random.default_rng(5)
    a = (rng.random((8, 8, 8)) * F32(1e-16)).astype(F32)
    a[0, 0, 0] = 1.0  # first in the brick: the sequential sum loses every later term, a pairwise one does not
    b = np.zeros_like(a)
    want = 0.0
    for z in range(8):
        for y in range(8):
            for x in range(8):
                want += abs(float(b[z, y, x]) - float(a[z, y, x]))
    got = R.volume_difference(a, b, 8)
    assert got.tolist() == [np.float32((want / 512.0) / 1.0)]
    pairwise = np.abs(b.astype(np.float64) - a.astype(np.float64)).sum()
    assert pairwise != want  # this data tells the two orders apart


def test_mix_by_hand():
    u8 = R.volume_mix(np.array([0, 0, 1, 255], np.uint8), np.array([255, 1, 2, 0], np.uint8), 0.5)
    assert u8.tolist() == [128, 0, 2, 128]  # 127.5 -> 128, 0.5 -> 0, 1.5 -> 2
    inf = F32(np.inf)
    f = R.volume_mix(np.array([1.0, 1.0, inf], F32), np.array([inf, 2.0, 1.0], F32), 0.0)
    assert np.isnan(f[0]) and f[1] == 1.0 and f[2] == inf  # inf * 0 = NaN, as the GLSL formula gives
    h = R.volume_mix(np.array([65504, 1], np.float16), np.array([65504, 0], np.float16), 0.25)
    assert h.dtype == np.float16 and h[0] == np.float16(65504) and h[1] == np.float16(0.75)


def _cases():
    for dt in (np.uint8, np.uint16, np.float32):
        for shape, region in [((18, 20, 48), 1), ((18, 20, 37), 3), ((18, 20, 40), 4), ((19, 21, 37), 5), ((18, 20, 40), 8),
                              ((18, 20, 37), 17), ((18, 20, 40), 64)]:
            yield dt, shape, region


@pytest.mark.parametrize("dtype,shape,region", list(_cases()))
def test_oracle_matches_the_reference(oracle, dtype, shape, region):
    seed = region + shape[2] + np.dtype(dtype).itemsize
    for k, (sc, off) in enumerate(MAPPINGS):
        if dtype == np.float32:
            extra = R.unorm16_ties(R.f32_tie_candidates(400, sc, off, seed), sc, off)
        else:
            extra = R.unorm16_ties(np.arange(np.iinfo(dtype).max + 1).astype(dtype), sc, off)
        a = R.value_volume(dtype, shape, seed + k, extra, special_slices=9)  # (z >= 9: bricks of finite differences)
        b = R.value_volume(dtype, shape, seed + k + 100, extra, nan_block=3, special_slices=9)
        got = oracle.volume_minmax(oracle.volume(a, sc, off), region)
        assert np.array_equal(got, R.volume_minmax(a, region, sc, off)), (sc, off)
        want = R.volume_difference(a, b, region)
        assert R.same_or_both_nan(oracle.volume_difference(oracle.volume(a, sc, off), oracle.volume(b, sc, off), region), want)
    if dtype == np.float32:
        assert np.isnan(want).any() and (region > 8 or np.isfinite(want).any())


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.float32])
def test_oracle_mix_matches_the_reference(oracle, dtype):
    if dtype == np.uint8:
        x, y = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
        x, y = x.astype(np.uint8), y.astype(np.uint8)
    elif dtype == np.uint16:
        rng = np.random.default_rng(1)
        e = np.array([0, 1, 2, 32767, 32768, 65534, 65535], np.uint16)
        x, y = np.meshgrid(e, e, indexing="ij")
        x = np.concatenate([x.ravel(), rng.integers(0, 65536, 20000).astype(np.uint16)])
        y = np.concatenate([y.ravel(), rng.integers(0, 65536, 20000).astype(np.uint16)])
    else:
        s = np.concatenate([R.specials(np.float32), np.random.default_rng(2).random(200, dtype=F32) * 4 - 2])
        x, y = np.meshgrid(s, s, indexing="ij")
    x, y = np.ascontiguousarray(x).reshape(1, 1, -1), np.ascontiguousarray(y).reshape(1, 1, -1)
    for w in (0.0, 0.25, 0.5, 0.3125, 0.999, 1.0):
        got = oracle.volume_mix(oracle.volume(x), oracle.volume(y), w, x)
        assert R.same_or_both_nan(got, R.volume_mix(x, y, w)), w
