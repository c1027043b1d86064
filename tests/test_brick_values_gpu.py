"""cpm_volume_minmax, cpm_volume_difference, cpm_volume_step and cpm_volume_mix over the whole voxel value domain, held to the numpy
restatement in tests/brick_reference.py (not to the oracle) bit for bit, NaN matching any NaN.

  * every brick case runs with the streaming brick-row kernels allowed and forbidden (cpm_debug_set_brick_streaming), and checks
    through the profiling hook that the launch took the form the dispatch rule names: rows 16-byte aligned, the LDS slots within
    48 KiB (u8 x = 6144 / 6160 at region 1, 3072 / 3088 for the one-pass step), f32 differences and f16 ones past region 16 per brick;
  * f32 and f16 volumes with negatives, values above 1, +-inf, NaN of either sign, -0, subnormals, +-FLT_MAX (+-65504), NaN-only bricks
    and unorm16 rounding ties; u8 / u16 with 0 and the maximum; under the default mapping, a 12-bit-in-16 one, non-zero offsets, a
    format_scaling above 1 (reversed) and format_scaling 1 (infinite voxels map to NaN);
  * the exactness bounds of the sums, cpm_volume_step with cur and next in different mappings, the mix of every u8 pair and every
    binary16 pattern, and one check that the importance grid built from a NaN-holding f32 volume does not depend on the form.
Nothing here traces photons through a volume with non-finite voxels."""
import numpy as np
import pytest

import brick_reference as R

pytestmark = pytest.mark.gpu
F32 = np.float32
MAPPINGS = [(0.0, 0.0), (1.0 - 65535.0 / 4095.0, 0.0), (0.0, 0.25), (0.0, -0.125), (1.5, 0.0), (1.5, -0.25), (1.0, 0.0)]
LDS_BYTES = 48 * 1024
ALL_F16 = np.arange(1 << 16, dtype=np.uint32).astype(np.uint16).view(np.float16)


def _n(t, dtype=None):
    a = t.detach().cpu().numpy()
    return a.view(dtype) if dtype is not None else a


def _volume(ctx, cpm, arr, mapping=(0.0, 0.0)):
    B = cpm.binding
    desc = B.default_volume_desc(arr.shape[::-1], B._np_dtype_code(arr.dtype))
    desc.format_scaling, desc.format_offset = mapping
    return ctx.volume_create(np.ascontiguousarray(arr), desc)


def _streams(dtype, dx, region, op, same_mapping=True):
    """Whether the dispatch takes brick_row_kernel for `op` (with streaming allowed)."""
    dtype = np.dtype(dtype)
    ox = (dx + region - 1) // region
    aligned = dx * dtype.itemsize % 16 == 0
    if op == "minmax":
        return aligned and ox * 8 <= LDS_BYTES
    pair = aligned and dtype != np.float32 and (dtype != np.float16 or region <= 16)
    if op == "difference":
        return pair and ox * 8 <= LDS_BYTES
    return pair and ox * 16 <= LDS_BYTES and same_mapping


def _bricks(ctx, cpm, a, b, region, streaming, ma=(0.0, 0.0), mb=None):
    """min/max of a, mean |b - a|, and the one-pass step (a -> b); and the kernels each call launched."""
    torch = ctx.torch
    mb = ma if mb is None else mb
    va, vb = _volume(ctx, cpm, a, ma), _volume(ctx, cpm, b, mb)
    nb = R.n_bricks(a.shape, region)
    mm = torch.zeros((nb, 2), dtype=torch.int16, device=ctx.device)
    diff = torch.full((nb,), -1.0, dtype=torch.float32, device=ctx.device)
    smm = torch.zeros_like(mm)
    sdiff = torch.full_like(diff, -1.0)
    launched = {}
    ctx.lib.cpm_debug_set_brick_streaming(ctx.h, int(streaming))
    ctx.profile_enable(True)
    try:
        for op, call in (("minmax", lambda: ctx.volume_minmax(va, region, mm)),
                         ("difference", lambda: ctx.volume_difference(va, vb, region, diff)),
                         ("step", lambda: ctx.volume_step(va, vb, region, sdiff, smm))):
            torch.cuda.synchronize()
            ctx.profile_reset()
            call()
            torch.cuda.synchronize()
            launched[op] = set(ctx.profile_collect())
    finally:
        ctx.profile_enable(False)
        ctx.lib.cpm_debug_set_brick_streaming(ctx.h, 1)
    return dict(mm=_n(mm, np.uint16).copy(), diff=_n(diff).copy(), smm=_n(smm, np.uint16).copy(), sdiff=_n(sdiff).copy(),
                launched=launched)


def _row_kernel(names, mode):
    return any("brick_row_kernel" in n and f", {mode}>" in n for n in names)


def _check(got, a, b, region, streaming, ma=(0.0, 0.0), mb=None):
    mb = ma if mb is None else mb
    want_mm, want_next = R.volume_minmax(a, region, *ma), R.volume_minmax(b, region, *mb)
    want_diff = R.volume_difference(a, b, region)
    bad = np.nonzero((got["mm"] != want_mm).any(1))[0]
    assert bad.size == 0, f"min/max: {bad.size} bricks, first {bad[0]}: {got['mm'][bad[0]]} != {want_mm[bad[0]]}"
    assert np.array_equal(got["smm"], want_next), "step: min/max of next"
    assert R.same_or_both_nan(got["diff"], want_diff), "difference"
    assert R.same_or_both_nan(got["sdiff"], want_diff), "step: difference"
    L = got["launched"]
    dx = a.shape[2]
    assert _row_kernel(L["minmax"], 0) == (streaming and _streams(a.dtype, dx, region, "minmax")), L
    assert _row_kernel(L["difference"], 1) == (streaming and _streams(a.dtype, dx, region, "difference")), L
    assert _row_kernel(L["step"], 2) == (streaming and _streams(a.dtype, dx, region, "step", tuple(ma) == tuple(mb))), L
    if not streaming:
        assert not any("brick_row_kernel" in n for names in L.values() for n in names), L


def _both_forms(ctx, cpm, a, b, region, ma=(0.0, 0.0), mb=None):
    runs = [_bricks(ctx, cpm, a, b, region, s, ma, mb) for s in (True, False)]
    for s, got in zip((True, False), runs):
        _check(got, a, b, region, s, ma, mb)
    for k in ("mm", "smm", "diff", "sdiff"):
        assert R.same_or_both_nan(runs[0][k], runs[1][k]), k
    return runs


def _ties(dtype, mapping, seed):
    if dtype == np.float32:
        return R.unorm16_ties(R.f32_tie_candidates(400, *mapping, seed), *mapping)
    if dtype == np.float16:
        return R.unorm16_ties(ALL_F16, *mapping)
    return R.unorm16_ties(np.arange(np.iinfo(dtype).max + 1).astype(dtype), *mapping)


# x sizes on both sides of the 16-byte row rule
X_SIZES = {np.uint8: (48, 40), np.uint16: (40, 36), np.float16: (40, 36), np.float32: (40, 38)}


@pytest.mark.parametrize("region", [1, 3, 4, 5, 8, 16, 17, 32, 64])
@pytest.mark.parametrize("aligned", [True, False])
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.float16, np.float32], ids=["u8", "u16", "f16", "f32"])
def test_bricks_over_the_value_domain(ctx, cpm, dtype, aligned, region):
    """(18, 20, x) volumes: region 64 is larger than the volume; 17 is f16's first per-brick region."""
    shape = (18, 20, X_SIZES[dtype][0 if aligned else 1])
    assert (shape[2] * np.dtype(dtype).itemsize % 16 == 0) == aligned
    for k, mapping in enumerate(MAPPINGS):
        seed = 1000 * region + 10 * k + int(aligned)
        extra = _ties(dtype, mapping, seed)
        a = R.value_volume(dtype, shape, seed, extra, special_slices=12)
        b = R.value_volume(dtype, shape, seed + 1, extra, nan_block=3, special_slices=12)
        runs = _both_forms(ctx, cpm, a, b, region, mapping)
        if np.dtype(dtype).kind == "f" and region <= 8:  # the data reach what they are meant to
            assert np.isnan(runs[0]["diff"]).any() and np.isfinite(runs[0]["diff"]).any()
            assert (runs[0]["mm"] == (65535, 0)).all(1).any()  # NaN-only bricks


@pytest.mark.parametrize("nan_bits", [0x7FC00000, 0xFFC00000])
@pytest.mark.parametrize("dx", [40, 38])
def test_f32_minmax_skips_nan_of_either_sign(ctx, cpm, nan_bits, dx):
    """Bricks {0.2, 0.9, NaN}: (13107, 58982) in both forms, whatever the NaN's sign; NaN-only bricks (65535, 0)."""
    a = np.zeros((4, 4, dx), F32)
    a[..., 0::4], a[..., 1::4] = F32(0.2), F32(0.9)
    a.view(np.uint32)[..., 2::4] = nan_bits
    a.view(np.uint32)[..., 3::4] = nan_bits
    a.view(np.uint32)[:, :, -4:] = nan_bits  # the last brick of the row is NaN only (dx 38: clipped to two voxels)
    runs = _both_forms(ctx, cpm, a, a, 4)
    want = np.tile([13107, 58982], (R.n_bricks(a.shape, 4), 1)).astype(np.uint16)  # (0.9 * 65535 = 58981.5 in float32: a tie)
    want[9::10] = (65535, 0)
    assert np.array_equal(runs[0]["mm"], want)


@pytest.mark.parametrize("dtype", [np.float32, np.float16], ids=["f32", "f16"])
@pytest.mark.parametrize("aligned", [True, False])
def test_scaling_one_with_infinite_voxels(ctx, cpm, dtype, aligned):
    """format_scaling 1: every finite voxel maps to +-0 and an infinite one to inf * 0 = NaN, which the min / max skip; a brick that
    holds -inf, a finite value and +inf is (0, 0), one of infinities only (65535, 0)."""
    dx = X_SIZES[dtype][0 if aligned else 1]
    a = np.full((4, 4, dx), 0.5, dtype)
    a[..., 0::4], a[..., 1::4] = -np.inf, np.inf
    a[:, :, 8:12] = np.inf
    a[:, :, 12:16] = -np.inf
    runs = _both_forms(ctx, cpm, a, a, 4, (1.0, 0.0))
    mm = runs[0]["mm"].reshape(1, 1, -1, 2)
    assert (mm[0, 0, :2] == (0, 0)).all() and (mm[0, 0, 2:4] == (65535, 0)).all()


@pytest.mark.parametrize("dx,region,op", [(6144, 1, "minmax"), (6160, 1, "minmax"), (3072, 1, "step"), (3088, 1, "step"),
                                          (6144 * 3, 3, "minmax"), (6160 * 3, 3, "minmax")])
def test_u8_rows_at_the_lds_limit(ctx, cpm, dx, region, op):
    """The streaming forms keep 8 (min/max, difference) or 16 (step) bytes of LDS per brick of a row: 6144 / 3072 bricks fit in 48 KiB,
    the next aligned size falls back to the per-brick kernels."""
    shape = (2, 3, dx)
    a = R.value_volume(np.uint8, shape, dx)
    b = R.value_volume(np.uint8, shape, dx + 1)
    runs = _both_forms(ctx, cpm, a, b, region)
    fits = (dx // region) * (8 if op == "minmax" else 16) <= LDS_BYTES
    assert _row_kernel(runs[0]["launched"][op], 0 if op == "minmax" else 2) == fits


def test_exactness_bounds_of_the_sums(ctx, cpm):
    """f16: 16^3 terms of the largest finite difference (65504 - -65504) sum to just below 2^53 and the mean is exactly 131008, in the
    streaming form's 2^-24 fixed point as in the per-brick double sum; u8 and u16 64^3 bricks of maximal differences give exactly 1."""
    h = np.full((16, 16, 32), -65504, np.float16)
    runs = _both_forms(ctx, cpm, h, -h, 16)
    assert runs[0]["diff"].tolist() == [131008.0, 131008.0] and runs[0]["sdiff"].tolist() == [131008.0, 131008.0]
    assert _row_kernel(runs[0]["launched"]["difference"], 1)
    for dtype in (np.uint8, np.uint16):
        a = np.zeros((64, 64, 64), dtype)
        runs = _both_forms(ctx, cpm, a, a + np.iinfo(dtype).max, 64)
        assert runs[0]["diff"].tolist() == [1.0] and runs[0]["sdiff"].tolist() == [1.0]
        assert runs[0]["smm"].tolist() == [[65535, 65535]] and runs[0]["mm"].tolist() == [[0, 0]]


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.float16, np.float32], ids=["u8", "u16", "f16", "f32"])
@pytest.mark.parametrize("region", [4, 8])
def test_step_with_cur_and_next_in_different_mappings(ctx, cpm, dtype, region):
    """cpm_volume_step's min / max are next's, in next's mapping: the one-pass form needs equal descs and the step falls back to two
    launches otherwise."""
    shape = (18, 20, X_SIZES[dtype][0])
    a = R.value_volume(dtype, shape, region, special_slices=12)
    b = R.value_volume(dtype, shape, region + 7, nan_block=3, special_slices=6)
    if np.dtype(dtype).kind == "f":  # finite values into [0.175, 0.675): the bricks past z = 8 span less than [0, 1] in any mapping
        b = np.where(np.abs(b) < 2, b * dtype(0.25) + dtype(0.3), b).astype(dtype)
    for ma, mb in (((0.0, 0.0), (0.0, 0.25)), ((0.0, 0.25), (0.0, -0.125)), ((0.0, 0.0), (1.5, -0.25))):
        runs = _both_forms(ctx, cpm, a, b, region, ma, mb)
        assert not _row_kernel(runs[0]["launched"]["step"], 2)
        assert not np.array_equal(runs[0]["smm"], R.volume_minmax(b, region, *ma))  # (the mappings tell apart)


# ---- cpm_volume_mix (no per-brick form: the streaming hook does not apply)

WEIGHTS = (0.0, 0.25, 0.5, 0.3125, 0.999, 1.0)


def _mix(ctx, cpm, x, y, w):
    out = ctx.volume_create(np.zeros_like(x))
    ctx.volume_mix(_volume(ctx, cpm, x), _volume(ctx, cpm, y), w, out)
    ctx.torch.cuda.synchronize()
    return out.download()


def test_mix_u8_every_pair(ctx, cpm):
    x, y = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    x, y = x.astype(np.uint8).reshape(16, 64, 64), y.astype(np.uint8).reshape(16, 64, 64)
    for w in WEIGHTS:
        got = _mix(ctx, cpm, x, y, w)
        assert np.array_equal(got, R.volume_mix(x, y, w)), w


def test_mix_u16_extremes_and_a_sample(ctx, cpm):
    rng = np.random.default_rng(16)
    e = np.array([0, 1, 2, 32767, 32768, 65534, 65535], np.uint16)
    ex, ey = np.meshgrid(e, e, indexing="ij")
    x = rng.integers(0, 65536, 1 << 16).astype(np.uint16)
    y = rng.integers(0, 65536, 1 << 16).astype(np.uint16)
    x[: ex.size], y[: ey.size] = ex.ravel(), ey.ravel()
    x, y = x.reshape(16, 64, 64), y.reshape(16, 64, 64)
    for w in WEIGHTS:
        assert np.array_equal(_mix(ctx, cpm, x, y, w), R.volume_mix(x, y, w)), w


def test_mix_f16_every_pattern(ctx, cpm):
    x = ALL_F16.reshape(16, 64, 64)
    partners = np.array([0x0000, 0x3C00, 0xBC00, 0x7C00, 0x7E00, 0x0001], np.uint16).view(np.float16)
    for p in partners:
        y = np.full_like(x, p)
        for w in WEIGHTS:
            for u, v in ((x, y), (y, x)):
                got = _mix(ctx, cpm, u, v, w)
                assert got.dtype == np.float16 and R.same_or_both_nan(got, R.volume_mix(u, v, w)), (p, w)


def test_mix_f32_special_values(ctx, cpm):
    rng = np.random.default_rng(32)
    s = np.concatenate([R.specials(np.float32), rng.random(256, dtype=F32) * F32(4) - F32(2)])[:256]
    x, y = np.meshgrid(s, s, indexing="ij")
    x, y = x.reshape(16, 64, 64), y.reshape(16, 64, 64)
    for w in WEIGHTS:
        want = R.volume_mix(x, y, w)
        assert R.same_or_both_nan(_mix(ctx, cpm, x, y, w), want), w
    assert np.isnan(R.volume_mix(np.array([1.0], F32), np.array([np.inf], F32), 0.0)).all()  # w = 0, y = inf: inf * 0


# ---- through to the importance grid (no trace)

def test_importance_from_a_nan_holding_volume(ctx, cpm, oracle):
    """min/max of an f32 volume with NaN voxels (and NaN-only bricks), merged with the previous step's and weighted by a finite
    difference grid in cpm_importance_tf: the same bits with the streaming form on and off, and the oracle's importance of the
    reference's bricks."""
    torch = ctx.torch
    shape, region = (32, 32, 64), 8
    rng = np.random.default_rng(8)
    cur = R.value_volume(np.float32, shape, 81, p=0.05)
    prev = (F32(0.3) + F32(0.05) * rng.random(shape, dtype=F32)).astype(F32)
    moved = np.roll(prev, 3, axis=2)
    pos = np.array([0.0, 0.5, 1.0], F32)
    col = np.array([[0, 0, 0, 0], [0.2, 0.1, 0.1, 0.3], [0.9, 0.5, 0.4, 1.0]], F32)
    nb = R.n_bricks(shape, region)
    out = []
    for streaming in (1, 0):
        ctx.lib.cpm_debug_set_brick_streaming(ctx.h, streaming)
        try:
            mm = torch.zeros((nb, 2), dtype=torch.int16, device=ctx.device)
            pm = torch.zeros_like(mm)
            diff = torch.zeros(nb, dtype=torch.float32, device=ctx.device)
            imp = torch.full((nb,), -1.0, dtype=torch.float32, device=ctx.device)
            ctx.volume_minmax(_volume(ctx, cpm, cur), region, mm)
            ctx.volume_minmax(_volume(ctx, cpm, prev), region, pm)
            ctx.volume_difference(_volume(ctx, cpm, prev), _volume(ctx, cpm, moved), region, diff)
            ctx.importance_tf(mm, nb, pos, col, imp, prev_minmax=pm, volume_diff=diff)
            torch.cuda.synchronize()
            out.append((_n(mm, np.uint16).copy(), _n(imp).copy()))
        finally:
            ctx.lib.cpm_debug_set_brick_streaming(ctx.h, 1)
    want_mm, want_pm = R.volume_minmax(cur, region), R.volume_minmax(prev, region)
    want = oracle.importance_tf(want_mm, pos, col, prev=want_pm, diff=R.volume_difference(prev, moved, region))
    for mm, imp in out:
        assert np.array_equal(mm, want_mm)
        assert np.array_equal(R.bits(imp), R.bits(want))
    assert np.isfinite(want).all() and len(np.unique(want)) > 10
