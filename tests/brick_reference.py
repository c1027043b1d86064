"""numpy restatement of the brick analysis (min / max bricks, mean |b - a| bricks) and of the volume mix, to the bit.

Independent of the oracle: what the tests hold both the HIP kernels and the oracle's C to.

  * min / max: each voxel mapped in float32 with separate roundings, s = raw * norm, then (s + offset) * (1 - scaling) (norm 1/255,
    1/65535 or 1; binary16 widened first); a NaN-skipping min seeded with FLT_MAX and a NaN-skipping max seeded with 0 (fmin / fmax);
    rint(clip(v, 0, 1) * 65535) in float32, ties to even.  Clipped border bricks take only their real voxels.
  * difference: |b - a| of the raw values over region^3 (also for clipped bricks) and the format's range (255, 65535, 1).  Integers
    sum exactly; floats in float64, sequentially in x-fastest z-y-x order within the brick (np.cumsum, not the pairwise np.sum).
  * mix (volume_mix.frag): unorm formats rint(clip(x / max * (1 - w) + y / max * w, 0, 1) * max) in float32; float32 x * (1 - w) + y * w;
    binary16 the float32 formula on the widened values, rounded to nearest even.

Brick b of a volume of x size dx lies at gx + ox * (gy + oy * gz); volumes are numpy arrays indexed [z, y, x].
"""
import numpy as np

F32 = np.float32
FLT_MAX = np.finfo(np.float32).max
RANGE = {np.dtype(np.uint8): 255.0, np.dtype(np.uint16): 65535.0, np.dtype(np.float32): 1.0, np.dtype(np.float16): 1.0}


def norm(dtype):
    dtype = np.dtype(dtype)
    if dtype == np.uint8:
        return F32(1) / F32(255)
    if dtype == np.uint16:
        return F32(1) / F32(65535)
    return F32(1)


def mapped(raw, format_scaling=0.0, format_offset=0.0):
    """Each voxel's float32 value under the volume's format mapping (NaN where the mapping gives NaN, e.g. inf * 0)."""
    raw = np.asarray(raw)
    with np.errstate(all="ignore"):
        s = raw.astype(F32) * norm(raw.dtype)
        return (s + F32(format_offset)) * (F32(1) - F32(format_scaling))


def to_unorm16(v):
    """rint(clip(v, 0, 1) * 65535) in float32, as uint16."""
    v = np.asarray(v, F32)
    return np.rint(np.minimum(np.maximum(v, F32(0)), F32(1)) * F32(65535)).astype(np.uint16)


def brick_dims(shape, region):
    """(oz, oy, ox) of a volume of numpy shape (dz, dy, dx)."""
    return tuple((d + region - 1) // region for d in shape)


def n_bricks(shape, region):
    return int(np.prod(brick_dims(shape, region)))


def _blocks(v, region, fill):
    """v padded with `fill` to whole bricks, as [brick, voxel of the brick in x-fastest z-y-x order]."""
    oz, oy, ox = brick_dims(v.shape, region)
    R = region
    p = np.full((oz * R, oy * R, ox * R), fill, v.dtype)
    p[: v.shape[0], : v.shape[1], : v.shape[2]] = v
    return p.reshape(oz, R, oy, R, ox, R).transpose(0, 2, 4, 1, 3, 5).reshape(oz * oy * ox, R * R * R)


def volume_minmax(vol, region, format_scaling=0.0, format_offset=0.0):
    """uint16 [n_bricks, 2]: the (min, max) of each brick's mapped values."""
    m = _blocks(mapped(vol, format_scaling, format_offset), region, F32(np.nan))  # padding: NaN, which fmin / fmax skip
    lo = np.fmin.reduce(m, axis=1, initial=FLT_MAX)
    hi = np.fmax.reduce(m, axis=1, initial=F32(0))
    return np.stack([to_unorm16(lo), to_unorm16(hi)], 1)


def volume_difference(a, b, region):
    """float32 [n_bricks]: mean |b - a| per brick over region^3, divided by the format's range."""
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape
    cnt = float(region) ** 3
    rng = RANGE[a.dtype]
    if a.dtype in (np.uint8, np.uint16):
        d = np.abs(b.astype(np.int64) - a.astype(np.int64))
        s = _blocks(d, region, 0).sum(axis=1).astype(np.float64)  # exact
    else:
        with np.errstate(all="ignore"):
            d = np.abs(b.astype(np.float64) - a.astype(np.float64))
        s = np.cumsum(_blocks(d, region, 0.0), axis=1)[:, -1]  # the sequential sum; +0 padding terms change nothing
    with np.errstate(all="ignore"):
        return ((s / cnt) / rng).astype(F32)


def volume_mix(x, y, weight):
    """The mixed volume of x and y at `weight` (volume_mix.frag), in x's dtype."""
    x, y = np.asarray(x), np.asarray(y)
    assert x.dtype == y.dtype and x.shape == y.shape
    w = F32(weight)
    oma = F32(1) - w
    with np.errstate(all="ignore"):
        if x.dtype in (np.uint8, np.uint16):
            mx = F32(RANGE[x.dtype])
            r = (x.astype(F32) / mx) * oma + (y.astype(F32) / mx) * w
            r = np.minimum(np.maximum(r, F32(0)), F32(1))
            return np.rint(r * mx).astype(x.dtype)
        r = x.astype(F32) * oma + y.astype(F32) * w
        return r if x.dtype == np.float32 else r.astype(np.float16)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same_or_both_nan(a, b):
    """Equal bit for bit, except that a NaN matches any NaN."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind != "f":
        return np.array_equal(a, b)
    nan = np.isnan(a)
    return np.array_equal(nan, np.isnan(b)) and np.array_equal(bits(a[~nan]), bits(b[~nan]))


def unorm16_ties(values, format_scaling=0.0, format_offset=0.0):
    """The values whose mapped clip(v, 0, 1) * 65535 in float32 is exactly k + 0.5 (where rint's ties-to-even decides)."""
    v = np.asarray(values)
    with np.errstate(all="ignore"):
        p = np.minimum(np.maximum(mapped(v, format_scaling, format_offset), F32(0)), F32(1)) * F32(65535)
    return v[np.isfinite(p) & (p - np.floor(p) == F32(0.5))]


def f32_tie_candidates(n, format_scaling=0.0, format_offset=0.0, seed=0):
    """float32 raw values near (k + 0.5) / 65535 under the mapping, for n random k; unorm16_ties picks the exact ties among them."""
    rng = np.random.default_rng(seed)
    k = rng.integers(0, 65535, n).astype(np.float64)
    oms = 1.0 - float(F32(format_scaling))
    if oms == 0.0:  # every finite voxel maps to +-0: no ties
        return np.zeros(0, F32)
    raw = ((k + 0.5) / 65535.0) / oms - float(F32(format_offset))
    base = raw.astype(F32)
    cand = [base]
    for _ in range(4):
        cand.append(np.nextafter(cand[-1], F32(np.inf)))
    down = [base]
    for _ in range(4):
        down.append(np.nextafter(down[-1], F32(-np.inf)))
    return np.unique(np.concatenate(cand + down[1:]))


# ---- value sets: the voxel values where the kernels could go wrong

F32_SPECIAL_BITS = np.array([
    0x7FC00000, 0xFFC00000,  # NaN of either sign (numpy's nan; what x86 gives for 0 / 0)
    0x7F800000, 0xFF800000,  # +-inf
    0x80000000,              # -0
    0x00000001, 0x007FFFFF, 0x80000001,  # subnormals
    0x7F7FFFFF, 0xFF7FFFFF,  # +-FLT_MAX
], np.uint32)
F16_SPECIAL_BITS = np.array([
    0x7E00, 0xFE00, 0x7C00, 0xFC00, 0x8000,
    0x0001, 0x03FF, 0x8001,  # the smallest and the largest subnormal, a negative one
    0x7BFF, 0xFBFF,          # +-65504
], np.uint16)
ORDINARY = np.array([-5.0, -0.3, 0.0, 0.5, 1.0, 1.7, 300.0], np.float32)


def specials(dtype):
    """The special values of a voxel type (integers: 0 and the maximum)."""
    dtype = np.dtype(dtype)
    if dtype == np.float32:
        return np.concatenate([F32_SPECIAL_BITS.view(np.float32), ORDINARY])
    if dtype == np.float16:
        return np.concatenate([F16_SPECIAL_BITS.view(np.float16), ORDINARY.astype(np.float16)])
    return np.array([0, np.iinfo(dtype).max], dtype)


def value_volume(dtype, shape, seed, extra=(), p=0.15, nan_block=8, special_slices=None):
    """A volume over the whole value domain of its type: random values (floats in [-0.5, 1.5)), a fraction p of the voxels of the
    first `special_slices` z slices (default: all) replaced by specials() and `extra`, and for floats a NaN-only block of nan_block^3
    voxels at the origin."""
    dtype = np.dtype(dtype)
    rng = np.random.default_rng(seed)
    if dtype.kind == "f":
        v = (rng.random(shape, dtype=np.float32) * F32(2) - F32(0.5)).astype(dtype)
    else:
        v = rng.integers(0, np.iinfo(dtype).max + 1, shape).astype(dtype)
    pool = np.concatenate([specials(dtype), np.asarray(extra, dtype)])
    at = rng.random(shape) < p
    if special_slices is not None:
        at[special_slices:] = False
    v[at] = pool[rng.integers(0, pool.size, int(at.sum()))]
    if dtype.kind == "f" and nan_block:
        v[:nan_block, :nan_block, :nan_block] = np.nan
    return v
