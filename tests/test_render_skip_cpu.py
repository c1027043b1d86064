"""The raycaster's empty-space rule (cpm_render_accel, include/cpm/cpm_ext.h; DESIGN.md "Raycasting the light volume"), without a GPU:
the entry points exist, and the rule -- restated here in numpy -- keeps its promise against the oracle's sampler: no sample whose
footprint is based in a brick marked empty has a non-zero alpha.

The restatement (also what tests/test_render_skip_gpu.py compares the device's empty-brick counts with):
  range grid   per brick, min / max of the normalised voxel value over the brick's voxels plus the one-voxel apron at +x, +y, +z,
               clamped at the volume's edge; a brick holding a NaN or an infinity is never empty;
  texel span   i0(min) - 1 .. i0(max) + 2 clamped to the TF, i0 = the sampler's texel floor (render_reference.coord): the two texels a
               value reads, over the range, widened by one texel on each side;
  bits         empty iff every alpha in the span is exactly zero."""
import re
from pathlib import Path

import numpy as np
import pytest

import render_reference as R

REPO = Path(__file__).resolve().parent.parent
F32 = np.float32
NEW_ENTRY_POINTS = ["cpm_render_accel_create", "cpm_render_accel_destroy", "cpm_render_accel_update", "cpm_render_accel_info", "cpm_render_ex"]


# ---------------------------------------------------------------------------------------------------------------- the rule, in numpy

def range_grid(vol, brick, format_scaling=0.0, format_offset=0.0):
    """(lo, hi) float32 arrays [nbz, nby, nbx]; NaN marks a brick that is never empty."""
    dz, dy, dx = vol.shape
    raw = vol.astype(F32)
    nb = [-(-d // brick) for d in (dz, dy, dx)]
    lo, hi = np.empty(nb, F32), np.empty(nb, F32)
    for bz in range(nb[0]):
        for by in range(nb[1]):
            for bx in range(nb[2]):
                sub = raw[bz * brick:min(bz * brick + brick + 1, dz), by * brick:min(by * brick + brick + 1, dy),
                          bx * brick:min(bx * brick + brick + 1, dx)]
                if not np.isfinite(sub).all():
                    lo[bz, by, bx] = hi[bz, by, bx] = np.nan
                else:
                    lo[bz, by, bx], hi[bz, by, bx] = sub.min(), sub.max()

    def g(c):   # the tail of the sampler: weakly monotone, so the images of the extremes bound everything between them
        return ((c * R.norm(vol.dtype) + F32(format_offset)) * (F32(1) - F32(format_scaling))).astype(F32)
    a, b = g(lo), g(hi)
    return np.minimum(a, b), np.maximum(a, b)


def empty_bricks(lo, hi, alpha):
    """bool [nbz, nby, nbx]: every texel a value in [lo, hi] can touch, widened by one on each side, has alpha exactly 0."""
    width = alpha.shape[0]
    nonzero = np.concatenate([[0], np.cumsum(~(alpha == 0))])   # prefix count; a NaN alpha counts as non-zero
    ok = np.isfinite(lo) & np.isfinite(hi)
    i_lo = np.maximum(R.coord(np.where(ok, lo, F32(0)), width)[0] - 1, 0)
    i_hi = np.minimum(R.coord(np.where(ok, hi, F32(0)), width)[0] + 2, width - 1)
    return ok & (nonzero[i_hi + 1] == nonzero[i_lo])


def base_brick(p, dims, brick):
    """(bz, by, bx) of the brick the footprint of a sample at p [n, 3] is based in: the sampler's floors, divided by the brick size."""
    dx, dy, dz = dims
    ix = R.coord(p[:, 0], dx, dx - 2)[0]
    iy = R.coord(p[:, 1], dy, max(dy - 2, 0))[0]
    iz = R.coord(p[:, 2], dz, max(dz - 2, 0))[0]
    return iz // brick, iy // brick, np.maximum(ix, 0) // brick


# ---------------------------------------------------------------------------------------------------------------------------- cases

def smooth_volume(dims, dtype, seed):
    """a few low-frequency waves: narrow value ranges per brick, so that a TF leaves bricks empty"""
    rng = np.random.default_rng(seed)
    dx, dy, dz = dims
    z, y, x = np.meshgrid((np.arange(dz) + 0.5) / dz, (np.arange(dy) + 0.5) / dy, (np.arange(dx) + 0.5) / dx, indexing="ij")
    f = rng.random(3) * 0.5 + 0.4
    v = 0.5 + 0.45 * np.sin(2 * np.pi * f[0] * x + 1) * (0.8 + 0.2 * np.cos(2 * np.pi * f[1] * y)) * (0.9 + 0.1 * np.sin(2 * np.pi * f[2] * z + 2))
    v = np.clip(v, 0, 1)
    if np.dtype(dtype) == np.float32:
        return v.astype(F32)
    return np.rint(v * np.iinfo(dtype).max).astype(dtype)


def skip_tfs(width=256, with_workspace=None):
    """name -> [width, 4] float32: the alpha shapes the rule has to survive (colours are irrelevant to it but not to the renderer)"""
    x = (np.arange(width) + 0.5) / width
    rgb = np.stack([0.6 + 0.4 * np.sin(7 * x), 0.5 + 0.5 * np.cos(5 * x), 0.3 + 0.2 * np.sin(11 * x + 1)], 1)

    def tf(a):
        return np.concatenate([rgb, np.asarray(a, np.float64)[:, None]], 1).astype(F32)

    def single(i):
        a = np.zeros(width)
        a[i] = 0.3
        return tf(a)
    out = {
        "threshold": tf(np.where(x < 0.6, 0.0, 0.05)),
        "band": tf(np.where((x > 0.35) & (x < 0.55), 0.0, 0.04)),
        "narrow": tf(np.where((x > 0.48) & (x < 0.52), 0.2, 0.0)),
        "all-zero": tf(np.zeros(width)),
        "all-non-zero": tf(np.full(width, 0.03)),
        "single-first": single(0),
        "single-last": single(width - 1),
        "single-interior": single(width // 2 + 3),
    }
    if with_workspace is not None:
        out["workspace"] = with_workspace
    return out


def positions(rng, dims, brick, n):
    """n texture-space points: half within 1e-3 voxels of a brick face along a random axis, a tenth outside [0,1]^3"""
    p = rng.random((n, 3))
    out = rng.random(n) < 0.1
    p[out] = p[out] * 1.6 - 0.3
    near = np.nonzero(rng.random(n) < 0.5)[0]
    axis = rng.integers(0, 3, near.size)
    d = np.asarray(dims, np.float64)[axis]
    face = rng.integers(0, np.ceil(d / brick).astype(np.int64) + 1) * brick
    delta = (rng.random(near.size) * 2 - 1) * 1e-3
    p[near, axis] = (face + 0.5 + delta) / d   # u = p * dim - 1/2 = face + delta
    return p.astype(F32)


CASES = [((37, 20, 9), 8), ((37, 20, 9), 4), ((16, 1, 23), 4), ((33, 18, 1), 8)]


# ---------------------------------------------------------------------------------------------------------------------------- tests

def test_header_declares_and_library_exports_the_entry_points(cpm):
    text = re.sub(r"/\*.*?\*/", "", (REPO / "include" / "cpm" / "cpm_ext.h").read_text(), flags=re.S)
    lib = cpm.binding.load_library()
    for name in NEW_ENTRY_POINTS:
        assert re.search(r"\b%s\s*\(" % name, text), f"{name} is not declared in cpm_ext.h"
        assert hasattr(lib, name), f"{name} is not exported by libcpm_hip.so"
        assert name in cpm.binding.EXT_SYMBOLS
    assert "cpm_render_options" in text and "clip_aabb" in text and "stats" in text
    assert lib.cpm_abi_version() == 2   # additive: the ABI version stays


def test_the_restatement_on_cases_worked_by_hand():
    vol = np.zeros((1, 1, 20), np.uint8)
    vol[0, 0, 8] = 255
    lo, hi = range_grid(vol, 8)
    # brick 0 covers voxels 0..7 and the apron voxel 8; brick 1 covers 8..15 and 16; brick 2 covers 16..19
    assert lo.shape == (1, 1, 3) and hi[0, 0].tolist() == [1.0, 1.0, 0.0] and lo[0, 0].tolist() == [0.0, 0.0, 0.0]
    a = np.zeros(16, F32)
    a[8] = 0.5   # values in [0, 0] touch texels 0, 1 (+ widening: 0..2): empty; [0, 1] touches all 16
    assert empty_bricks(lo, hi, a)[0, 0].tolist() == [False, False, True]
    a[:] = 0
    a[2] = 0.5   # texel 2 is in brick 2's widened span 0..2
    assert empty_bricks(lo, hi, a)[0, 0].tolist() == [False, False, False]
    a[:] = 0
    a[3] = 0.5
    assert empty_bricks(lo, hi, a)[0, 0].tolist() == [False, False, True]
    f = np.zeros((1, 1, 20), F32)
    f[0, 0, 16] = np.inf
    f[0, 0, 3] = np.nan
    lo, hi = range_grid(f, 8)
    assert empty_bricks(lo, hi, np.zeros(16, F32))[0, 0].tolist() == [False, False, False]   # never empty, even under an all-zero TF
    f[0, 0, 16] = 0
    lo, hi = range_grid(f, 8)
    assert empty_bricks(lo, hi, np.zeros(16, F32))[0, 0].tolist() == [False, True, True]


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.float32])
@pytest.mark.parametrize("dims,brick", CASES)
def test_no_sample_based_in_an_empty_brick_has_alpha(oracle, dims, brick, dtype):
    n = 100_000
    seed = 1000 * dims[0] + 10 * brick + np.dtype(dtype).itemsize
    rng = np.random.default_rng(seed)
    vol = smooth_volume(dims, dtype, seed)
    ov = oracle.volume(vol)
    p = positions(rng, dims, brick, n)
    assert (np.abs(p - 0.5) > 0.5).any(1).sum() > n // 20
    bz, by, bx = base_brick(p, dims, brick)
    lo, hi = range_grid(vol, brick)
    value = None
    some_empty = some_full = mixed = 0
    for name, lut in skip_tfs().items():
        empty = empty_bricks(lo, hi, lut[:, 3])
        if name == "all-zero":
            assert empty.all()
        if name == "all-non-zero":
            assert not empty.any()
        inside = np.nonzero(empty[bz, by, bx])[0]
        some_full += n - inside.size
        mixed += bool(empty.any() and not empty.all() and name in ("threshold", "band", "narrow"))
        if inside.size == 0:
            continue
        if value is None:   # the oracle's sampler, once per point
            value = np.array([oracle.lib.cpmo_sample_volume(ov, float(q[0]), float(q[1]), float(q[2])) for q in p], F32)
            # the samples stay in their brick's range up to the few ulps the widening is there for
            assert (value >= lo[bz, by, bx] - 1e-6).all() and (value <= hi[bz, by, bx] + 1e-6).all()
        lut = np.ascontiguousarray(lut, F32)   # (the oracle reads the alpha of an RGBA column)
        alpha = np.array([oracle.lib.cpmo_sample_tf_alpha(lut.ctypes.data, lut.shape[0], float(v)) for v in value[inside]], F32)
        bad = inside[alpha != 0]
        assert bad.size == 0, (name, p[bad[:3]], value[bad[:3]], alpha[alpha != 0][:3])
        some_empty += inside.size
    # the cases bite: many samples in empty bricks, many outside them, and a TF that splits the volume's bricks
    assert some_empty > n and some_full > n and mixed >= 1, (some_empty, some_full, mixed)
