"""Every dtype dispatch of the library (CPM_DISPATCH_DTYPE and its three-way sibling, csrc/cpm_voxel.h) sends a volume to the kernel
instantiated for ITS type.  The profiling hook reports a launch under the kernel expression its CPM_LAUNCH was written with, and that
expression spells the enumerator, so the recorded names tell which instantiation ran -- also on data where the bits of two types
happen to agree (an I16 volume sent to the U16 kernels would pass a value test on non-negative voxels).

Per type, on a 16 x 6 x 5 volume (a row is 16, 32 or 64 bytes: the four types with a brick row kernel take it, I16 takes the per-brick
kernels): a plain trace, a trace over selected indices through a mixed volume (stale footprint copy: the LINEAR instantiation),
cpm_volume_mix, cpm_volume_minmax, cpm_volume_difference, cpm_volume_step, cpm_render, and cpm_render_accel_update + a skipping
render.  The fused re-trace (importance_retrace_kernel) is not called here: it needs a whole correlated mapper; its dispatch is the
same macro, and tests/test_f16_volume_gpu.py and tests/test_i16_volume_gpu.py hold its results to the F32 twin's bits."""
import re

import numpy as np
import pytest

from test_render_gpu import light_volume, matrix

pytestmark = pytest.mark.gpu
DIMS = (16, 6, 5)
TYPES = {"CPM_U8": np.uint8, "CPM_U16": np.uint16, "CPM_F32": np.float32, "CPM_F16": np.float16, "CPM_I16": np.int16}
REGION = 4


def _voxels(rng, dtype):
    shape = DIMS[::-1]
    if np.dtype(dtype).kind == "f":
        return rng.random(shape, dtype=np.float32).astype(dtype)
    info = np.iinfo(dtype)
    return rng.integers(info.min, info.max + 1, shape).astype(dtype)


def _launched(ctx, call):
    ctx.torch.cuda.synchronize()
    ctx.profile_reset()
    call()
    ctx.torch.cuda.synchronize()
    return sorted(ctx.profile_collect())


def _only(names, own, *wanted):
    """every dtype a recorded name spells is the volume's own, and each of `wanted` is part of some name"""
    for n in names:
        assert set(re.findall(r"CPM_(?:U8|U16|F32|F16|I16)\b", n)) <= {own}, (own, names)
    for w in wanted:
        assert any(w in n for n in names), (w, names)


@pytest.mark.parametrize("own", list(TYPES))
def test_each_dispatch_runs_the_volumes_own_instantiation(ctx, cpm, own):
    torch = ctx.torch
    B, P, S = cpm.binding, cpm.pipeline, cpm.synthetic
    dtype = TYPES[own]
    rng = np.random.default_rng(list(TYPES).index(own))
    a, b = _voxels(rng, dtype), _voxels(rng, dtype)
    va, vb, mixed = ctx.volume_create(a), ctx.volume_create(b), ctx.volume_create(np.zeros_like(a))
    assert int(va.desc.dtype) == getattr(B, own) == B._np_dtype_code(dtype)
    assert (DIMS[0] * B.DTYPE_SIZE[getattr(B, own)]) % 16 == 0
    row = own != "CPM_I16"                      # a brick row kernel exists for the type ...
    pair_row = row and own != "CPM_F32"         # ... and one that takes differences
    tf = ctx.tf_create(S.workspace_tf(256))
    fr = P.PhotonFrame(ctx, va, tf, 48, (8, 8, 8), light_travel_direction=(0.3, 0.5, -1.0))   # 2304 photons, single scattering
    nb = int(np.prod([(d + REGION - 1) // REGION for d in DIMS]))
    mm = torch.zeros((nb, 2), dtype=torch.int16, device=ctx.device)
    diff = torch.zeros(nb, dtype=torch.float32, device=ctx.device)
    idx = torch.arange(0, fr.n, 8, dtype=torch.int32, device=ctx.device)
    W = H = 32
    ldims = (8, 8, 8)
    lv = torch.from_numpy(light_volume(np.random.default_rng(3), ldims, 4)).to(ctx.device)
    g = B.default_grid_desc(ldims, 4)
    m = matrix(cpm, "diagonal", W, H)
    accel = ctx.render_accel(va, 4)

    ctx.profile_enable(True)
    try:
        _only(_launched(ctx, fr.trace), own, f"trace_kernel<{own}, EMIT_NONE, true>")
        _only(_launched(ctx, lambda: ctx.volume_mix(va, vb, 0.25, mixed)), own, f"volume_mix_kernel<{own}>")
        selected = _launched(ctx, lambda: ctx.trace(mixed, tf, fr.aabb, fr.params, fr.light_samples, fr.isect, fr.rng, fr.photons,
                                                    recompute_indices=idx, n_recompute=idx.numel()))
        _only(selected, own, f"trace_kernel<{own}, EMIT_NONE, true, true>")
        assert not any("quads_kernel" in n for n in selected), selected          # the footprint copy stayed stale: the linear block was read
        _only(_launched(ctx, lambda: ctx.volume_minmax(va, REGION, mm)), own, f"brick_row_kernel<{own}, 0>" if row else "minmax_kernel")
        _only(_launched(ctx, lambda: ctx.volume_difference(va, vb, REGION, diff)), own,
              f"brick_row_kernel<{own}, 1>" if pair_row else "difference_kernel")
        step = _launched(ctx, lambda: ctx.volume_step(va, vb, REGION, diff, mm))
        if pair_row:
            _only(step, own, f"brick_row_kernel<{own}, 2>")
        else:
            _only(step, own, "difference_kernel", f"brick_row_kernel<{own}, 0>" if row else "minmax_kernel")
        if not row:
            assert not any("brick_row_kernel" in n for n in step), step
        _only(_launched(ctx, lambda: ctx.render(va, tf, lv, g, W, H, ndc_to_texture=m)), own, f"render_kernel<{own}, 4>")
        _only(_launched(ctx, lambda: accel.update(va, tf)), own, f"render_range_kernel<{own}>")
        skipping = _launched(ctx, lambda: ctx.render(va, tf, lv, g, W, H, ndc_to_texture=m, accel=accel))
        _only(skipping, own, f"render_ex_kernel<{own}, 4, R_EX | R_SKIP>")
    finally:
        ctx.profile_enable(False)
        accel.close()
