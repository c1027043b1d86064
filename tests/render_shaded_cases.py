"""The inputs of the shaded raycaster's comparison against its restatement, shared by the CPU test (which holds them to the exclusion cap and
measures the float32 deviation on them) and the GPU test (which renders them): the random volume / TF / light volume of
tests/test_render_gpu.py, every shading mode x voxel type x light layout x ray mode."""
import numpy as np

import render_reference as R
import render_shaded_reference as RS
from test_render_gpu import CAMERAS, H, W, light_volume, random_tf, random_volume   # the issue's inputs: that test's own generators

F32 = np.float32
DTYPES = [np.uint8, np.uint16, np.float16, np.float32]
CHANNELS = [1, 4]
RAYS = ["camera", "buffers"]
MODE_NAMES = ["ambient", "diffuse", "specular", "blinn_phong", "phong"]
LIGHT_DIMS = (11, 9, 7)
RATE = 1.0
# an affine texture -> world with unequal scales and a shear, so that A, its inverse transpose and the translation all matter
TEXTURE_TO_WORLD = np.array([[2.0, 0.25, 0.0, -1.0],
                             [0.0, 1.5, 0.125, -0.75],
                             [0.0, 0.0, 1.0, -0.5],
                             [0.0, 0.0, 0.0, 1.0]], np.float64)
MAX_AMBIGUOUS = 0.005   # of the live pixels

# What float32 costs the shading itself, measured without the kernel (test_render_shaded_cpu.test_float32_shading_deviation):
# the formulas evaluated in numpy float32 instead of float64 on these very samples need, with atol 1e-6, an rtol of at most
MEASURED_F32_RTOL = 7e-7
# The device's rsqrt and powf are a few ulps off numpy's, so the kernel gets four times that -- or the project's own rtol, if larger.
RTOL = max(1e-5, 4 * MEASURED_F32_RTOL)
ATOL = 1e-6


def shading(mode):
    return dict(mode=mode, texture_to_world=TEXTURE_TO_WORLD.T.reshape(16).astype(F32), light_position=(1.5, 2.5, 2.0),
                ambient=(0.2, 0.15, 0.1), diffuse=(0.6, 0.7, 0.5), specular=(0.4, 0.3, 0.5), shininess=12.0)


def camera_matrix(cpm, name, w=W, h=H):
    """world-space cameras looking at the transformed volume: tests/test_render_gpu.py's, moved by TEXTURE_TO_WORLD"""
    f, t, u, fov = CAMERAS[name]
    to_world = lambda p: (TEXTURE_TO_WORLD @ np.array([*p, 1.0]))[:3]   # noqa: E731
    return cpm.binding.camera_ndc_to_texture(to_world(f), to_world(t), u, fov, w / h, 0.1, 50.0, texture_to_world=TEXTURE_TO_WORLD)


def inputs(cpm, dtype, channels, rays):
    """-> (vol, lut, lv, ray keywords for the restatement: ndc_to_texture, or entry / exit as numpy)"""
    rng = np.random.default_rng(17 + channels + np.dtype(dtype).itemsize)
    vol = random_volume(rng, dtype)
    lut = random_tf(rng)
    lv = light_volume(rng, LIGHT_DIMS, channels)
    if rays == "camera":
        return vol, lut, lv, dict(ndc_to_texture=camera_matrix(cpm, "diagonal"))
    e, x = R.camera_buffers(camera_matrix(cpm, "inside"), W, H)
    return vol, lut, lv, dict(entry=e, exit=x)


def reference(vol, lut, lv, channels, rays_kw, mode, dtype=np.float64):
    return RS.render(vol, lut, lv, LIGHT_DIMS, channels, W, H, shading=shading(mode), dtype=dtype, sampling_rate=RATE, **rays_kw)
