// cpm_render_accel.h -- the raycaster's skip structure (cpm_render_accel, include/cpm/cpm_ext.h; DESIGN.md "Raycasting the light
// volume", empty-space skipping): built by cpm_render_accel.hip, read by cpm_render.hip.
#pragma once
#include "cpm_ctx.h"

struct cpm_render_accel {
    int dims[3] = { 0, 0, 0 };
    int dtype = 0;
    int brick = 8, lg = 3;            // brick edge in voxels (4, 8 or 16) and its log2
    int nb[3] = { 0, 0, 0 };          // bricks along x, y, z: ceil(dim / brick)
    uint32_t n_bricks = 0, n_words = 0;
    // range grid: per brick (lo, hi) of the normalised voxel value over the brick's voxels and their +x, +y, +z apron; (NaN, NaN) for a
    // brick that holds a voxel that is not finite (never empty)
    float2* range = nullptr;
    // empty bits: bit (b & 31) of word b >> 5, brick b = bx + nb.x (by + nb.y bz); 1 = every TF texel a sample based there can touch has
    // alpha 0.  n_words is a multiple of 2 (the bits kernel stores one 64-lane ballot at a time)
    uint32_t* bits = nullptr;
    // prefix[i] = texels j < i whose alpha is not zero (width + 1 entries)
    uint32_t* prefix = nullptr;
    int prefix_capacity = 0;
    // what the last update saw (cpm_render_ex refuses anything else)
    const cpm_volume* vol = nullptr;
    const cpm_tf* tf = nullptr;
    int tf_width = 0;
    bool have_range = false, have_bits = false;
};
