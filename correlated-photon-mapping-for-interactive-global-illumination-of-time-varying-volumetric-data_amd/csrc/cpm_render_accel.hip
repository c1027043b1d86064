// cpm_render_accel.hip -- the raycaster's skip structure (cpm_render_accel_*, include/cpm/cpm_ext.h; DESIGN.md "Raycasting the light
// volume", empty-space skipping).  Two parts, each rebuilt by the edit that invalidates it:
//   * the range grid (a new time step): per brick the (lo, hi) of the normalised voxel value over the brick's voxels and their one-voxel
//     apron at +x, +y, +z -- every voxel a trilinear footprint based in the brick can read;
//   * the empty bits (a TF edit, or a new range grid): a brick is empty iff every TF texel that a value in [lo, hi] can touch, widened by
//     one texel on each side, has alpha 0 -- a prefix count of the non-zero alpha texels answers that in two loads per brick.
//
// MI355X mapping
//   * range grid: one 256-thread workgroup per (chunk of 256 x-columns, brick row y, brick slab z); a lane walks its column through the
//     (brick + 1)^2 rows of the slab, so every load of a wave is one contiguous run of the linear block (x fastest) and a voxel is read
//     (1 + 1 / brick)^2 times, from L2 after the first; the columns meet in LDS, where one lane per brick folds brick + 1 of them.
//   * empty bits: one lane per brick, one v_cmp + ballot per 64 bricks, one 8-byte store per wave.  No atomics anywhere.
#include "cpm_render_accel.h"
#include "cpm_trace_body.hip.h"

using namespace cpm;
using namespace cpm::tracer;

namespace {

constexpr int kColumns = 256;

template <int DT>
__global__ __launch_bounds__(256) void render_range_kernel(const void* voxels, int dx, int dy, int dz, int lg, int nbx, int nby, float norm,
                                                           float offset, float one_minus_scaling, float2* range) {
    typedef typename Voxel<DT>::T T;
    __shared__ float smin[kColumns + 1], smax[kColumns + 1];
    __shared__ int sbad[kColumns + 1];
    const int B = 1 << lg;
    const int x0 = blockIdx.x * kColumns;
    const int by = blockIdx.y, bz = blockIdx.z;
    const int y0 = by << lg, z0 = bz << lg;
    const int y1 = min(y0 + B, dy - 1), z1 = min(z0 + B, dz - 1);  // inclusive: the apron row / slice, clamped at the volume's edge
    const T* vox = static_cast<const T*>(voxels);
    // column kColumns is the apron of the chunk's last brick: inside the volume only when another chunk follows
    const int n_cols = x0 + kColumns < dx ? kColumns + 1 : kColumns;
    for (int c = threadIdx.x; c < n_cols; c += 256) {
        const int x = min(x0 + c, dx - 1);
        float lo = __builtin_inff(), hi = -__builtin_inff();
        int bad = 0;
        for (int z = z0; z <= z1; ++z)
            for (int y = y0; y <= y1; ++y) {
                const float v = Voxel<DT>::widen(vox[(size_t)x + (size_t)dx * ((size_t)y + (size_t)dy * (size_t)z)]);
                if (Voxel<DT>::is_float) bad |= !(__builtin_fabsf(v) < __builtin_inff());  // NaN or inf
                lo = min_(lo, v);  // (fminf / fmaxf drop a NaN; the brick is marked by `bad`)
                hi = max_(hi, v);
            }
        smin[c] = lo; smax[c] = hi; sbad[c] = bad;
    }
    __syncthreads();
    const int bx = (x0 >> lg) + (int)threadIdx.x;
    if ((int)threadIdx.x >= (kColumns >> lg) || bx >= nbx) return;
    const int c0 = (int)threadIdx.x << lg, c1 = min(c0 + B, n_cols - 1);
    float lo = smin[c0], hi = smax[c0];
    int bad = sbad[c0];
    for (int c = c0 + 1; c <= c1; ++c) { lo = min_(lo, smin[c]); hi = max_(hi, smax[c]); bad |= sbad[c]; }
    // the tail of tracer::sample_volume, operation by operation: weakly monotone in the interpolated raw value (every rounding is), so the
    // images of the extremes bound the images of everything between them, whichever way one_minus_scaling points
    const float a = (lo * norm + offset) * one_minus_scaling, b = (hi * norm + offset) * one_minus_scaling;
    const float nan = __builtin_nanf("");
    range[(size_t)bx + (size_t)nbx * ((size_t)by + (size_t)nby * (size_t)bz)] = bad ? make_float2(nan, nan) : make_float2(min_(a, b), max_(a, b));
}

// prefix[i] = texels j < i with alpha != 0 (a NaN alpha counts as non-zero); one workgroup
__global__ __launch_bounds__(256) void render_prefix_kernel(const float4* rgba, int width, uint32_t* prefix) {
    __shared__ uint32_t part[256];
    const int per = (width + 255) / 256;
    const int b = min((int)threadIdx.x * per, width), e = min(b + per, width);
    uint32_t c = 0;
    for (int i = b; i < e; ++i) c += !(rgba[i].w == 0.0f);
    part[threadIdx.x] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t run = 0;
        for (int j = 0; j < 256; ++j) { const uint32_t v = part[j]; part[j] = run; run += v; }
    }
    __syncthreads();
    uint32_t run = part[threadIdx.x];
    for (int i = b; i < e; ++i) { prefix[i] = run; run += !(rgba[i].w == 0.0f); }
    if (b < e && e == width) prefix[width] = run;
}

__global__ __launch_bounds__(256) void render_bits_kernel(const float2* range, uint32_t n_bricks, const uint32_t* prefix, int width, float wf,
                                                          float m1, float m2, uint32_t* bits) {
    const uint32_t b = blockIdx.x * 256u + threadIdx.x;
    bool empty = false;
    if (b < n_bricks) {
        const float2 r = range[b];
        if (r.x <= r.y && __builtin_fabsf(r.x) < __builtin_inff() && __builtin_fabsf(r.y) < __builtin_inff()) {  // (false for the NaN mark)
            // the sampler's own coord(): a value v reads texels i0(v) and i0(v) + 1, and i0 is weakly monotone in v
            float fl, a;
            coord(r.x, wf, m1, m2, fl, a);
            const int lo = max((int)fl - 1, 0);
            coord(r.y, wf, m1, m2, fl, a);
            const int hi = min((int)fl + 2, width - 1);
            empty = prefix[hi + 1] == prefix[lo];
        }
    }
    const unsigned long long m = __ballot(empty);
    if ((threadIdx.x & 63u) == 0u) {
        bits[2u * (b >> 6)] = (uint32_t)m;
        bits[2u * (b >> 6) + 1u] = (uint32_t)(m >> 32);
    }
}

}  // namespace

extern "C" {

int cpm_render_accel_create(cpm_ctx* ctx, const cpm_volume_desc* desc, int brick, cpm_render_accel** out) {
    CPM_ENTER(ctx);
    CPM_REQUIRE(ctx, desc && out, "cpm_render_accel_create: null argument");
    *out = nullptr;
    if (brick <= 0) brick = 8;
    CPM_REQUIRE(ctx, brick == 4 || brick == 8 || brick == 16, "cpm_render_accel_create: brick must be 4, 8 or 16");
    CPM_REQUIRE(ctx, desc->dims[0] > 0 && desc->dims[1] > 0 && desc->dims[2] > 0, "cpm_render_accel_create: dims must be positive");
    CPM_REQUIRE(ctx, cpm_dtype_valid(desc->dtype), "cpm_render_accel_create: unknown voxel type");
    CPM_REQUIRE(ctx, (unsigned long long)desc->dims[0] * desc->dims[1] * desc->dims[2] < (1ull << 32), "cpm_render_accel_create: volume too large");
    cpm_render_accel* a = new cpm_render_accel();
    for (int i = 0; i < 3; ++i) a->dims[i] = desc->dims[i];
    a->dtype = desc->dtype;
    a->brick = brick;
    a->lg = brick == 4 ? 2 : (brick == 8 ? 3 : 4);
    for (int i = 0; i < 3; ++i) a->nb[i] = (a->dims[i] + brick - 1) >> a->lg;
    a->n_bricks = (uint32_t)a->nb[0] * (uint32_t)a->nb[1] * (uint32_t)a->nb[2];
    a->n_words = (a->n_bricks + 31u) / 32u;
    const size_t padded_words = 8u * (size_t)div_up(a->n_bricks, 256);  // the bits kernel stores whole 64-lane ballots
    hipError_t e = hipMalloc((void**)&a->range, (size_t)a->n_bricks * sizeof(float2));
    if (e == hipSuccess) e = hipMalloc((void**)&a->bits, padded_words * sizeof(uint32_t));
    if (e != hipSuccess) {
        if (a->range) (void)hipFree(a->range);
        delete a;
        return set_error(ctx, CPM_ERR_DEVICE, "cpm_render_accel_create", hipGetErrorString(e));
    }
    *out = a;
    return CPM_OK;
}

void cpm_render_accel_destroy(cpm_ctx* ctx, cpm_render_accel* accel) {
    if (!ctx || !accel) return;
    if (accel->range) (void)hipFree(accel->range);
    if (accel->bits) (void)hipFree(accel->bits);
    if (accel->prefix) (void)hipFree(accel->prefix);
    delete accel;
}

int cpm_render_accel_update(cpm_ctx* ctx, cpm_render_accel* accel, const cpm_volume* vol, const cpm_tf* tf, cpm_stream stream) {
    CPM_ENTER(ctx);
    CPM_REQUIRE(ctx, accel, "cpm_render_accel_update: null accel");
    CPM_REQUIRE(ctx, vol || accel->have_range, "cpm_render_accel_update: the first update needs the volume");
    CPM_REQUIRE(ctx, tf || accel->tf, "cpm_render_accel_update: the first update needs the TF");
    if (vol) {
        const cpm_volume_desc& d = vol->desc;
        CPM_REQUIRE(ctx, d.dims[0] == accel->dims[0] && d.dims[1] == accel->dims[1] && d.dims[2] == accel->dims[2] && d.dtype == accel->dtype,
                    "cpm_render_accel_update: the volume's dims or type are not the accel's");
    }
    if (tf) CPM_REQUIRE(ctx, tf->width >= 2, "cpm_render_accel_update: tf width < 2");
    hipStream_t s = (hipStream_t)stream;
    if (tf && tf->width + 1 > accel->prefix_capacity) {
        uint32_t* p = nullptr;
        CPM_HIP_CHECK(ctx, hipMalloc((void**)&p, ((size_t)tf->width + 1) * sizeof(uint32_t)));
        if (accel->prefix) {
            CPM_HIP_CHECK(ctx, hipStreamSynchronize(s));  // a bits launch in flight may still read the old table
            (void)hipFree(accel->prefix);
        }
        accel->prefix = p;
        accel->prefix_capacity = tf->width + 1;
    }
    if (vol) {
        tracer::VolDev V{};
        make_vol_dev(vol, V);
        // the linear block: current after cpm_volume_update, cpm_volume_mix and a streamed acquire alike (the footprint copy may be stale
        // after a mix, and this launch neither needs nor rebuilds it)
        const dim3 g(div_up(accel->dims[0], kColumns), accel->nb[1], accel->nb[2]), b(256);
#define CPM_RANGE_LAUNCH(DT)                                                                                                              \
    CPM_LAUNCH(ctx, (render_range_kernel<DT>), g, b, 0, s, (const void*)vol->voxels, accel->dims[0], accel->dims[1], accel->dims[2], accel->lg, \
               accel->nb[0], accel->nb[1], V.norm, V.offset, V.one_minus_scaling, accel->range)
        CPM_DISPATCH_DTYPE(accel->dtype, CPM_RANGE_LAUNCH);  // (I16: w(v) is finite, never `bad`)
#undef CPM_RANGE_LAUNCH
        CPM_LAUNCH_CHECK(ctx, "render_range_kernel");
        accel->vol = vol;
        accel->have_range = true;
    }
    if (tf) {
        CPM_LAUNCH(ctx, render_prefix_kernel, dim3(1), dim3(256), 0, s, reinterpret_cast<const float4*>(tf->rgba), tf->width, accel->prefix);
        CPM_LAUNCH_CHECK(ctx, "render_prefix_kernel");
        accel->tf = tf;
        accel->tf_width = tf->width;
    }
    if (vol || tf) {
        const int w = accel->tf_width;
        CPM_LAUNCH(ctx, render_bits_kernel, dim3(div_up(accel->n_bricks, 256)), dim3(256), 0, s, (const float2*)accel->range, accel->n_bricks,
                   (const uint32_t*)accel->prefix, w, (float)w, (float)(w - 1), (float)(w - 2), accel->bits);
        CPM_LAUNCH_CHECK(ctx, "render_bits_kernel");
        accel->have_bits = true;
    }
    return CPM_OK;
}

int cpm_render_accel_info(cpm_ctx* ctx, const cpm_render_accel* accel, int32_t bricks[3], uint32_t* n_empty, cpm_stream stream) {
    CPM_ENTER(ctx);
    CPM_REQUIRE(ctx, accel, "cpm_render_accel_info: null accel");
    if (bricks) for (int i = 0; i < 3; ++i) bricks[i] = accel->nb[i];
    if (n_empty) {
        CPM_REQUIRE(ctx, accel->have_bits, "cpm_render_accel_info: the accel was never fully updated");
        std::vector<uint32_t> w(accel->n_words);
        hipStream_t s = (hipStream_t)stream;
        CPM_HIP_CHECK(ctx, hipMemcpyAsync(w.data(), accel->bits, w.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        CPM_HIP_CHECK(ctx, hipStreamSynchronize(s));
        uint32_t n = 0;
        for (uint32_t v : w) n += (uint32_t)__builtin_popcount(v);
        *n_empty = n;
    }
    return CPM_OK;
}

}  // extern "C"
