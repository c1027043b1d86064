// cpm_render.hip -- emission-absorption raycaster of the photon-lit volume (cpm_render, include/cpm/cpm_ext.h; DESIGN.md
// "Raycasting the light volume").
//
// Stands where the workspace's org.inviwo.LightingRaycaster (a GLSL node fed by CL-GL sharing,
// workspaces/CorrelatedPhotonMappingSingleVolume.inv:821-970) stood: CDNA has no image hardware and the GPU hosts no GL context,
// so the volume, the TF and the light volume are composited into an RGBA float image here.
//
// MI355X mapping
//   * one lane per pixel; a 256-thread workgroup covers a 16 x 16 tile as four waves of 8 x 8 pixels, so the rays of a wave are
//     a compact bundle whose footprints share cache lines (a 64 x 1 row would spread over 64 columns of the volume).
//   * the volume sample is the tracer's own device function (tracer::sample_volume<DT>: one load of the 2 x 2 x 2 footprint
//     from cpm_volume::quads, 7 two-fma lerps) -- the same voxels and the same bits as a Woodcock step at the same point.
//   * the TF's RGBA column is staged once per workgroup into LDS (width x 16 B: 16 KiB for Inviwo's 1024 texels) and read with
//     two ds_read_b128 per sample; the tracer's coord() rule, applied to each channel, gives alpha the bits of sample_alpha.
//   * the light volume (8 loads of 4 B, or 8 of 16 B for 4 channels) is fetched only behind c.a > 0, so empty space costs the
//     volume and TF fetches alone.
//   * no atomics, no global writes but the one float4 pixel store: the image is deterministic by construction.
//
// cpm_render_ex adds, as instantiations of their own (render_ex_kernel; render_kernel compiles as it did without them):
//   * R_SKIP: empty-space skipping over a cpm_render_accel.  A sample whose footprint is based in a brick whose bit is set has alpha 0
//     (cpm_render_accel.hip), and a sample with alpha 0 changes no state, so the loop may jump k over a run of such samples.  The brick
//     comes from the sampler's own coord() floors; how far to jump is a guess from the ray's exit out of the brick, and the guess is
//     VERIFIED: a sample's floors are weakly monotone in k along every axis (k -> t -> p -> floor are all monotone roundings), so if
//     sample k and sample k + j are based in the same brick, so is every sample between them.  A wrong guess costs a short jump, never
//     a wrong pixel.  The bits sit in LDS behind the TF column when they are small (4 KiB for 32^3 bricks), else they are read through
//     L2; one word per sample.
//   * R_STATS: samples evaluated / skipped, summed over the wave and added with one atomic per counter and wave.
//   * the clip box: the slab test against (lo, hi) from the arguments instead of (0, 1).
//
// cpm_render_shaded adds R_SHADE (render_shaded_kernel: the same render_ex_body, one more argument block): gradient shading of the TF
// colour behind c.a > 0, before the multiplication by the light volume.
//   * the gradient is six more calls of the same sample_volume<DT> at p +- (1 / dim) e_a -- the contract is their bits, so nothing is
//     shared between them.  They are independent of each other and of the light volume's eight loads, and all fourteen fetches are in
//     flight together before the first is consumed (one lane has no other work to hide them behind: DESIGN.md).  CPM_SHADE_AMBIENT needs
//     no gradient and fetches none.
//   * the matrices, the light and the material ride in the kernel arguments: SGPRs, no loads in the loop.
//   * the view vector is the ray's, so it is computed once per pixel; N, L, H, R once per shaded sample in float32 (v_rsq_f32, powf).
#include "cpm_render_accel.h"
#include "cpm_trace_body.hip.h"

using namespace cpm;
using namespace cpm::tracer;

namespace {

constexpr float kRefSamplingInterval = 150.0f;  // Inviwo's REF_SAMPLING_INTERVAL (opacity correction)
constexpr float kErtThreshold = 0.99f;          // early ray termination: stop once res.a exceeds it
constexpr float kMaxSamples = 16777216.0f;      // a ray that would take more samples (entry / exit far outside the box) is a miss

struct RenderArgs {
    VolDev vol;
    const float4* tf;                 // cpm_tf::rgba
    int tf_width;
    float tf_wf, tf_m1, tf_m2;
    const float* light;               // cells x channels, channels fastest
    int ldx, ldy, ldz;
    float lfx, lfy, lfz, lm1x, lm1y, lm1z, lm2x, lm2y, lm2z;
    uint32_t lsy, lsz;                // row / slice stride in cells
    int colored;
    int width, height;
    float wf, hf;
    float m[16];                      // ndc -> texture, column-major
    float rate;
    const float4* entry;              // nullable: buffer mode
    const float4* exit;
    float4* out;
};

// The light volume at p: texel centres at (i + 1/2) / dim, clamp to edge, trilinear in the tracer's lerp order (x, then y, then z).
template <int CH>
CPM_DEV void sample_light(const RenderArgs& A, float px, float py, float pz, float& lr, float& lg, float& lb) {
    float flx, fly, flz, ax, ay, az;
    coord(px, A.lfx, A.lm1x, A.lm2x, flx, ax);
    coord(py, A.lfy, A.lm1y, A.lm2y, fly, ay);
    coord(pz, A.lfz, A.lm1z, A.lm2z, flz, az);
    const uint32_t ix = (uint32_t)flx, iy = (uint32_t)fly, iz = (uint32_t)flz;
    // the upper neighbour, clamped (a dimension of 1 has none: its weight is 0 and the texel is read twice)
    const uint32_t dx1 = (float)ix < A.lm1x ? 1u : 0u;
    const uint32_t dy1 = (float)iy < A.lm1y ? A.lsy : 0u;
    const uint32_t dz1 = (float)iz < A.lm1z ? A.lsz : 0u;
    const uint32_t b = ix + A.lsy * iy + A.lsz * iz;
    const uint32_t off[4] = { 0u, dy1, dz1, dy1 + dz1 };  // (y, z), (y', z), (y, z'), (y', z')
    float c[4][3];
    if (CH == 1) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float v0 = A.light[b + off[k]], v1 = A.light[b + off[k] + dx1];
            c[k][0] = lerp_(v0, v1, ax);
        }
        const float r = lerp_(lerp_(c[0][0], c[1][0], ay), lerp_(c[2][0], c[3][0], ay), az);
        lr = lg = lb = r;
    } else {
        const float4* L4 = reinterpret_cast<const float4*>(A.light);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float4 v0 = L4[b + off[k]], v1 = L4[b + off[k] + dx1];
            c[k][0] = lerp_(v0.x, v1.x, ax);
            c[k][1] = lerp_(v0.y, v1.y, ax);
            c[k][2] = lerp_(v0.z, v1.z, ax);
        }
        float o[3];
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) o[ch] = lerp_(lerp_(c[0][ch], c[1][ch], ay), lerp_(c[2][ch], c[3][ch], ay), az);
        lr = o[0];
        lg = A.colored ? o[1] : o[0];
        lb = A.colored ? o[2] : o[0];
    }
}

// p = M (x, y, z, 1), divided by its w; sums in column order, no fma (the numpy restatement's order)
CPM_DEV void unproject(const float* m, float x, float y, float z, float& px, float& py, float& pz) {
    const float w = m[3] * x + m[7] * y + m[11] * z + m[15];
    px = (m[0] * x + m[4] * y + m[8] * z + m[12]) / w;
    py = (m[1] * x + m[5] * y + m[9] * z + m[13]) / w;
    pz = (m[2] * x + m[6] * y + m[10] * z + m[14]) / w;
}

CPM_DEV void slab(float o, float d, float lo, float hi, float& s0, float& s1) {
    const float inv = 1.0f / d;
    // d = 0: +-inf outside the slab, [-inf, inf] inside it; o on a face gives 0 * inf = NaN for that face, which fminf / fmaxf drop,
    // so the other face's infinity empties the range -- a ray in the plane of a face is a miss
    const float ta = (lo - o) * inv, tb = (hi - o) * inv;
    s0 = max_(s0, min_(ta, tb));
    s1 = min_(s1, max_(ta, tb));
}

enum { R_SKIP = 1, R_STATS = 2, R_EX = 4, R_SHADE = 8 };

// what cpm_render_ex adds to a launch
struct RenderExArgs {
    float clip_lo[3], clip_hi[3];
    const uint32_t* bits;             // cpm_render_accel::bits (1 = empty); R_SKIP only
    uint32_t bits_words;              // words staged into LDS behind the TF column; 0: read them from `bits`
    int lg, nbx, nbxy;                // log2(brick), bricks along x, bricks per z slab
    float last_bx, last_by, last_bz;  // the last brick a footprint can be based in along each axis: max(dim - 2, 0) >> lg
    uint32_t* stats;                  // R_STATS only
};

CPM_DEV void sample_position(const float ex, const float ey, const float ez, const float dirx, const float diry, const float dirz,
                             const float tIncr, const int k, float& px, float& py, float& pz) {
    const float t = ((float)k + 0.5f) * tIncr;
    px = ex + t * dirx; py = ey + t * diry; pz = ez + t * dirz;
}

// the brick a sample at p is based in: the floors of sample_volume's own coord() calls, shifted
CPM_DEV int sample_brick(const VolDev& V, const RenderExArgs& X, float px, float py, float pz, int& ix, int& iy, int& iz) {
    float flx, fly, flz, a;
    coord(px, V.fx, V.mx1, V.mx2, flx, a);
    coord(py, V.fy, V.my1, V.my2, fly, a);
    coord(pz, V.fz, V.mz1, V.mz2, flz, a);
    ix = (int)flx; iy = (int)fly; iz = (int)flz;
    return (ix >> X.lg) + X.nbx * (iy >> X.lg) + X.nbxy * (iz >> X.lg);
}

// along one axis: the (real-valued) sample index at which u = p * dim - 1/2 leaves the brick [b << lg, (b + 1) << lg); the first and the
// last brick reach to infinity (coord() clamps).  A guess: rounded any way, v_rcp_f32.
CPM_DEV float brick_exit(float e, float step, float dimf, int i, int lg, float last) {
    const int b = i >> lg;
    const float su = step * dimf;                       // voxels per sample
    const float u0 = fma_(e, dimf, fma_(0.5f, su, -0.5f));  // u of sample 0
    const float inf = __builtin_inff();
    const float bound = su > 0.0f ? ((float)b < last ? (float)((b + 1) << lg) : inf) : (b > 0 ? (float)(b << lg) : -inf);
    return su == 0.0f ? inf : (bound - u0) * __builtin_amdgcn_rcpf(su);
}

// what cpm_render_shaded adds to a launch (R_SHADE only)
struct RenderShadeArgs {
    int mode;                         // CPM_SHADE_AMBIENT .. CPM_SHADE_PHONG
    float h[3];                       // 1 / dim: the central difference's offset along each axis
    float s[3];                       // dim / 2: what the difference is multiplied by
    float a[9];                       // texture -> world, linear part A, column-major (a[3 c + r])
    float t[3];                       // ... and translation
    float nit[9];                     // inverse transpose of A, column-major: normals
    float light[3];                   // world space
    float ka[3], kd[3], ks[3];
    float shininess;
};

// m v, m column-major 3 x 3; sums in column order
CPM_DEV void mul3(const float* m, float x, float y, float z, float& ox, float& oy, float& oz) {
    ox = m[0] * x + m[3] * y + m[6] * z;
    oy = m[1] * x + m[4] * y + m[7] * z;
    oz = m[2] * x + m[5] * y + m[8] * z;
}

// v / |v|; the zero vector stays zero (a light at the sample's own position, L = -V)
CPM_DEV void normalize0(float& x, float& y, float& z) {
    const float l2 = x * x + y * y + z * z;
    const float inv = l2 > 0.0f ? __builtin_amdgcn_rsqf(l2) : 0.0f;
    x *= inv; y *= inv; z *= inv;
}

// central differences of the sampler itself: g_a = (S(p + h_a e_a) - S(p - h_a e_a)) * (dim_a / 2), six sample_volume values bit for bit.
// One-sided at half magnitude where the sampler clamps (the volume's edge).
template <int DT>
CPM_DEV void sample_gradient(const VolDev& V, const RenderShadeArgs& S, float px, float py, float pz, float& gx, float& gy, float& gz) {
    const float xp = sample_volume<DT>(V, px + S.h[0], py, pz), xm = sample_volume<DT>(V, px - S.h[0], py, pz);
    const float yp = sample_volume<DT>(V, px, py + S.h[1], pz), ym = sample_volume<DT>(V, px, py - S.h[1], pz);
    const float zp = sample_volume<DT>(V, px, py, pz + S.h[2]), zm = sample_volume<DT>(V, px, py, pz - S.h[2]);
    gx = (xp - xm) * S.s[0];
    gy = (yp - ym) * S.s[1];
    gz = (zp - zm) * S.s[2];
}

// c = ka c + kd c |N.L| + ks spec, spec = |N.H|^s (Blinn) or max(R.V, 0)^s (Phong); (vx, vy, vz) = V, unit, world space.
// A gradient of exactly +-0 in all three components leaves the ambient term alone: decided on g, before any matrix.
CPM_DEV void shade(const RenderShadeArgs& S, float gx, float gy, float gz, float px, float py, float pz, float vx, float vy, float vz,
                   float& cr, float& cg, float& cb) {
    float dif = 0.0f, spec = 0.0f;
    if (S.mode != CPM_SHADE_AMBIENT && !(gx == 0.0f && gy == 0.0f && gz == 0.0f)) {
        // the gradient's scale is the data's: bring its largest component to [1/2, 1) first, so that the squares neither underflow nor overflow
        const int e = __builtin_amdgcn_frexp_expf(max_(max_(__builtin_fabsf(gx), __builtin_fabsf(gy)), __builtin_fabsf(gz)));
        float nx, ny, nz;
        mul3(S.nit, __builtin_ldexpf(gx, -e), __builtin_ldexpf(gy, -e), __builtin_ldexpf(gz, -e), nx, ny, nz);
        normalize0(nx, ny, nz);
        float wx, wy, wz;
        mul3(S.a, px, py, pz, wx, wy, wz);
        float lx = S.light[0] - (wx + S.t[0]), ly = S.light[1] - (wy + S.t[1]), lz = S.light[2] - (wz + S.t[2]);
        normalize0(lx, ly, lz);
        const float nl = nx * lx + ny * ly + nz * lz;
        if (S.mode != CPM_SHADE_SPECULAR) dif = __builtin_fabsf(nl);
        if (S.mode == CPM_SHADE_BLINN_PHONG) {
            float hx = lx + vx, hy = ly + vy, hz = lz + vz;
            normalize0(hx, hy, hz);
            spec = powf(__builtin_fabsf(nx * hx + ny * hy + nz * hz), S.shininess);
        } else if (S.mode == CPM_SHADE_SPECULAR || S.mode == CPM_SHADE_PHONG) {
            const float k = 2.0f * nl;
            const float rv = (k * nx - lx) * vx + (k * ny - ly) * vy + (k * nz - lz) * vz;
            spec = powf(max_(rv, 0.0f), S.shininess);
        }
    }
    cr = S.ka[0] * cr + S.kd[0] * cr * dif + S.ks[0] * spec;
    cg = S.ka[1] * cg + S.kd[1] * cg * dif + S.ks[1] * spec;
    cb = S.ka[2] * cb + S.kd[2] * cb * dif + S.ks[2] * spec;
}

template <int DT, int CH, int MODE>
CPM_DEV float4 render_pixel(const RenderArgs& A, const RenderExArgs& X, const RenderShadeArgs& S, const float4* lut, const uint32_t* lbits, const int pi, const int pj,
                            const int pix, uint32_t& evaluated, uint32_t& skipped) {
    float ex, ey, ez, rx, ry, rz;
    bool hit;
    if (A.entry) {
        const float4 e = A.entry[pix], x = A.exit[pix];
        hit = e.w != 0.0f;
        ex = e.x; ey = e.y; ez = e.z;
        rx = x.x - e.x; ry = x.y - e.y; rz = x.z - e.z;
    } else {
        const float nx = 2.0f * ((float)pi + 0.5f) / A.wf - 1.0f;
        const float ny = 2.0f * ((float)pj + 0.5f) / A.hf - 1.0f;
        float ox, oy, oz, fx, fy, fz;
        unproject(A.m, nx, ny, -1.0f, ox, oy, oz);
        unproject(A.m, nx, ny, 1.0f, fx, fy, fz);
        const float dx = fx - ox, dy = fy - oy, dz = fz - oz;
        float s0 = 0.0f, s1 = 1.0f;
        if (MODE & R_EX) {
            slab(ox, dx, X.clip_lo[0], X.clip_hi[0], s0, s1);
            slab(oy, dy, X.clip_lo[1], X.clip_hi[1], s0, s1);
            slab(oz, dz, X.clip_lo[2], X.clip_hi[2], s0, s1);
        } else {
            slab(ox, dx, 0.0f, 1.0f, s0, s1);
            slab(oy, dy, 0.0f, 1.0f, s0, s1);
            slab(oz, dz, 0.0f, 1.0f, s0, s1);
        }
        hit = s0 < s1;
        ex = ox + s0 * dx; ey = oy + s0 * dy; ez = oz + s0 * dz;
        rx = (ox + s1 * dx) - ex; ry = (oy + s1 * dy) - ey; rz = (oz + s1 * dz) - ez;
    }
    const float tEnd = __builtin_sqrtf(rx * rx + ry * ry + rz * rz);
    const float qx = rx * A.vol.fx, qy = ry * A.vol.fy, qz = rz * A.vol.fz;
    const float nf = max_(__builtin_ceilf(A.rate * __builtin_sqrtf(qx * qx + qy * qy + qz * qz)), 1.0f);
    float4 res = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (hit && tEnd > 0.0f && nf <= kMaxSamples) {
        const int n = (int)nf;
        const float tIncr = tEnd / nf;
        const float dirx = rx / tEnd, diry = ry / tEnd, dirz = rz / tEnd;
        const float expo = tIncr * kRefSamplingInterval;
        float vx = 0.0f, vy = 0.0f, vz = 0.0f;  // V = -normalize(A dir): the ray's, in either ray mode
        if (MODE & R_SHADE) {
            mul3(S.a, dirx, diry, dirz, vx, vy, vz);
            normalize0(vx, vy, vz);
            vx = -vx; vy = -vy; vz = -vz;
        }
        for (int k = 0; k < n; ++k) {
            float px, py, pz;
            sample_position(ex, ey, ez, dirx, diry, dirz, tIncr, k, px, py, pz);
            if (MODE & R_SKIP) {
                int ix, iy, iz;
                const int b = sample_brick(A.vol, X, px, py, pz, ix, iy, iz);
                const uint32_t word = X.bits_words ? lbits[b >> 5] : X.bits[b >> 5];
                if ((word >> (b & 31)) & 1u) {
                    // every sample up to `last` is skipped: the guess, then the proof (the header comment) -- or this sample alone
                    const float kx = brick_exit(ex, tIncr * dirx, A.vol.fx, ix, X.lg, X.last_bx);
                    const float ky = brick_exit(ey, tIncr * diry, A.vol.fy, iy, X.lg, X.last_by);
                    const float kz = brick_exit(ez, tIncr * dirz, A.vol.fz, iz, X.lg, X.last_bz);
                    const float kf = __builtin_floorf(min_(min_(kx, ky), kz) - 0.0625f);
                    int last = (int)max_(min_(kf, (float)(n - 1)), (float)k);  // (fminf / fmaxf drop a NaN guess)
                    if (last > k) {
                        float qx, qy, qz;
                        int jx, jy, jz;
                        sample_position(ex, ey, ez, dirx, diry, dirz, tIncr, last, qx, qy, qz);
                        if (sample_brick(A.vol, X, qx, qy, qz, jx, jy, jz) != b) last = k;
                    }
                    if (MODE & R_STATS) skipped += (uint32_t)(last - k + 1);
                    k = last;
                    continue;
                }
            }
            if (MODE & R_STATS) ++evaluated;
            const float v = sample_volume<DT>(A.vol, px, py, pz);
            float fl, a;
            coord(v, A.tf_wf, A.tf_m1, A.tf_m2, fl, a);
            const int i = (int)fl;
            const float4 lo = lut[i], hi = lut[i + 1];
            const float ca = lerp_(lo.w, hi.w, a);
            if (ca > 0.0f) {
                float lr, lg, lb;
                sample_light<CH>(A, px, py, pz, lr, lg, lb);
                float cr = lerp_(lo.x, hi.x, a), cg = lerp_(lo.y, hi.y, a), cb = lerp_(lo.z, hi.z, a);
                if (MODE & R_SHADE) {
                    // the six fetches of the gradient and the light volume's eight above depend on p alone: all in flight together
                    float gx = 0.0f, gy = 0.0f, gz = 0.0f;
                    if (S.mode != CPM_SHADE_AMBIENT) sample_gradient<DT>(A.vol, S, px, py, pz, gx, gy, gz);
                    shade(S, gx, gy, gz, px, py, pz, vx, vy, vz, cr, cg, cb);
                }
                cr = cr * lr; cg = cg * lg; cb = cb * lb;
                // 1 - (1 - ca)^expo without the cancellation of 1 - pow(): the small opacities of fine sampling keep their digits
                const float ap = -expm1f(expo * log1pf(-ca));
                const float wgt = (1.0f - res.w) * ap;
                res.x = res.x + wgt * cr;
                res.y = res.y + wgt * cg;
                res.z = res.z + wgt * cb;
                res.w = res.w + wgt;
                if (res.w > kErtThreshold) break;
            }
        }
    }
    return res;
}

template <int DT, int CH>
__global__ __launch_bounds__(256) void render_kernel(const RenderArgs A) {
    extern __shared__ float4 lut[];
    for (int i = threadIdx.x; i < A.tf_width; i += 256) lut[i] = A.tf[i];
    __syncthreads();

    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int pi = blockIdx.x * 16 + (w & 1) * 8 + (lane & 7);
    const int pj = blockIdx.y * 16 + (w >> 1) * 8 + (lane >> 3);
    if (pi >= A.width || pj >= A.height) return;
    const int pix = pj * A.width + pi;
    uint32_t evaluated = 0, skipped = 0;
    const RenderExArgs X{};
    const RenderShadeArgs S{};
    A.out[pix] = render_pixel<DT, CH, 0>(A, X, S, lut, nullptr, pi, pj, pix, evaluated, skipped);
}

template <int DT, int CH, int MODE>
CPM_DEV void render_ex_body(const RenderArgs& A, const RenderExArgs& X, const RenderShadeArgs& S) {
    extern __shared__ float4 lut[];
    uint32_t* lbits = reinterpret_cast<uint32_t*>(lut + A.tf_width);
    for (int i = threadIdx.x; i < A.tf_width; i += 256) lut[i] = A.tf[i];
    if (MODE & R_SKIP)
        for (uint32_t i = threadIdx.x; i < X.bits_words; i += 256) lbits[i] = X.bits[i];
    __syncthreads();

    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int pi = blockIdx.x * 16 + (w & 1) * 8 + (lane & 7);
    const int pj = blockIdx.y * 16 + (w >> 1) * 8 + (lane >> 3);
    uint32_t evaluated = 0, skipped = 0;
    if (pi < A.width && pj < A.height) {
        const int pix = pj * A.width + pi;
        A.out[pix] = render_pixel<DT, CH, MODE>(A, X, S, lut, lbits, pi, pj, pix, evaluated, skipped);
    }
    if (MODE & R_STATS) {  // all 64 lanes are here again: the wave's sums, one atomic each
#pragma unroll
        for (int m = 32; m > 0; m >>= 1) {
            evaluated += (uint32_t)__shfl_xor((int)evaluated, m);
            skipped += (uint32_t)__shfl_xor((int)skipped, m);
        }
        if (lane == 0) {
            atomicAdd(&X.stats[0], evaluated);
            if (MODE & R_SKIP) atomicAdd(&X.stats[1], skipped);
        }
    }
}

template <int DT, int CH, int MODE>
__global__ __launch_bounds__(256) void render_ex_kernel(const RenderArgs A, const RenderExArgs X) {
    const RenderShadeArgs S{};
    render_ex_body<DT, CH, MODE>(A, X, S);
}

// MODE includes R_SHADE
template <int DT, int CH, int MODE>
__global__ __launch_bounds__(256) void render_shaded_kernel(const RenderArgs A, const RenderExArgs X, const RenderShadeArgs S) {
    render_ex_body<DT, CH, MODE>(A, X, S);
}

}  // namespace

// validation and kernel arguments shared by cpm_render and cpm_render_ex; lds = the TF column's bytes
static int render_prepare(cpm_ctx* ctx, const char* who, const cpm_volume* vol, const cpm_tf* tf, const float* light_volume, const cpm_grid_desc* grid,
                          const cpm_render_desc* desc, float* rgba_out, RenderArgs& A, size_t& lds) {
    CPM_REQUIRE(ctx, vol && tf && light_volume && grid && desc && rgba_out, "cpm_render: null argument");
    const cpm_render_desc& D = *desc;
    CPM_REQUIRE(ctx, grid->channels == 1 || grid->channels == 4, "cpm_render: light volume channels must be 1 or 4");
    CPM_REQUIRE(ctx, grid->dims[0] > 0 && grid->dims[1] > 0 && grid->dims[2] > 0, "cpm_render: light volume dims must be positive");
    CPM_REQUIRE(ctx, (unsigned long long)grid->dims[0] * grid->dims[1] * grid->dims[2] * grid->channels < (1ull << 32),
                "cpm_render: light volume too large");
    CPM_REQUIRE(ctx, D.width > 0 && D.height > 0 && (long long)D.width * D.height < (1ll << 31), "cpm_render: 0 < width, height and width * height < 2^31");
    CPM_REQUIRE(ctx, D.sampling_rate > 0.0f && D.sampling_rate <= 3.402823466e+38f, "cpm_render: sampling_rate must be finite and > 0");
    CPM_REQUIRE(ctx, tf->width >= 2, "cpm_render: tf width < 2");
    CPM_REQUIRE(ctx, (D.entry == nullptr) == (D.exit == nullptr), "cpm_render: entry and exit are given together or not at all");
    CPM_REQUIRE_ALIGNED16(ctx, rgba_out, "cpm_render");
    if (grid->channels == 4) CPM_REQUIRE_ALIGNED16(ctx, light_volume, "cpm_render");
    if (D.entry) { CPM_REQUIRE_ALIGNED16(ctx, D.entry, "cpm_render"); CPM_REQUIRE_ALIGNED16(ctx, D.exit, "cpm_render"); }
    const cpm_volume_desc& vd = vol->desc;
    CPM_REQUIRE(ctx, (unsigned long long)vd.dims[0] * vd.dims[1] * vd.dims[2] < (1ull << 32), "cpm_render: volume too large");
    lds = (size_t)tf->width * sizeof(float4);
    if (lds > ctx->lds_per_block) return set_error(ctx, CPM_ERR_UNSUPPORTED, who, "the TF's RGBA column does not fit the workgroup's LDS");

    A.tf = reinterpret_cast<const float4*>(tf->rgba);
    A.tf_width = tf->width;
    A.tf_wf = (float)tf->width; A.tf_m1 = (float)(tf->width - 1); A.tf_m2 = (float)(tf->width - 2);
    A.light = light_volume;
    A.ldx = grid->dims[0]; A.ldy = grid->dims[1]; A.ldz = grid->dims[2];
    A.lfx = (float)A.ldx; A.lfy = (float)A.ldy; A.lfz = (float)A.ldz;
    A.lm1x = (float)(A.ldx - 1); A.lm1y = (float)(A.ldy - 1); A.lm1z = (float)(A.ldz - 1);
    A.lm2x = (float)(A.ldx > 2 ? A.ldx - 2 : 0); A.lm2y = (float)(A.ldy > 2 ? A.ldy - 2 : 0); A.lm2z = (float)(A.ldz > 2 ? A.ldz - 2 : 0);
    A.lsy = (uint32_t)A.ldx;
    A.lsz = (uint32_t)A.ldx * (uint32_t)A.ldy;
    A.colored = D.colored_light != 0;
    A.width = D.width; A.height = D.height;
    A.wf = (float)D.width; A.hf = (float)D.height;
    memcpy(A.m, D.ndc_to_texture, sizeof(A.m));
    A.rate = D.sampling_rate;
    A.entry = reinterpret_cast<const float4*>(D.entry);
    A.exit = reinterpret_cast<const float4*>(D.exit);
    A.out = reinterpret_cast<float4*>(rgba_out);
    return CPM_OK;
}

// the tracer's view of the volume; a stale footprint copy (cpm_volume_mix) is rebuilt first
static int render_volume(cpm_ctx* ctx, const cpm_volume* vol, hipStream_t s, RenderArgs& A) {
    tracer::TraceArgs T{};
    make_vol_dev(vol, T.vol);
    bool linear = false;
    const int rc = trace_volume_source(ctx, vol, false, s, T, &linear);
    if (rc) return rc;
    A.vol = T.vol;
    return CPM_OK;
}

extern "C" {

int cpm_render(cpm_ctx* ctx, const cpm_volume* vol, const cpm_tf* tf, const float* light_volume, const cpm_grid_desc* grid,
               const cpm_render_desc* desc, float* rgba_out, cpm_stream stream) {
    CPM_ENTER(ctx);
    RenderArgs A{};
    size_t lds = 0;
    int rc = render_prepare(ctx, "cpm_render", vol, tf, light_volume, grid, desc, rgba_out, A, lds);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    rc = render_volume(ctx, vol, s, A);
    if (rc) return rc;

    const dim3 g(div_up(A.width, 16), div_up(A.height, 16)), b(256);
#define CPM_RENDER_LAUNCH(DT)                                                                               \
    do {                                                                                                    \
        if (grid->channels == 1) CPM_LAUNCH(ctx, (render_kernel<DT, 1>), g, b, lds, s, A);                  \
        else CPM_LAUNCH(ctx, (render_kernel<DT, 4>), g, b, lds, s, A);                                      \
    } while (0)
    CPM_DISPATCH_DTYPE(vol->desc.dtype, CPM_RENDER_LAUNCH);
#undef CPM_RENDER_LAUNCH
    CPM_LAUNCH_CHECK(ctx, "render_kernel");
    return CPM_OK;
}

void cpm_debug_set_render_bits_lds(cpm_ctx* ctx, int max_bytes) { if (ctx) ctx->dbg.render_bits_lds = max_bytes; }

}  // extern "C"

// texture_to_world (column-major, affine) -> the kernel's A, t and inverse transpose of A (in double, rounded once); false: not finite, a
// last row other than (0, 0, 0, 1), or a singular A
static bool shade_matrices(const float* m, RenderShadeArgs& S) {
    for (int i = 0; i < 16; ++i) if (!(m[i] - m[i] == 0.0f)) return false;
    if (m[3] != 0.0f || m[7] != 0.0f || m[11] != 0.0f || m[15] != 1.0f) return false;
    double a[3][3];  // [row][col]
    for (int c = 0; c < 3; ++c)
        for (int r = 0; r < 3; ++r) { a[r][c] = m[4 * c + r]; S.a[3 * c + r] = m[4 * c + r]; }
    for (int r = 0; r < 3; ++r) S.t[r] = m[12 + r];
    double cof[3][3];  // cofactors: inverse transpose = cof / det
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) {
            const int r1 = (r + 1) % 3, r2 = (r + 2) % 3, c1 = (c + 1) % 3, c2 = (c + 2) % 3;
            cof[r][c] = a[r1][c1] * a[r2][c2] - a[r1][c2] * a[r2][c1];
        }
    const double det = a[0][0] * cof[0][0] + a[0][1] * cof[0][1] + a[0][2] * cof[0][2];
    if (det == 0.0 || !(det - det == 0.0)) return false;
    for (int c = 0; c < 3; ++c)
        for (int r = 0; r < 3; ++r) {
            const float v = (float)(cof[r][c] / det);
            if (!(v - v == 0.0f)) return false;
            S.nit[3 * c + r] = v;
        }
    return true;
}

// cpm_render_ex and cpm_render_shaded: shading == NULL or CPM_SHADE_NONE launches render_ex_kernel
static int render_ex_impl(cpm_ctx* ctx, const char* who, const cpm_volume* vol, const cpm_tf* tf, const float* light_volume, const cpm_grid_desc* grid,
                          const cpm_render_desc* desc, const cpm_render_options* options, const cpm_render_shading* shading, float* rgba_out,
                          cpm_stream stream) {
    RenderArgs A{};
    size_t lds = 0;
    int rc = render_prepare(ctx, who, vol, tf, light_volume, grid, desc, rgba_out, A, lds);
    if (rc) return rc;
    // a refusal of this layer, under the name of the entry point that was called
    auto refuse = [&](const char* why) { return set_error(ctx, CPM_ERR_INVALID_ARGUMENT, who, why); };
    RenderShadeArgs S{};
    if (shading) {
        const cpm_render_shading& H = *shading;
        CPM_REQUIRE(ctx, H.mode >= CPM_SHADE_NONE && H.mode <= CPM_SHADE_PHONG, "cpm_render_shaded: unknown shading mode");
        if (H.mode != CPM_SHADE_NONE) {
            for (int a = 0; a < 3; ++a) {
                const float f[4] = { H.light_position[a], H.ambient[a], H.diffuse[a], H.specular[a] };
                for (float v : f) CPM_REQUIRE(ctx, v - v == 0.0f, "cpm_render_shaded: the light position and the colours must be finite");
                S.light[a] = f[0]; S.ka[a] = f[1]; S.kd[a] = f[2]; S.ks[a] = f[3];
            }
            CPM_REQUIRE(ctx, H.shininess > 0.0f && H.shininess <= 3.402823466e+38f, "cpm_render_shaded: shininess must be finite and > 0");
            CPM_REQUIRE(ctx, shade_matrices(H.texture_to_world, S),
                        "cpm_render_shaded: texture_to_world must be finite and affine (last row 0 0 0 1) with an invertible linear part");
            S.mode = H.mode;
            S.shininess = H.shininess;
            for (int a = 0; a < 3; ++a) {
                S.h[a] = 1.0f / (float)vol->desc.dims[a];
                S.s[a] = 0.5f * (float)vol->desc.dims[a];
            }
        }
    }
    const cpm_render_accel* accel = options ? options->accel : nullptr;
    const float* clip = options ? options->clip_aabb : nullptr;
    uint32_t* stats = options ? options->stats : nullptr;
    RenderExArgs X{};
    for (int a = 0; a < 3; ++a) { X.clip_lo[a] = 0.0f; X.clip_hi[a] = 1.0f; }
    if (clip) {
        for (int a = 0; a < 3; ++a) {
            const float lo = clip[a], hi = clip[4 + a];
            if (!(lo - lo == 0.0f && hi - hi == 0.0f && lo < hi)) return refuse("the clip box must be finite with min < max on every axis");
            X.clip_lo[a] = lo; X.clip_hi[a] = hi;
        }
    }
    int mode = R_EX | (S.mode != CPM_SHADE_NONE ? R_SHADE : 0);
    if (accel) {
        const cpm_volume_desc& vd = vol->desc;
        if (!(accel->have_range && accel->have_bits)) return refuse("the accel was never fully updated");
        if (!(accel->vol == vol && accel->tf == tf)) return refuse("the accel's last update saw another volume or TF");
        if (!(accel->dims[0] == vd.dims[0] && accel->dims[1] == vd.dims[1] && accel->dims[2] == vd.dims[2] && accel->dtype == vd.dtype))
            return refuse("the accel was made for other dims or another voxel type");
        if (!(accel->tf_width == tf->width)) return refuse("the accel's last update saw another TF width");
        mode |= R_SKIP;
        X.bits = accel->bits;
        X.lg = accel->lg;
        X.nbx = accel->nb[0];
        X.nbxy = accel->nb[0] * accel->nb[1];
        X.last_bx = (float)((vd.dims[0] > 2 ? vd.dims[0] - 2 : 0) >> accel->lg);
        X.last_by = (float)((vd.dims[1] > 2 ? vd.dims[1] - 2 : 0) >> accel->lg);
        X.last_bz = (float)((vd.dims[2] > 2 ? vd.dims[2] - 2 : 0) >> accel->lg);
        const size_t bits_bytes = (size_t)accel->n_words * sizeof(uint32_t);
        if ((long long)bits_bytes <= (long long)ctx->dbg.render_bits_lds && lds + bits_bytes <= ctx->lds_per_block) {
            X.bits_words = accel->n_words;
            lds += bits_bytes;
        }
    }
    if (stats) { mode |= R_STATS; X.stats = stats; }
    hipStream_t s = (hipStream_t)stream;
    rc = render_volume(ctx, vol, s, A);
    if (rc) return rc;

    const dim3 g(div_up(A.width, 16), div_up(A.height, 16)), b(256);
#define CPM_RENDER_EX_LAUNCH_M(DT, CH)                                                                                    \
    do {                                                                                                                  \
        switch (mode) {                                                                                                   \
            case R_EX: CPM_LAUNCH(ctx, (render_ex_kernel<DT, CH, R_EX>), g, b, lds, s, A, X); break;                       \
            case R_EX | R_SKIP: CPM_LAUNCH(ctx, (render_ex_kernel<DT, CH, R_EX | R_SKIP>), g, b, lds, s, A, X); break;     \
            case R_EX | R_STATS: CPM_LAUNCH(ctx, (render_ex_kernel<DT, CH, R_EX | R_STATS>), g, b, lds, s, A, X); break;   \
            case R_EX | R_SKIP | R_STATS: CPM_LAUNCH(ctx, (render_ex_kernel<DT, CH, R_EX | R_SKIP | R_STATS>), g, b, lds, s, A, X); break; \
            case R_SHADE | R_EX: CPM_LAUNCH(ctx, (render_shaded_kernel<DT, CH, R_SHADE | R_EX>), g, b, lds, s, A, X, S); break; \
            case R_SHADE | R_EX | R_SKIP: CPM_LAUNCH(ctx, (render_shaded_kernel<DT, CH, R_SHADE | R_EX | R_SKIP>), g, b, lds, s, A, X, S); break; \
            case R_SHADE | R_EX | R_STATS: CPM_LAUNCH(ctx, (render_shaded_kernel<DT, CH, R_SHADE | R_EX | R_STATS>), g, b, lds, s, A, X, S); break; \
            default: CPM_LAUNCH(ctx, (render_shaded_kernel<DT, CH, R_SHADE | R_EX | R_SKIP | R_STATS>), g, b, lds, s, A, X, S); break; \
        }                                                                                                                 \
    } while (0)
#define CPM_RENDER_EX_LAUNCH(DT)                                                                            \
    do {                                                                                                    \
        if (grid->channels == 1) CPM_RENDER_EX_LAUNCH_M(DT, 1);                                             \
        else CPM_RENDER_EX_LAUNCH_M(DT, 4);                                                                 \
    } while (0)
    CPM_DISPATCH_DTYPE(vol->desc.dtype, CPM_RENDER_EX_LAUNCH);
#undef CPM_RENDER_EX_LAUNCH
#undef CPM_RENDER_EX_LAUNCH_M
    CPM_LAUNCH_CHECK(ctx, mode & R_SHADE ? "render_shaded_kernel" : "render_ex_kernel");
    return CPM_OK;
}

extern "C" {

int cpm_render_ex(cpm_ctx* ctx, const cpm_volume* vol, const cpm_tf* tf, const float* light_volume, const cpm_grid_desc* grid,
                  const cpm_render_desc* desc, const cpm_render_options* options, float* rgba_out, cpm_stream stream) {
    CPM_ENTER(ctx);
    return render_ex_impl(ctx, "cpm_render_ex", vol, tf, light_volume, grid, desc, options, nullptr, rgba_out, stream);
}

int cpm_render_shaded(cpm_ctx* ctx, const cpm_volume* vol, const cpm_tf* tf, const float* light_volume, const cpm_grid_desc* grid,
                      const cpm_render_desc* desc, const cpm_render_options* options, const cpm_render_shading* shading, float* rgba_out,
                      cpm_stream stream) {
    CPM_ENTER(ctx);
    return render_ex_impl(ctx, "cpm_render_shaded", vol, tf, light_volume, grid, desc, options, shading, rgba_out, stream);
}

}  // extern "C"
