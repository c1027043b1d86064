"""numpy restatement of cpm_render_shaded (include/cpm/cpm_ext.h, DESIGN.md "Gradient shading"): tests/render_reference.py plus the
shading of the classified colour behind c.a > 0, before the light volume multiplies it.

  * the gradient: float32, operation by operation -- six sample_volume values at the float32 positions one add away from p, the
    difference, one multiply by dim / 2 (the contract: the kernel's g has these bits);
  * the shading (x, N, V, L, H, R, the three terms): float64 from those float32 gradients, positions and directions.  `dtype=F32` evaluates
    the same formulas in float32 instead: what the tests measure the float32 kernel's legitimate deviation with;
  * rays, sample positions, lookups, compositing, opacity correction and early termination: the statements of render_reference.render,
    which mode NONE reproduces exactly.

A shading is a dict: mode (a number or a name of MODES), texture_to_world (16 floats, column-major, affine; None: identity),
light_position, ambient, diffuse, specular (3 floats each, world space / colours), shininess.
"""
import numpy as np

import render_reference as R

F32 = R.F32
NONE, AMBIENT, DIFFUSE, SPECULAR, BLINN_PHONG, PHONG = range(6)
MODES = {"none": NONE, "ambient": AMBIENT, "diffuse": DIFFUSE, "specular": SPECULAR, "blinn_phong": BLINN_PHONG, "phong": PHONG}


def mode_of(shading):
    if shading is None:
        return NONE
    m = shading.get("mode", NONE)
    return MODES[m.lower()] if isinstance(m, str) else int(m)


def gradient(vol, p, format_scaling=0.0, format_offset=0.0):
    """g [..., 3] float32 at texture-space points p [..., 3] float32: central differences of sample_volume over one voxel."""
    p = np.asarray(p, F32)
    dims = vol.shape[::-1]
    g = []
    for a in range(3):
        h = F32(1) / F32(dims[a])
        pp, pm = p.copy(), p.copy()
        pp[..., a] = p[..., a] + h
        pm[..., a] = p[..., a] - h
        d = R.sample_volume(vol, pp, format_scaling, format_offset) - R.sample_volume(vol, pm, format_scaling, format_offset)
        g.append((d.astype(F32) * (F32(0.5) * F32(dims[a]))).astype(F32))
    return np.stack(g, -1)


def matrices(shading):
    """(A [3, 3], t [3], inverse transpose of A) in float64 from the float32 texture_to_world"""
    m = shading.get("texture_to_world")
    m = np.eye(4, dtype=F32) if m is None else np.asarray(m, F32).reshape(4, 4).T   # column-major -> M @ p
    A = m[:3, :3].astype(np.float64)
    return A, m[:3, 3].astype(np.float64), np.linalg.inv(A).T


def normalize0(v):
    """v / |v| in v's own type; the zero vector stays zero"""
    l2 = (v * v).sum(-1, keepdims=True)
    with np.errstate(all="ignore"):
        inv = np.where(l2 > 0, v.dtype.type(1) / np.sqrt(l2), v.dtype.type(0))
    return v * inv


def shade(c, g, p, d, shading, dtype=np.float64):
    """the shaded colour [n, 3] (dtype) of TF colours c [n, 3] at samples p [n, 3] with gradients g [n, 3] on rays of texture-space
    direction d [n, 3] (all float32)"""
    mode = mode_of(shading)
    T = np.dtype(dtype).type
    A, t, nit = (x.astype(dtype) for x in matrices(shading))
    ka, kd, ks, light = (np.asarray(shading[k], F32).astype(dtype) for k in ("ambient", "diffuse", "specular", "light_position"))
    s = T(F32(shading["shininess"]))
    c = c.astype(dtype)
    n = c.shape[0]
    dif, spec = np.zeros(n, dtype), np.zeros(n, dtype)
    live = (g != 0).any(-1)
    if mode != AMBIENT and live.any():
        gl = g[live]
        _, e = np.frexp(np.abs(gl).max(-1, keepdims=True))   # the largest component to [1/2, 1): exact, and no square under- or overflows
        N = normalize0(np.ldexp(gl, -e).astype(dtype) @ nit.T)
        x = p[live].astype(dtype) @ A.T + t
        L = normalize0(light - x)
        V = -normalize0(d[live].astype(dtype) @ A.T)
        nl = (N * L).sum(-1)
        if mode != SPECULAR:
            dif[live] = np.abs(nl)
        if mode == BLINN_PHONG:
            H = normalize0(L + V)
            spec[live] = np.power(np.abs((N * H).sum(-1)), s)
        elif mode in (SPECULAR, PHONG):
            Rv = (T(2) * nl)[:, None] * N - L
            spec[live] = np.power(np.maximum((Rv * V).sum(-1), T(0)), s)
    return (ka * c + kd * c * dif[:, None] + ks * spec[:, None]).astype(dtype)


def render(vol, lut, light, light_dims, channels, width, height, *, shading=None, dtype=np.float64, ndc_to_texture=None, entry=None,
           exit=None, sampling_rate=1.0, colored_light=True, format_scaling=0.0, format_offset=0.0, stats=False):
    """render_reference.render with `shading` -> (image [H, W, 4] float64, ambiguous [H, W] bool) (+ (samples taken, samples shaded)
    with stats=True).  dtype: the type the shading formulas are evaluated in."""
    mode = mode_of(shading)
    lut = np.asarray(lut, F32)
    dz, dy, dx = vol.shape
    if entry is not None:
        e4, x4 = np.asarray(entry, F32), np.asarray(exit, F32)
        ent, ext, hit = e4[..., :3], x4[..., :3], e4[..., 3] != 0
    else:
        ent, ext, hit = R.camera_rays(ndc_to_texture, width, height)
    n, t_incr, d, live = R.sample_counts(ent, ext, hit, (dx, dy, dz), sampling_rate)
    ent, n, t_incr, d = ent.reshape(-1, 3), n.reshape(-1), t_incr.reshape(-1), d.reshape(-1, 3)
    expo = (t_incr * F32(R.REF_SAMPLING_INTERVAL)).astype(F32).astype(np.float64)
    res = np.zeros((n.size, 4), np.float64)
    ambiguous = np.zeros(n.size, bool)
    active = n > 0
    taken = fetched = 0
    k = 0
    while active.any():
        idx = np.nonzero(active)[0]
        t = ((F32(k) + F32(0.5)) * t_incr[idx]).astype(F32)
        p = (ent[idx] + t[:, None] * d[idx]).astype(F32)
        taken += idx.size
        c = R.sample_tf(lut, R.sample_volume(vol, p, format_scaling, format_offset))
        lit = c[:, 3] > 0
        if lit.any():
            li = idx[lit]
            fetched += li.size
            L = R.sample_light(light, light_dims, channels, p[lit])
            if channels == 4 and not colored_light:
                L = np.repeat(L[:, :1], 3, axis=1)
            if mode == NONE:
                rgb = (c[lit, :3] * L).astype(F32).astype(np.float64)
            else:
                g = gradient(vol, p[lit], format_scaling, format_offset) if mode != AMBIENT else np.zeros((li.size, 3), F32)
                rgb = (shade(c[lit, :3], g, p[lit], d[li], shading, dtype) * L.astype(dtype)).astype(np.float64)
            ap = -np.expm1(expo[li] * np.log1p(-c[lit, 3].astype(np.float64)))
            w = (1.0 - res[li, 3]) * ap
            res[li, :3] += w[:, None] * rgb
            res[li, 3] += w
            ambiguous[li] |= np.abs(res[li, 3] - R.ERT) <= R.AMBIGUOUS
            active[li[res[li, 3] > R.ERT]] = False
        k += 1
        active &= n > k
    img = res.reshape(height, width, 4)
    if stats:
        return img, ambiguous.reshape(height, width), (taken, fetched)
    return img, ambiguous.reshape(height, width)


def needed_rtol(got, want, atol):
    """the smallest rtol with |got - want| <= atol + rtol |want| everywhere (0 where atol alone suffices)"""
    d = np.abs(np.asarray(got, np.float64) - want) - atol
    with np.errstate(all="ignore"):
        r = np.where(d > 0, d / np.abs(want), 0.0)
    return float(np.nanmax(r)) if r.size else 0.0
