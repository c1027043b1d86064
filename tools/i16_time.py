#!/usr/bin/env python3
"""Signed 16-bit volumes at config 2's shape (256^3, 1 048 576 photons, 128^3 light volume): config 2's volume requantised to int16 over
the type's whole range, and the same normalised field stored as u16, f16 and f32 -- and what each costs:

  * trace_us: one cpm_trace of the 1 M photons, per store (i16 under its default mapping, offset 1 / scaling 0.5);
  * step_us: cpm_volume_step at region 8 -- i16's two per-brick launches beside u16's and f16's one-pass row kernel;
  * streamed step ms for i16 and u16, full uploads and delta uploads: config 5's walk (steps 0 - 7 of the 32-step moving blob round and
    round, 48 steps, step t + 1 prefetched before step t's correlated update, one synchronisation at the end), the resident step beside it.

--without-i16 leaves the type out, so that a library built from the commit before it (CPM_LIB=...) runs the same script: the figures that
show whether the existing kernels moved.

Kernel figures are HIP-event times (torch.cuda.Event) over batches after warm-up, the median batch divided by its length; a walk is timed
the same way around its 48 steps.  Prints one JSON line.
usage: python tools/i16_time.py [--without-i16] [--out FILE]"""
import json
import sys

sys.path.insert(0, ".")
import numpy as np
import torch

import cpm_amd

S, P, B = cpm_amd.synthetic, cpm_amd.pipeline, cpm_amd.binding
HAVE_I16 = hasattr(B, "CPM_I16") and "--without-i16" not in sys.argv
LIGHT_DIR = (0.3, 0.5, -1.0)
vdim, gdim, lattice, n_steps, region = 256, 128, 1024, 8, 8
WARMUP, BATCHES, PER_BATCH = 3, 7, 10


def field(t=None):
    """config 2's volume (config 5's step t) as int16: (u8 / 255 * 2 - 1) * 32767, rounded"""
    u8 = S.heterogeneous_volume(vdim) if t is None else S.heterogeneous_volume(vdim, S.sequence_blob_center(t, 32))
    return np.rint((u8.astype(np.float64) / 255.0 * 2.0 - 1.0) * 32767.0).astype(np.int16)


def stores(v):
    """the same normalised field (w(v) + 1) / 2 in each store, up to the store's precision"""
    n = (v.astype(np.float32) * np.float32(1 / 32767) + np.float32(1)) * np.float32(0.5)
    out = {"i16": v} if HAVE_I16 else {}
    out.update({"u16": (v.astype(np.int32) + 32768).astype(np.uint16), "f16": n.astype(np.float16), "f32": n})
    return out


def device_us(fn, per_batch=PER_BATCH):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(WARMUP):
        fn()
    times = []
    for _ in range(BATCHES):
        e0.record()
        for _ in range(per_batch):
            fn()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) * 1e3 / per_batch)
    return round(float(np.median(times)), 2)


ctx = B.Context(0)
out = {"have_i16": HAVE_I16}
v0 = field()
# trace, per store, twice round (the second round shows what the order of measurement does to a figure)
trace = {}
for rnd in range(2):
    for name, arr in stores(v0).items():
        fr = P.PhotonFrame(ctx, arr, S.workspace_tf(), lattice, (gdim,) * 3, light_travel_direction=LIGHT_DIR)
        trace.setdefault(name, []).append(device_us(fr.trace))
        del fr
        torch.cuda.synchronize()
out["trace_us"] = trace
# the time step's brick analysis
v1 = field(1)
nb = (vdim // region) ** 3
step = {}
for name in [n for n in ("i16", "u16", "f16") if n in stores(v0)]:
    va, vb = ctx.volume_create(stores(v0)[name]), ctx.volume_create(stores(v1)[name])
    diff = torch.zeros(nb, dtype=torch.float32, device=ctx.device)
    mm = torch.zeros((nb, 2), dtype=torch.int16, device=ctx.device)
    step[name] = device_us(lambda: ctx.volume_step(va, vb, region, diff, mm))
    del va, vb
out["step_us"] = step
# streamed steps, full and delta
walk = [k % n_steps for k in range(1, 6 * n_steps + 1)]
fields = [field(t) for t in range(n_steps)]
walks = {}
for name in [n for n in ("i16", "u16") if n in stores(v0)]:
    seq_np = [stores(f)[name] for f in fields]
    vols = [ctx.volume_create(v) for v in seq_np]
    cm = P.CorrelatedPhotonMapper(ctx, seq_np[0], S.workspace_tf(), lattice, (gdim,) * 3, light_travel_direction=LIGHT_DIR,
                                  tf_points=list(S.WORKSPACE_TF_POINTS))
    cm.full_frame()
    pinned = B.PinnedSequence(ctx, seq_np)
    full_stream = B.VolumeStream(ctx, seq_np[0], n_slots=3)
    delta = B.SequenceDelta(ctx, pinned, wrap=True)
    delta_stream = B.VolumeStream(ctx, seq_np[0], n_slots=3)
    delta_stream.use_delta(delta)

    def run_walk(volume_of, ahead=None):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        if ahead is not None:
            ahead(-1)
        torch.cuda.synchronize()
        e0.record()
        for j, t in enumerate(walk):
            if ahead is not None:
                ahead(j)
            cm.set_volume(volume_of(t))
            cm.correlated_update()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / len(walk)

    def streamed(vs):
        def ahead(j):
            if j + 1 < len(walk):
                vs.prefetch(walk[j + 1], pinned.steps[walk[j + 1]])
        return run_walk(lambda t: vs.acquire(t, pinned.steps[t]), ahead)

    variants = {"resident": lambda: run_walk(lambda t: vols[t]), "streamed": lambda: streamed(full_stream),
                "streamed_delta": lambda: streamed(delta_stream)}
    for f in variants.values():
        f()
    res = {k: [] for k in variants}
    for _ in range(3):
        for k, f in variants.items():
            res[k].append(f())
    walks[name] = {k + "_step_ms": round(float(np.median(v)), 4) for k, v in res.items()}
    walks[name]["step_bytes"] = int(seq_np[0].nbytes)
    walks[name]["delta_bytes_per_step"] = int(np.mean([delta.transition(a, b)[1] for a, b in zip([walk[-1]] + walk[:-1], walk)]))
    full_stream.close(); delta_stream.close(); delta.close(); pinned.close()
    del cm, vols
    torch.cuda.synchronize()
out["walk"] = walks
out["shape"] = f"{vdim}^3 volume, {lattice * lattice} photons, {gdim}^3 light volume; field: config 2's volume as (u8 / 255 * 2 - 1) * 32767 in int16"
out["notes"] = ("trace_us (two rounds over the stores) / step_us: HIP events, median of 7 batches of 10 after 3 warm-up calls; walk: steps 0-7 of "
                "config 5's 32-step sequence round and round, 48 steps, prefetch t + 1 before step t's correlated update, median of 3 walks "
                "per variant")
line = json.dumps(out)
print(line)
if "--out" in sys.argv:
    with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
        f.write(line + "\n")
