#!/usr/bin/env python3
"""Float volumes at config 2's shape (256^3, 1 048 576 photons, 128^3 light volume): one float field stored three ways -- u8 (the field
quantised), f16 (CPM_F16), and f32 holding the f16-widened values -- and what each costs:

  * trace_us: one cpm_trace of the 1 M photons, per store;
  * step_us: cpm_volume_step at region 8 -- f16's one-pass launch against f32's two (per-brick difference + min/max);
  * update_us: a device-source cpm_volume_update (copy + footprint re-layout in one launch), per store;
  * streamed step ms, f16 and f32, full uploads and delta uploads: config 5's walk (steps 0 - 7 of the 32-step moving blob round and round,
    48 steps, step t + 1 prefetched before step t's correlated update, one synchronisation at the end), with the resident step beside it.

Kernel figures are HIP-event times (torch.cuda.Event) over batches after warm-up, the median batch divided by its length; a walk is timed
the same way around its 48 steps.  Prints one JSON line.
usage: python tools/f16_time.py [--out FILE]"""
import json
import sys

sys.path.insert(0, ".")
import numpy as np
import torch

import cpm_amd

S, P, B = cpm_amd.synthetic, cpm_amd.pipeline, cpm_amd.binding
LIGHT_DIR = (0.3, 0.5, -1.0)
vdim, gdim, lattice, n_steps, region = 256, 128, 1024, 8, 8
WARMUP, BATCHES, PER_BATCH = 3, 7, 10


def field(t=None):
    u8 = S.heterogeneous_volume(vdim) if t is None else S.heterogeneous_volume(vdim, S.sequence_blob_center(t, 32))
    x = np.arange(vdim, dtype=np.float32)
    ripple = np.float32(0.003) * np.sin(np.float32(0.37) * x[None, None, :] + np.float32(0.21) * x[None, :, None] + x[:, None, None])
    return np.clip(u8.astype(np.float32) / np.float32(255.0) + ripple, 0, 1).astype(np.float16)


def stores(h):
    return {"u8": np.rint(h.astype(np.float32) * np.float32(255.0)).astype(np.uint8), "f16": h, "f32": h.astype(np.float32)}


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
out = {}
h = field()
# trace, per store
trace = {}
for name, arr in stores(h).items():
    fr = P.PhotonFrame(ctx, arr, S.workspace_tf(), lattice, (gdim,) * 3, light_travel_direction=LIGHT_DIR)
    trace[name] = device_us(fr.trace)
    del fr
    torch.cuda.synchronize()
out["trace_us"] = trace
# time step's brick analysis: f16 one pass against f32 two launches
h1 = field(1)
nb = (vdim // region) ** 3
step = {}
for name in ("f16", "f32"):
    a, b = stores(h)[name], stores(h1)[name]
    va, vb = ctx.volume_create(a), ctx.volume_create(b)
    diff = torch.zeros(nb, dtype=torch.float32, device=ctx.device)
    mm = torch.zeros((nb, 2), dtype=torch.int16, device=ctx.device)
    step[name] = device_us(lambda: ctx.volume_step(va, vb, region, diff, mm))
out["step_us"] = step
# device-source volume update (copy + re-layout)
update = {}
for name, arr in stores(h).items():
    v = ctx.volume_create(arr)
    src = torch.from_numpy(arr.copy()).to(ctx.device)
    update[name] = device_us(lambda: v.update(src))
out["update_us"] = update
# streamed steps, full and delta, f16 and f32
walk = [k % n_steps for k in range(1, 6 * n_steps + 1)]
fields = [field(t) for t in range(n_steps)]
walks = {}
for name in ("f16", "f32"):
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
out["shape"] = f"{vdim}^3 volume, {lattice * lattice} photons, {gdim}^3 light volume; field: config 2's volume / 255 + a 0.003 ripple, in f16"
out["notes"] = ("trace_us / step_us / update_us: HIP events, median of 7 batches of 10 after 3 warm-up calls; walk: steps 0-7 of config 5's "
                "32-step sequence round and round, 48 steps, prefetch t + 1 before step t's correlated update, median of 3 walks per variant")
line = json.dumps(out)
print(line)
if "--out" in sys.argv:
    with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
        f.write(line + "\n")
