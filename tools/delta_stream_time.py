#!/usr/bin/env python3
"""Config 5's time step streamed from host memory, in full and as deltas (cpm_sequence_delta), beside the resident step: bench.py's walk
(steps 0 - 7 of the 32-step 256^3 sequence round and round, 48 steps, step t + 1 prefetched before step t's update is enqueued, one
synchronisation at the end), the three variants alternated in one process, best of 3 each.  Also: the delta walk's copy stream alone
(uploads without the update) and the per-kernel times of its launches (patch, re-layout) from HIP events.
Prints one JSON line.
usage: python tools/delta_stream_time.py [--out FILE]"""
import json
import sys
import time

sys.path.insert(0, ".")
import numpy as np
import torch

import cpm_amd

S, P, B = cpm_amd.synthetic, cpm_amd.pipeline, cpm_amd.binding
LIGHT_DIR = (0.3, 0.5, -1.0)
vdim, gdim, lattice, n_steps = 256, 128, 1024, 8

ctx = B.Context(0)
seq_np = [S.heterogeneous_volume(vdim, S.sequence_blob_center(t, 32)) for t in range(n_steps)]
vols = [ctx.volume_create(v) for v in seq_np]
cm = P.CorrelatedPhotonMapper(ctx, seq_np[0], S.workspace_tf(), lattice, (gdim,) * 3, light_travel_direction=LIGHT_DIR,
                              tf_points=list(S.WORKSPACE_TF_POINTS))
cm.full_frame()
walk = [k % n_steps for k in range(1, 6 * n_steps + 1)]
pinned = B.PinnedSequence(ctx, seq_np)
full_stream = B.VolumeStream(ctx, seq_np[0], n_slots=3)
delta = B.SequenceDelta(ctx, pinned, wrap=True)
delta_stream = B.VolumeStream(ctx, seq_np[0], n_slots=3)
delta_stream.use_delta(delta)


def run_walk(volume_of, before=None, update=True):
    if before is not None:
        before(-1)
    torch.cuda.synchronize(); ta = time.perf_counter()
    for j, t in enumerate(walk):
        if before is not None:
            before(j)
        v = volume_of(j, t)
        if update:
            cm.set_volume(v)
            cm.correlated_update()
    torch.cuda.synchronize()
    return (time.perf_counter() - ta) * 1e3 / len(walk)


def streamed(vs, update=True):
    def ahead(j):
        if j + 1 < len(walk):
            vs.prefetch(walk[j + 1], pinned.steps[walk[j + 1]])
    return run_walk(lambda j, t: vs.acquire(t, pinned.steps[t]), ahead, update)


variants = {"resident": lambda: run_walk(lambda j, t: vols[t]), "streamed": lambda: streamed(full_stream),
            "streamed_delta": lambda: streamed(delta_stream)}
for f in variants.values():
    f()
best = {k: float("inf") for k in variants}
for _ in range(3):
    for k, f in variants.items():
        best[k] = min(best[k], f())
torch.cuda.synchronize()
di, ds, si = delta.info(), delta_stream.delta_stats(), delta_stream.stats()
fi = full_stream.stats()
walk_bytes = [delta.transition(a, b)[1] for a, b in zip([walk[-1]] + walk[:-1], walk)]
# the copy stream alone: uploads of the delta walk without the update, and its launches' event times
copy_only = min(streamed(delta_stream, update=False) for _ in range(3))
ctx.profile_reset(); ctx.profile_enable(True)
streamed(delta_stream, update=False)
torch.cuda.synchronize()
kern = ctx.profile_collect()
ctx.profile_enable(False)
per_step = {name: round(ms / max(calls, 1), 4) for name, (ms, calls) in kern.items() if "delta_patch" in name or "quads" in name}
# the copy of the base slot's linear block (a 16 MiB device-to-device hipMemcpyAsync), alone, from events
src_d, dst_d = torch.empty(di.step_bytes, dtype=torch.uint8, device=ctx.device), torch.empty(di.step_bytes, dtype=torch.uint8, device=ctx.device)
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
d2d = []
for _ in range(20):
    e0.record(); dst_d.copy_(src_d); e1.record(); torch.cuda.synchronize()
    d2d.append(e0.elapsed_time(e1))
out = {
    "resident_step_ms": round(best["resident"], 4),
    "streamed_step_ms": round(best["streamed"], 4),
    "streamed_delta_step_ms": round(best["streamed_delta"], 4),
    "delta_bytes_per_step": int(np.mean(walk_bytes)),
    "step_bytes": int(di.step_bytes),
    "dirty_fraction": round(di.dirty_fraction, 4),
    "delta_h2d_ms": round(ds.delta_h2d_ms_total / max(ds.delta_uploads_timed, 1), 4),
    "full_h2d_ms": round(fi.upload_ms_total / max(fi.uploads_timed, 1), 4),
    "sequence_analysis_ms": round(di.analysis_ms, 2),
    "delta_uploads": int(ds.delta_uploads), "full_uploads": int(ds.full_uploads),
    "delta_transitions_stored": int(di.n_delta_transitions), "transitions": int(di.n_transitions),
    "copy_stream_only_step_ms": round(copy_only, 4),
    "copy_stream_kernel_ms_per_launch": per_step,
    "d2d_step_copy_ms": round(min(d2d[5:]), 4),
    "walk": f"steps 0-{n_steps - 1} of the 32-step {vdim}^3 u8 sequence round and round, {len(walk)} steps, prefetch t + 1 before step t's "
            "correlated update, one synchronisation at the end; resident / streamed in full / streamed as deltas alternated, best of 3 each",
    "notes": "delta_h2d_ms: HIP events around the block's H2D on the stream's H2D stream (mean per delta upload); sequence_analysis_ms: the host "
             "pre-pass over the 8 steps, once, outside the step; copy_stream_only_step_ms: the delta walk's uploads without the update; d2d_step_copy_ms: a 16 MiB device-to-device copy alone",
}
line = json.dumps(out)
print(line)
if "--out" in sys.argv:
    with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
        f.write(line + "\n")
full_stream.close(); delta_stream.close(); delta.close(); pinned.close()
