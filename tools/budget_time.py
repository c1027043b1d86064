#!/usr/bin/env python3
"""The budgeted correlated update, timed: one evaluation and one continuation at budgets of 1 %, 5 % and 25 % for
  (a) the legacy budgeted chain (device_budget=False: count read-back, 31-bit sort of all keys, sort of the batch, plain trace, two splats),
  (b) the device-resident one (device_budget=True: cpm_selection_finish_budget / cpm_selection_select_pending),
  (c) the 100 % fused update, (d) a full frame,
at the shapes of BASELINE config 3 (TF edit) and config 5 (time step) as tools/bench_correlated.py builds them, with a change large
enough that more photons change than the budget admits.  HIP events around each call (the device time between them, host waits of the
call included) and the host's wall clock; median over the batches after warm-up.  Prints one JSON line; --out writes it to a file.
    python tools/budget_time.py [--quick] [--batches 9] [--out profiles/budget_update.json]"""
import argparse
import json
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import numpy as np
import torch
import cpm_amd

S, P, B = cpm_amd.synthetic, cpm_amd.pipeline, cpm_amd.binding

ap = argparse.ArgumentParser()
ap.add_argument("--quick", action="store_true", help="config 3 at 5 % only, 7 batches (for a kernel trace)")
ap.add_argument("--batches", type=int, default=9)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--out", default=None)
args = ap.parse_args()
batches = 7 if args.quick else max(args.batches, 7)
ctx = B.Context(0)
N_SIDE, GRID = 1024, (128,) * 3
LIGHT = (0.3, 0.5, -1.0)


def timed(calls):
    """calls: functions run back to back; returns per call (device ms between events, host wall ms, result)."""
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(calls) + 1)]
    torch.cuda.synchronize()
    wall, res = [], []
    ev[0].record()
    for i, f in enumerate(calls):
        t = time.perf_counter()
        res.append(f())
        wall.append((time.perf_counter() - t) * 1e3)
        ev[i + 1].record()
    torch.cuda.synchronize()
    return [(ev[i].elapsed_time(ev[i + 1]), wall[i], res[i]) for i in range(len(calls))]


def drain(cm):
    while cm.remaining > 0:
        cm.continue_update()


def med(xs):
    return round(float(np.median(xs)), 4)


def run_variant(cm, change, n_batches):
    """change(k): the k-th edit / time step (importance grid included, untimed).  One batch = change, evaluation, one continuation."""
    rows = []
    for k in range(args.warmup + n_batches):
        change(k)
        first = {}

        def evaluation():
            n = cm.correlated_update()
            first["changed"] = n + cm.remaining        # |C|: what it traced and what it left pending
            return n

        (e_dev, e_wall, n1), (c_dev, c_wall, n2) = timed([evaluation, cm.continue_update])
        rows.append((e_dev, e_wall, c_dev, c_wall, n1, n2, first["changed"], cm.last_path))
        drain(cm)
    r = rows[args.warmup:]
    return {"evaluation_ms": med([x[0] for x in r]), "evaluation_wall_ms": med([x[1] for x in r]),
            "continuation_ms": med([x[2] for x in r]), "continuation_wall_ms": med([x[3] for x in r]),
            "traced_first": int(np.median([x[4] for x in r])), "traced_continuation": int(np.median([x[5] for x in r])),
            "changed": int(np.median([x[6] for x in r])), "light_volume_path": r[-1][7], "batches": len(r)}


def mapper(vol, base, pct, device_budget):
    cm = P.CorrelatedPhotonMapper(ctx, vol, S.workspace_tf(), N_SIDE, GRID, light_travel_direction=LIGHT, tf_points=base,
                                  max_incremental_percent=pct, device_budget=device_budget)
    cm.full_frame()
    cm.full_frame()
    return cm


out = {"photons": N_SIDE * N_SIDE, "light_volume": list(GRID), "timing": "HIP events around each call, median of the batches after warm-up",
       "warmup": args.warmup}
budgets = (5.0,) if args.quick else (1.0, 5.0, 25.0)

# ---- config 3: a TF edit (point 4 moved from 0.2218 to 0.30 and back: more photons change than any of the budgets admits at once)
vol = S.heterogeneous_volume(256)
base = list(S.WORKSPACE_TF_POINTS)
edit = list(base)
edit[3] = (0.30,) + base[3][1:]
c3 = {}
for pct in budgets:
    for name, dev in (("legacy_chain", False), ("device_budget", True)):
        cm = mapper(vol, base, pct, dev)
        c3[f"{name}_{pct:g}pct"] = dict(run_variant(cm, lambda k: cm.set_transfer_function(edit if k % 2 == 0 else base), batches),
                                        budget=ctx.update_budget(cm.n, pct))
        del cm
cm = mapper(vol, base, 100.0, False)
c3["fused_100pct"] = run_variant(cm, lambda k: cm.set_transfer_function(edit if k % 2 == 0 else base), batches)
full = [timed([cm.full_frame])[0][0] for _ in range(batches + args.warmup)][args.warmup:]
c3["full_frame_ms"] = med(full)
del cm
out["config3_tf_edit"] = c3

# ---- config 5: time steps of a 32-step sequence (blob moving along x), two steps at a time, resident volumes
if not args.quick:
    n_steps = 32
    vols = [torch.from_numpy(S.heterogeneous_volume(256, S.sequence_blob_center(t, n_steps))).to(ctx.device) for t in range(0, n_steps, 2)]
    vol0 = S.heterogeneous_volume(256, S.sequence_blob_center(0, n_steps))
    c5 = {}

    def step(cm):
        return lambda k: cm.set_volume(vols[(k + 1) % len(vols)])

    for pct in budgets:
        for name, dev in (("legacy_chain", False), ("device_budget", True)):
            cm = mapper(vol0, base, pct, dev)
            c5[f"{name}_{pct:g}pct"] = dict(run_variant(cm, step(cm), batches), budget=ctx.update_budget(cm.n, pct))
            del cm
    cm = mapper(vol0, base, 100.0, False)
    c5["fused_100pct"] = run_variant(cm, step(cm), batches)
    full = [timed([cm.full_frame])[0][0] for _ in range(batches + args.warmup)][args.warmup:]
    c5["full_frame_ms"] = med(full)
    del cm
    out["config5_time_step"] = c5

line = json.dumps(out)
print(line)
if args.out:
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(out, indent=1) + "\n")
ctx.close()
