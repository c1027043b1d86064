#!/usr/bin/env python3
"""Empty-space skipping (cpm_render_ex with a cpm_render_accel) against plain cpm_render, same process, same inputs: 1024 x 1024, sampling
rate 1, the box seen face-on and along a diagonal, 128^3 light volume of one real frame of the case's volume and TF.

Cases: (a) config 2 with the workspace TF (nothing to skip); (b) config 2 with a threshold TF transparent below 0.6; (c) config 2 with a
TF that is transparent but for a narrow band; (d) the blob-only volume with the workspace TF.

Per case and camera:
  * plain / skip: ms (median, min, max) of cpm_render and of cpm_render_ex with the accel -- HIP events, 3 warm-up renders, then the
    median of 9 batches of 5; the two images are compared bit for bit;
  * stats: samples evaluated / skipped by the skipping render, and the samples the plain loop evaluates (cpm_render_ex's own counters);
  * verdict: "faster" / "slower" when the medians differ by more than the plain path's own min - max spread in this run, else "within".
Per case: the share of empty bricks, and the two update costs on their own -- the range grid (a time step) and the bits (a TF edit).
--bits-lds BYTES: the largest set of empty bits staged into LDS (cpm_debug_set_render_bits_lds; default: the library's 4096);
--brick N: brick size (default 8).  Prints one JSON line and writes it to --out.
usage: python tools/render_skip_time.py [--out FILE] [--brick N] [--bits-lds BYTES] [--quick]"""
import json
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))
import numpy as np
import torch

import cpm_amd
from render_time import CAMERAS, W, H, device_ms

S, P, B = cpm_amd.synthetic, cpm_amd.pipeline, cpm_amd.binding


def threshold_tf(width=1024):
    tf = S.workspace_tf(width)
    x = (np.arange(width) + 0.5) / width
    tf[:, 3] = np.where(x < 0.6, 0.0, tf[:, 3])
    return tf


def band_tf(width=1024):
    tf = S.workspace_tf(width)
    x = (np.arange(width) + 0.5) / width
    tf[:, 3] = np.where((x > 0.70) & (x < 0.74), tf[:, 3], 0.0)
    return tf


def arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def main():
    quick = "--quick" in sys.argv
    out_path = arg("--out", "")
    brick, bits_lds = arg("--brick", 8), arg("--bits-lds", -1)
    if not torch.cuda.is_available():
        raise SystemExit("render_skip_time.py needs a GPU")
    ctx = B.Context(0)
    if bits_lds >= 0:
        ctx.lib.cpm_debug_set_render_bits_lds(ctx.h, bits_lds)
    config2, blob = S.heterogeneous_volume(256), S.blob_volume(256)
    todo = [("a: config 2, workspace TF", config2, S.workspace_tf()), ("b: config 2, threshold TF (transparent below 0.6)", config2, threshold_tf()),
            ("c: config 2, narrow-band TF", config2, band_tf()), ("d: blob-only volume, workspace TF", blob, S.workspace_tf())]
    img_p = torch.empty((H, W, 4), dtype=torch.float32, device=ctx.device)
    img_s = torch.empty((H, W, 4), dtype=torch.float32, device=ctx.device)
    cases = []
    for name, vol, tf in todo[:2] if quick else todo:
        fr = P.PhotonFrame(ctx, vol, tf, 1024, (128, 128, 128), light_travel_direction=(0.3, 0.5, -1.0))
        fr.frame_fast()
        accel = ctx.render_accel(fr.vol, brick)
        accel.update(fr.vol, fr.tf)
        nb, n_empty = accel.info()
        case = {"case": name, "bricks": list(nb), "empty_brick_share": round(n_empty / (nb[0] * nb[1] * nb[2]), 4), "cameras": []}
        if not quick:
            for key, kw in (("range_grid_update_ms", dict(vol=fr.vol)), ("bits_update_ms", dict(tf=fr.tf))):
                ms, lo, hi = device_ms(lambda: accel.update(**kw))
                case[key] = {"median": round(ms, 4), "min": round(lo, 4), "max": round(hi, 4)}
        for cam, (f, t, u, fov) in CAMERAS.items():
            m = B.camera_ndc_to_texture(f, t, u, fov, W / H, 0.1, 100.0)

            def plain():
                fr.render(W, H, ndc_to_texture=m, out=img_p)

            def skip():
                ctx.render(fr.vol, fr.tf, fr.light_volume, fr.grid, W, H, ndc_to_texture=m, out=img_s, accel=accel)
            st_p = torch.zeros(2, dtype=torch.int32, device=ctx.device)
            st_s = torch.zeros(2, dtype=torch.int32, device=ctx.device)
            ctx.render(fr.vol, fr.tf, fr.light_volume, fr.grid, W, H, ndc_to_texture=m, out=img_p, stats=st_p)
            ctx.render(fr.vol, fr.tf, fr.light_volume, fr.grid, W, H, ndc_to_texture=m, out=img_s, accel=accel, stats=st_s)
            plain()
            skip()
            torch.cuda.synchronize()
            same = bool(torch.equal(img_p.view(torch.int32), img_s.view(torch.int32)))
            sp, ss = [int(v) & 0xffffffff for v in st_p.cpu().tolist()], [int(v) & 0xffffffff for v in st_s.cpu().tolist()]
            row = {"camera": cam, "same_bits": same, "plain_samples": sp[0], "evaluated": ss[0], "skipped": ss[1]}
            if not quick:
                pm, pl, ph = device_ms(plain)
                sm, sl, sh = device_ms(skip)
                spread = ph - pl
                row.update({"plain_ms": {"median": round(pm, 4), "min": round(pl, 4), "max": round(ph, 4)},
                            "skip_ms": {"median": round(sm, 4), "min": round(sl, 4), "max": round(sh, 4)},
                            "plain_over_skip": round(pm / sm, 3),
                            "verdict": "faster" if sm < pm - spread else ("slower" if sm > pm + spread else "within")})
            case["cameras"].append(row)
        cases.append(case)
        accel.close()
        fr.forget_described()
        del fr
    res = {"what": "cpm_render_ex with a cpm_render_accel against cpm_render, 1024 x 1024, rate 1, 256^3 u8 volumes, 128^3 light volume",
           "timing": "HIP events; median of 9 batches of 5 after 3 warm-up; the baseline is plain cpm_render in the same process",
           "brick": brick, "bits_lds_max_bytes": bits_lds if bits_lds >= 0 else 4096, "device": torch.cuda.get_device_name(0), "cases": cases}
    line = json.dumps(res)
    print(line)
    if out_path:
        Path(out_path).parent.mkdir(parents=True, exist_ok=True)
        Path(out_path).write_text(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
