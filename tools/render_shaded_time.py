#!/usr/bin/env python3
"""Gradient shading (cpm_render_shaded) against plain cpm_render_ex, same process, same inputs: config 2's 256^3 u8 volume, 1024 x 1024,
sampling rate 1, the box seen face-on and along a diagonal, the 128^3 light volume of one real frame.

TFs: the workspace TF (every sample is shaded) and case (c) of profiles/render_skip.json, the narrow-band TF (few samples are), each
without and with empty-space skipping.

Per TF, skipping and camera:
  * baseline: ms (median, min, max) of cpm_render_ex (whose kernels this feature leaves as they were) -- HIP events, 3 warm-up renders, then
    the median of 9 batches of 5;
  * per mode (none, ambient, diffuse, specular, blinn_phong, phong): the same for cpm_render_shaded, and baseline / mode.  Mode none is
    the baseline's kernel: "none_within_spread" says whether its median lies within the baseline's own min - max;
  * evaluated / skipped: the render's own counters (cpm_render_options::stats), exact.  shaded_estimate: NOT a counter -- stats has no
    word for it.  The share of samples with alpha > 0 that the numpy restatement (tests/render_reference.py) finds on a 64 x 64 image of
    the same view (other rays than the 1024 x 1024 image's), times the render's own sample count;
  * model: a shaded sample costs seven footprint fetches instead of one plus the light loads: with f = shaded / evaluated, fetches per
    evaluated sample go from 1 + f to 1 + 7 f ("fetch_model" = (1 + f) / (1 + 7 f), the baseline / mode ratio if fetches were all).
Prints one JSON line and writes it to --out.
usage: python tools/render_shaded_time.py [--out FILE] [--quick]"""
import json
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(REPO / "tests"))
import numpy as np
import torch

import cpm_amd
from render_skip_time import band_tf
from render_time import CAMERAS, W, H, device_ms

S, P, B = cpm_amd.synthetic, cpm_amd.pipeline, cpm_amd.binding
MODES = ["none", "ambient", "diffuse", "specular", "blinn_phong", "phong"]
UNIT_BOX = (0.0, 0.0, 0.0, 1.0, 1.0, 1.0, 1.0, 1.0)


def shaded_share(vol, tf, lv, m, step=16):
    """(samples with alpha > 0) / (samples taken), from the restatement on every `step`-th pixel"""
    import render_reference as R
    w, h = W // step, H // step
    # the same rays: pixel centres of the coarse image are not those of the fine one, but the share is a property of the view
    _, _, (taken, lit) = R.render(vol, tf, lv, (128, 128, 128), 1, w, h, ndc_to_texture=m, stats=True)
    return lit / max(taken, 1)


def main():
    quick = "--quick" in sys.argv
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else ""
    if not torch.cuda.is_available():
        raise SystemExit("render_shaded_time.py needs a GPU")
    ctx = B.Context(0)
    vol = S.heterogeneous_volume(256)
    img = torch.empty((H, W, 4), dtype=torch.float32, device=ctx.device)
    cases = []
    for name, tf in (("config 2, workspace TF", S.workspace_tf()), ("config 2, narrow-band TF (render_skip case c)", band_tf())):
        fr = P.PhotonFrame(ctx, vol, tf, 1024, (128, 128, 128), light_travel_direction=(0.3, 0.5, -1.0))
        fr.frame_fast()
        accel = ctx.render_accel(fr.vol, 8)
        accel.update(fr.vol, fr.tf)
        lv_np = fr.light_volume.cpu().numpy()
        for cam, (f, t, u, fov) in CAMERAS.items():
            m = B.camera_ndc_to_texture(f, t, u, fov, W / H, 0.1, 100.0)
            share = shaded_share(vol, tf, lv_np, m)
            for skip in (False, True):
                opts = dict(accel=accel) if skip else dict(clip=UNIT_BOX)   # either way cpm_render_ex / cpm_render_shaded

                def render(mode=None, stats=None):
                    sh = None if mode is None else B.Shading(mode=mode, light_position=(2.0, 3.0, 2.5), shininess=60.0)
                    ctx.render(fr.vol, fr.tf, fr.light_volume, fr.grid, W, H, ndc_to_texture=m, out=img, shading=sh, stats=stats, **opts)

                st = torch.zeros(2, dtype=torch.int32, device=ctx.device)
                render("phong", st)
                torch.cuda.synchronize()
                ev, sk = [int(v) & 0xffffffff for v in st.cpu().tolist()]
                row = {"case": name, "camera": cam, "skip": skip, "evaluated": ev, "skipped": sk,
                       "shaded_estimate": int(round(share * (ev + sk))), "shaded_share_of_evaluated_estimate": round(min(share * (ev + sk) / ev, 1.0), 4)}
                fsh = row["shaded_share_of_evaluated_estimate"]
                row["fetch_model"] = round((1 + fsh) / (1 + 7 * fsh), 3)
                if not quick:
                    bm, bl, bh = device_ms(lambda: render())
                    row["baseline_ms"] = {"median": round(bm, 4), "min": round(bl, 4), "max": round(bh, 4)}
                    for mode in MODES:
                        mm, ml, mh = device_ms(lambda: render(mode))
                        row[mode + "_ms"] = {"median": round(mm, 4), "min": round(ml, 4), "max": round(mh, 4)}
                        row["baseline_over_" + mode] = round(bm / mm, 3)
                    # the same kernel twice: compared against the baseline's spread, measured once more after the modes
                    am, al, ah = device_ms(lambda: render())
                    row["baseline_again_ms"] = {"median": round(am, 4), "min": round(al, 4), "max": round(ah, 4)}
                    row["none_within_spread"] = bool(min(bl, al) <= row["none_ms"]["median"] <= max(bh, ah))
                cases.append(row)
        accel.close()
        fr.forget_described()
        del fr
    res = {"what": "cpm_render_shaded per mode against cpm_render_ex, 1024 x 1024, rate 1, config 2's 256^3 u8 volume, 128^3 light volume",
           "timing": "HIP events; median of 9 batches of 5 after 3 warm-up; the baseline is cpm_render_ex in the same process",
           "counts": "evaluated / skipped: the render's stats counters; shaded_estimate: restatement on a 64 x 64 image of the same view, scaled",
           "device": torch.cuda.get_device_name(0), "rows": cases}
    line = json.dumps(res)
    print(line)
    if out_path:
        Path(out_path).parent.mkdir(parents=True, exist_ok=True)
        Path(out_path).write_text(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
