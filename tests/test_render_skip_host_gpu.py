"""PhotonFrame.render(skip_empty=True) (pipeline.py): the frame owns the skip structure and rebuilds the half of it that its own edits
outdate -- a TF edit, time steps -- so the image has the bits of skip_empty=False throughout, with the frame's clip box given to both.
LightingRaycasterHIP.emptySpaceSkipping (host/, through cpmh_render_ex): the same for the processor, following its inports."""
import numpy as np
import pytest

from test_render_gpu import matrix

pytestmark = pytest.mark.gpu
F32 = np.float32


def test_photon_frame_skip_empty_across_a_tf_edit_and_two_time_steps(ctx, cpm):
    import torch
    S, P = cpm.synthetic, cpm.pipeline
    steps = [S.blob_volume(64, c) for c in ((0.4, 0.5, 0.5), (0.5, 0.5, 0.5), (0.6, 0.5, 0.45))]
    fr = P.CorrelatedPhotonMapper(ctx, steps[0], S.workspace_tf(), 128, (32, 32, 32), light_travel_direction=(0.3, 0.5, -1.0))
    fr.tf_points = list(S.WORKSPACE_TF_POINTS)
    fr.full_frame()
    m = matrix(cpm, "diagonal", 80, 64)
    seen = []

    def check(what):
        # the clip box in both: `clip` without skipping, the frame's own aabb (the default of skip_empty) with it
        plain = fr.render(80, 64, ndc_to_texture=m, sampling_rate=1.5, clip=fr.aabb)
        st = torch.zeros(2, dtype=torch.int32, device=ctx.device)
        fast = fr.render(80, 64, ndc_to_texture=m, sampling_rate=1.5, skip_empty=True, stats=st)
        assert torch.equal(plain.view(torch.int32), fast.view(torch.int32)), what
        # ... and the unit-cube aabb of this frame is no box at all
        assert torch.equal(plain.view(torch.int32), fr.render(80, 64, ndc_to_texture=m, sampling_rate=1.5).view(torch.int32)), what
        assert plain[..., 3].max() > 0 and int(st[1]) > 0, what
        assert all(not torch.equal(plain, s) for s in seen), what
        seen.append(plain.clone())

    check("first frame")
    pts = list(S.WORKSPACE_TF_POINTS)
    pts[3] = (0.26,) + pts[3][1:]   # config 3's edit
    fr.set_transfer_function(pts)
    check("tf edit")
    for i in (1, 2):
        fr.set_volume(steps[i])
        check("time step %d" % i)
    assert fr._render_accel is not None


@pytest.fixture(scope="module")
def host(cpm, ctx):
    import ctypes as C
    import importlib
    hl = importlib.import_module(cpm.__name__ + ".hostlayer")
    lib = hl.load()   # after torch brought up the HIP runtime (the ctx fixture)
    for name, res, args in [("cpmh_tf_lut", None, [C.c_void_p, C.c_void_p]),
                            ("cpmh_light_volume_dims", None, [C.c_void_p, C.c_void_p, C.c_void_p]),
                            ("cpmh_download_light_volume", C.c_int, [C.c_void_p, C.c_void_p])]:
        f = getattr(lib, name)
        f.restype, f.argtypes = res, args
    return hl, lib


def test_lighting_raycaster_property_on_and_off(host, ctx, cpm):
    """LightingRaycasterHIP.emptySpaceSkipping: the same bits on and off, after a TF edit and after a time step on the volume inport; with
    a clip box set on the tracer, the skipping render is Context.render with that box"""
    import ctypes as C
    import torch
    hl, lib = host
    S = cpm.synthetic
    steps = np.stack([S.blob_volume(32, c) for c in ((0.4, 0.5, 0.5), (0.6, 0.5, 0.45))])
    d = cpm.pipeline._normalize((0.3, 0.5, -1.0))
    net = hl.HostNetwork(lib, steps[0], 64, np.array([0.5, 0.5, 0.5], F32) - F32(2.0) * d, d, S.WORKSPACE_TF_POINTS, size_option=2)
    net.evaluate(first=True)
    cam = dict(look_from=(1.6, 1.3, 2.0), look_to=(0.5, 0.5, 0.5), look_up=(0.0, 1.0, 0.0), fov_deg=40.0)
    seen = []

    def check(what):
        off = net.render(72, 56, sampling_rate=1.5, skip_empty=False, **cam)
        on = net.render(72, 56, sampling_rate=1.5, skip_empty=True, **cam)
        again = net.render(72, 56, sampling_rate=1.5, **cam)   # the property stays as it was set
        assert np.array_equal(off.view(np.uint32), on.view(np.uint32)) and np.array_equal(on.view(np.uint32), again.view(np.uint32)), what
        assert (off[..., 3] > 0).any() and all(not np.array_equal(off, s) for s in seen), what
        seen.append(off)

    check("first frame")
    pts = list(S.WORKSPACE_TF_POINTS)
    pts[3] = (0.26,) + pts[3][1:]
    net.set_transfer_function(pts)
    net.evaluate()
    check("tf edit")
    seq = hl.HostSequence(lib, steps)
    seq.attach(net)
    seq.step(net, 1.0)
    check("time step")
    seq.close()
    net.close()
    # the clip box: 32 slices cut to x 8..24, y 4..32, z 0..20
    net = hl.HostNetwork(lib, steps[0], 64, np.array([0.5, 0.5, 0.5], F32) - F32(2.0) * d, d, S.WORKSPACE_TF_POINTS, size_option=2)
    net.set_clip(8, 24, 4, 32, 0, 20)
    net.evaluate(first=True)
    on = net.render(72, 56, sampling_rate=1.5, skip_empty=True, **cam)
    m = net.last_render_matrix()
    dims = (C.c_int * 3)()
    ch = C.c_int()
    lib.cpmh_light_volume_dims(net.h, dims, C.byref(ch))
    lv = np.empty(int(np.prod(list(dims))) * ch.value, F32)
    assert lib.cpmh_download_light_volume(net.h, lv.ctypes.data) == 0
    lut = np.empty(4096, F32)
    lib.cpmh_tf_lut(net.h, lut.ctypes.data)
    box = (8 / 32, 4 / 32, 0.0, 1.0, 24 / 32, 1.0, 20 / 32, 1.0)
    want = ctx.render(ctx.volume_create(steps[0]), ctx.tf_create(lut.reshape(1024, 4)), torch.from_numpy(lv).to(ctx.device),
                      cpm.binding.default_grid_desc(tuple(dims), ch.value), 72, 56, ndc_to_texture=m, sampling_rate=1.5, clip=box).cpu().numpy()
    assert np.array_equal(on.view(np.uint32), want.view(np.uint32)) and (on[..., 3] > 0).any()
    off = net.render(72, 56, sampling_rate=1.5, skip_empty=False, **cam)
    assert not np.array_equal(on, off)   # unclipped without the property: the behaviour of cpm_render stays
    net.close()
