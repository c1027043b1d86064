"""LightingRaycasterHIP's `lighting` properties (Inviwo's SimpleLightingProperty ids) through the C facade: the processor offers the six
ids; with shadingMode none cpmh_render gives the bits of plain Context.render; with Phong set through cpmh_set_property_* it gives the bits
of Context.render(shading=...) on the same volume, TF, light volume and matrices, with and without empty-space skipping; the network
evaluates as before afterwards."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
F32 = np.float32
LIGHTING_IDS = {"shadingMode", "lightPosition", "lightColorAmbient", "lightColorDiffuse", "lightColorSpecular", "materialShininess"}


@pytest.fixture(scope="module")
def host(cpm, ctx):
    import importlib
    hl = importlib.import_module(cpm.__name__ + ".hostlayer")
    lib = hl.load()   # after torch brought up the HIP runtime (the ctx fixture)
    for name, res, args in [("cpmh_tf_lut", None, [C.c_void_p, C.c_void_p]),
                            ("cpmh_light_volume_dims", None, [C.c_void_p, C.c_void_p, C.c_void_p]),
                            ("cpmh_download_light_volume", C.c_int, [C.c_void_p, C.c_void_p]),
                            ("cpmh_describe_surface", C.c_char_p, [C.c_void_p]),
                            ("cpmh_factory_create", C.c_char_p, [C.c_char_p])]:
        f = getattr(lib, name)
        f.restype, f.argtypes = res, args
    return hl, lib


def light_volume(lib, net):
    dims = (C.c_int * 3)()
    ch = C.c_int()
    lib.cpmh_light_volume_dims(net.h, dims, C.byref(ch))
    out = np.empty(int(np.prod(list(dims))) * ch.value, F32)
    assert lib.cpmh_download_light_volume(net.h, out.ctypes.data) == 0
    return tuple(dims), ch.value, out


def test_processor_offers_the_lighting_ids(host):
    _, lib = host
    props = lib.cpmh_factory_create(b"org.inviwo.LightingRaycasterHIP").decode().split("|")[3]
    assert LIGHTING_IDS | {"lighting", "supportColoredLight"} <= set(filter(None, props[5:].split(",")))


def test_phong_through_the_property_facade_is_context_render(host, ctx, cpm):
    import torch
    hl, lib = host
    S, B = cpm.synthetic, cpm.binding
    vol = S.heterogeneous_volume(32)
    d = cpm.pipeline._normalize((0.3, 0.5, -1.0))
    net = hl.HostNetwork(lib, vol, 64, np.array([0.5, 0.5, 0.5], F32) - F32(2.0) * d, d, S.WORKSPACE_TF_POINTS, size_option=2)
    net.evaluate(first=True)
    dims, ch, lv = light_volume(lib, net)
    surface = lib.cpmh_describe_surface(net.h)
    cam = dict(look_from=(1.6, 1.3, 2.0), look_to=(0.5, 0.5, 0.5), look_up=(0.0, 1.0, 0.0), fov_deg=40.0)
    lut = np.empty(4096, F32)
    lib.cpmh_tf_lut(net.h, lut.ctypes.data)
    v, t = ctx.volume_create(vol), ctx.tf_create(lut.reshape(1024, 4))
    lvt, g = torch.from_numpy(lv).to(ctx.device), B.default_grid_desc(dims, ch)

    def context_render(m, **kw):
        return ctx.render(v, t, lvt, g, 72, 56, ndc_to_texture=m, sampling_rate=1.5, **kw).cpu().numpy()

    # shadingMode none (the default, and set explicitly): today's bits
    plain = net.render(72, 56, sampling_rate=1.5, **cam)
    m = net.last_render_matrix()
    assert np.array_equal(plain.view(np.uint32), context_render(m).view(np.uint32)) and (plain[..., 3] > 0).mean() > 0.2
    net.set_shading("none", light_position=(9.0, 9.0, 9.0))
    assert np.array_equal(net.render(72, 56, sampling_rate=1.5, **cam).view(np.uint32), plain.view(np.uint32))
    # Phong through the facade
    sh = dict(light_position=(2.0, 3.0, 2.5), ambient=(0.2, 0.15, 0.1), diffuse=(0.6, 0.7, 0.5), specular=(0.4, 0.3, 0.5), shininess=12.0)
    net.set_shading("phong", **sh)
    img = net.render(72, 56, sampling_rate=1.5, **cam)
    t2w = net.last_render_texture_to_world()
    assert np.array_equal(t2w, B.texture_to_world())   # this network's volume carries identity model and world matrices
    want = context_render(net.last_render_matrix(), shading=B.Shading(mode="phong", texture_to_world=t2w, **sh))
    assert np.array_equal(img.view(np.uint32), want.view(np.uint32)) and not np.array_equal(img, plain)
    # a volume with model and world matrices of its own: neither symmetric, and they do not commute, so a transposed matrix, model * world
    # or no matrix at all would each give another image
    model = np.array([[2.0, 0.25, 0.0, -1.0], [0.0, 1.5, 0.125, -0.75], [0.0, 0.0, 1.0, -0.5], [0.0, 0.0, 0.0, 1.0]])
    world = np.array([[0.0, -1.0, 0.0, 0.5], [1.0, 0.0, 0.0, 0.25], [0.0, 0.0, 1.25, 0.0], [0.0, 0.0, 0.0, 1.0]])
    assert not np.allclose(world @ model, model @ world) and not np.allclose(world @ model, (world @ model).T)
    net.set_volume_matrices(model, world)
    to_world = lambda p: ((world @ model) @ np.array([*p, 1.0]))[:3]   # noqa: E731
    wcam = dict(look_from=to_world(cam["look_from"]), look_to=to_world(cam["look_to"]), look_up=cam["look_up"], fov_deg=cam["fov_deg"])
    moved = net.render(72, 56, sampling_rate=1.5, **wcam)
    t2w = net.last_render_texture_to_world()
    assert np.allclose(t2w, B.texture_to_world(model, world), rtol=1e-6, atol=1e-7)
    for wrong in (B.texture_to_world(world, model), B.texture_to_world(model.T, world.T), B.texture_to_world()):
        assert not np.allclose(t2w, wrong, atol=1e-3)
    m_moved = net.last_render_matrix()
    assert np.allclose(m_moved, B.camera_ndc_to_texture(**wcam, aspect=72 / 56, near=0.1, far=100.0, texture_to_world=world @ model),
                       rtol=1e-4, atol=1e-5)
    want_moved = context_render(m_moved, shading=B.Shading(mode="phong", texture_to_world=t2w, **sh))
    assert np.array_equal(moved.view(np.uint32), want_moved.view(np.uint32)) and (moved[..., 3] > 0).mean() > 0.05
    assert not np.array_equal(moved, context_render(m_moved, shading=B.Shading(mode="phong", **sh)))   # ... the matrix matters
    net.set_volume_matrices()
    # ... with empty-space skipping on (the property stays set): the same bits
    assert np.array_equal(net.render(72, 56, sampling_rate=1.5, skip_empty=True, **cam).view(np.uint32), want.view(np.uint32))
    net.render(72, 56, sampling_rate=1.5, skip_empty=False, **cam)
    # the defaults of the other properties are Inviwo's
    net2 = hl.HostNetwork(lib, vol, 64, np.array([0.5, 0.5, 0.5], F32) - F32(2.0) * d, d, S.WORKSPACE_TF_POINTS, size_option=2)
    net2.evaluate(first=True)
    lvt = torch.from_numpy(light_volume(lib, net2)[2]).to(ctx.device)   # (context_render reads it)
    net2.set_shading("blinn_phong")
    got = net2.render(72, 56, sampling_rate=1.5, **cam)
    want2 = context_render(net2.last_render_matrix(), shading=B.Shading(mode="blinn_phong"))
    assert np.array_equal(got.view(np.uint32), want2.view(np.uint32))
    net2.close()
    # an unknown property or processor is reported
    with pytest.raises(KeyError):
        net.set_vec3("raycaster", "lightColour", (1.0, 1.0, 1.0))
    with pytest.raises(KeyError):
        net.set_vec3("canvas", "lightPosition", (1.0, 1.0, 1.0))
    # rendering is not part of the frame: the light volume and the network's surface are what the evaluation left, and it evaluates again
    assert np.array_equal(light_volume(lib, net)[2].view(np.uint32), lv.view(np.uint32))
    assert lib.cpmh_describe_surface(net.h) == surface
    net.evaluate()
    assert light_volume(lib, net)[0] == dims and np.isfinite(light_volume(lib, net)[2]).all()
    net.close()
