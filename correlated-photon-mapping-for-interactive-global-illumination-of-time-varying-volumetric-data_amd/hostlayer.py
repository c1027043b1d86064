"""ctypes access to libcpm_host.so's C facade (host/cpm_host_c.cpp): the C++ Processor/Port layer as bench.py drives it.

Load it AFTER torch has initialised its HIP runtime (a second libamdhip64 brought up first does not see the GPU)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import binding as B
from . import build as _build


def load():
    _build.build_host_library(verbose=False)
    lib = C.CDLL(str(B.LIB_PATH.parent / "libcpm_host.so"))
    vp, i32 = C.c_void_p, C.c_int
    sigs = {
        "cpmh_create": (vp, [vp, i32, i32, i32, i32, i32, i32, C.POINTER(C.c_float * 3), C.POINTER(C.c_float * 3), vp, i32, i32, i32, i32]),
        "cpmh_destroy": (None, [vp]),
        "cpmh_evaluate": (i32, [vp, i32]),
        "cpmh_set_transfer_function": (None, [vp, vp, i32]),
        "cpmh_set_property_float": (i32, [vp, C.c_char_p, C.c_char_p, C.c_float]),
        "cpmh_set_property_string": (i32, [vp, C.c_char_p, C.c_char_p, C.c_char_p]),
        "cpmh_set_property_vec3": (i32, [vp, C.c_char_p, C.c_char_p, C.POINTER(C.c_float * 3)]),
        "cpmh_n_photons": (i32, [vp]),
        "cpmh_n_recomputed": (i32, [vp]),
        "cpmh_remaining": (i32, [vp]),
        "cpmh_refine": (i32, [vp]),
        "cpmh_tracer_host_waits": (i32, [vp]),
        "cpmh_download_photons": (i32, [vp, vp]),
        "cpmh_last_light_volume_path": (C.c_char_p, [vp]),
        "cpmh_last_tracer_decision": (C.c_char_p, [vp]),
        "cpmh_path_costs": (None, [vp, vp]),
        "cpmh_bench_tf_edits": (i32, [vp, vp, i32, vp, i32, i32, vp, vp]),
        "cpmh_bench_tf_edits_timeline": (i32, [vp, vp, i32, vp, i32, i32, vp]),
        "cpmh_bench_full_frames": (i32, [vp, i32, vp]),
        "cpmh_bench_frames_back_to_back": (i32, [vp, i32, vp, vp]),
        "cpmh_profile_full_frames": (C.c_char_p, [vp, i32]),
        "cpmh_add_light": (i32, [vp, C.POINTER(C.c_float * 3), C.POINTER(C.c_float * 3)]),
        "cpmh_n_lights": (i32, [vp]),
        "cpmh_set_clip": (None, [vp, i32, i32, i32, i32, i32, i32]),
        "cpmh_sequence_create": (vp, [vp, i32, i32, i32, i32, i32, i32]),
        "cpmh_sequence_destroy": (None, [vp]),
        "cpmh_sequence_keep_on_device": (None, [vp, i32]),
        "cpmh_sequence_stream_stats": (i32, [vp, vp]),
        "cpmh_sequence_upload_changes_only": (None, [vp, i32]),
        "cpmh_sequence_delta_stats": (i32, [vp, vp]),
        "cpmh_attach_sequence": (i32, [vp, vp]),
        "cpmh_sequence_step": (i32, [vp, vp, C.c_float, vp]),
        "cpmh_sequence_step_total": (i32, [vp, vp, C.c_float, vp]),
        "cpmh_render": (i32, [vp, i32, i32, C.POINTER(C.c_float * 11), C.c_float, vp]),
        "cpmh_render_ex": (i32, [vp, i32, i32, C.POINTER(C.c_float * 11), C.c_float, i32, vp]),
        "cpmh_last_render_matrix": (None, [vp, vp]),
        "cpmh_last_render_texture_to_world": (None, [vp, vp]),
        "cpmh_set_volume_matrices": (None, [vp, vp, vp]),
    }
    for name, (res, args) in sigs.items():
        f = getattr(lib, name)
        f.restype, f.argtypes = res, args
    return lib


class HostNetwork:
    """The CorrelatedPhotonMappingSingleVolume network in C++ (sample generator -> light sampler -> tracer -> light volume,
    min/max -> importance -> tracer): cpmh_create's wiring.  The volume's numpy type picks the format (uint8, uint16, float32, float16, int16)."""

    def __init__(self, lib, volume_u8, n_side, light_position, light_direction, tf_points, size_option=2, max_scattering=1,
                 correlated=True):
        self.lib = lib
        vol = np.ascontiguousarray(volume_u8)
        pts = np.ascontiguousarray(np.asarray(tf_points, np.float32))
        self.max_scattering = max_scattering
        self.h = lib.cpmh_create(vol.ctypes.data, B._np_dtype_code(vol.dtype), vol.shape[2], vol.shape[1], vol.shape[0], n_side, n_side,
                                 C.byref((C.c_float * 3)(*light_position)), C.byref((C.c_float * 3)(*light_direction)),
                                 pts.ctypes.data, pts.shape[0], size_option, max_scattering, int(correlated))
        if not self.h:
            raise RuntimeError("cpmh_create failed")

    def evaluate(self, first=False):
        if self.lib.cpmh_evaluate(self.h, int(first)) != 0:
            raise RuntimeError("cpmh_evaluate failed")

    def set_float(self, processor: str, prop: str, value: float):
        if self.lib.cpmh_set_property_float(self.h, processor.encode(), prop.encode(), float(value)) != 0:
            raise KeyError(f"{processor}.{prop}")

    def set_string(self, processor: str, prop: str, value: str):
        if self.lib.cpmh_set_property_string(self.h, processor.encode(), prop.encode(), value.encode()) != 0:
            raise KeyError(f"{processor}.{prop}")

    def set_vec3(self, processor: str, prop: str, value):
        if self.lib.cpmh_set_property_vec3(self.h, processor.encode(), prop.encode(), C.byref((C.c_float * 3)(*value))) != 0:
            raise KeyError(f"{processor}.{prop}")

    def set_shading(self, mode, light_position=None, ambient=None, diffuse=None, specular=None, shininess=None):
        """The raycaster's `lighting` properties (Inviwo's SimpleLightingProperty ids): shadingMode (a name of binding.SHADE_MODES or its
        number; "none", the default, keeps cpm_render's images), and whichever of the others are given."""
        self.set_float("raycaster", "shadingMode", B.SHADE_MODES[mode.lower()] if isinstance(mode, str) else int(mode))
        for prop, v in (("lightPosition", light_position), ("lightColorAmbient", ambient), ("lightColorDiffuse", diffuse),
                        ("lightColorSpecular", specular)):
            if v is not None:
                self.set_vec3("raycaster", prop, np.broadcast_to(np.asarray(v, np.float32), (3,)).tolist())
        if shininess is not None:
            self.set_float("raycaster", "materialShininess", shininess)

    def set_transfer_function(self, tf_points):
        pts = np.ascontiguousarray(np.asarray(tf_points, np.float32))
        self.lib.cpmh_set_transfer_function(self.h, pts.ctypes.data, pts.shape[0])

    def refine(self):
        """One firing of the refinement timer and the evaluation it causes (a pending correlated update continues with its next batch)."""
        if self.lib.cpmh_refine(self.h) < 0:
            raise RuntimeError("cpmh_refine failed")

    @property
    def n_recomputed(self):
        """Photons the last evaluation re-traced (-1: all of them)."""
        return int(self.lib.cpmh_n_recomputed(self.h))

    @property
    def remaining(self):
        """Changed photons the update budget has left for the timer's evaluations."""
        return int(self.lib.cpmh_remaining(self.h))

    @property
    def host_waits(self):
        """Times the tracer has blocked on a device count between its importance pass and its trace."""
        return int(self.lib.cpmh_tracer_host_waits(self.h))

    def photons(self):
        """The photon records, (I * N, 8) float32, interaction by interaction."""
        out = np.zeros((self.n_photons * self.max_scattering, 8), np.float32)
        if self.lib.cpmh_download_photons(self.h, out.ctypes.data) != 0:
            raise RuntimeError("cpmh_download_photons failed")
        return out

    @property
    def n_photons(self):
        return int(self.lib.cpmh_n_photons(self.h))

    @property
    def last_path(self):
        return self.lib.cpmh_last_light_volume_path(self.h).decode()

    @property
    def last_decision(self):
        return self.lib.cpmh_last_tracer_decision(self.h).decode()

    def path_costs(self):
        c = (C.c_float * 4)()
        self.lib.cpmh_path_costs(self.h, C.byref(c))
        return {"full_trace_ms": c[0], "full_light_volume_ms": c[1], "branch_trace_ms": c[2], "branch_light_volume_ms": c[3]}

    def bench_tf_edits(self, points_a, points_b, reps):
        a = np.ascontiguousarray(np.asarray(points_a, np.float32))
        b = np.ascontiguousarray(np.asarray(points_b, np.float32))
        ms, n = (C.c_double * reps)(), (C.c_int * reps)()
        if self.lib.cpmh_bench_tf_edits(self.h, a.ctypes.data, a.shape[0], b.ctypes.data, b.shape[0], reps, C.byref(ms), C.byref(n)) != 0:
            raise RuntimeError("cpmh_bench_tf_edits failed")
        return np.array(list(ms)), np.array(list(n))

    def bench_tf_edits_timeline(self, points_a, points_b, reps):
        """Host clock since the edit after: property set, importance, tracer, light volume returned, device idle -> (reps, 5) ms."""
        a = np.ascontiguousarray(np.asarray(points_a, np.float32))
        b = np.ascontiguousarray(np.asarray(points_b, np.float32))
        ms = (C.c_double * (5 * reps))()
        if self.lib.cpmh_bench_tf_edits_timeline(self.h, a.ctypes.data, a.shape[0], b.ctypes.data, b.shape[0], reps, C.byref(ms)) != 0:
            raise RuntimeError("cpmh_bench_tf_edits_timeline failed")
        return np.array(list(ms)).reshape(reps, 5)

    def bench_full_frames(self, reps):
        """Latency: every frame timed from an idle device until it is idle again."""
        ms = (C.c_double * reps)()
        if self.lib.cpmh_bench_full_frames(self.h, reps, C.byref(ms)) != 0:
            raise RuntimeError("cpmh_bench_full_frames failed")
        return np.array(list(ms))

    def bench_frames_back_to_back(self, reps):
        """Throughput: `reps` full frames enqueued back to back, one synchronisation; (ms per frame, host enqueue ms per frame)."""
        total, host = C.c_double(0), C.c_double(0)
        if self.lib.cpmh_bench_frames_back_to_back(self.h, reps, C.byref(total), C.byref(host)) != 0:
            raise RuntimeError("cpmh_bench_frames_back_to_back failed")
        return total.value / reps, host.value / reps

    def profile_full_frames(self, reps):
        """{kernel name: ms per frame} over `reps` full frames (HIP events around every launch)."""
        text = self.lib.cpmh_profile_full_frames(self.h, reps).decode()
        return {k: float(v) for k, v in (item.split("=") for item in text.split(";") if item)}

    def render(self, width, height, look_from, look_to, look_up=(0.0, 1.0, 0.0), fov_deg=38.0, aspect=None, sampling_rate=2.0, skip_empty=None):
        """LightingRaycasterHIP over the network's volume, TF and light volume as the last evaluate() left them:
        (height, width, 4) float32 RGBA, row 0 = the bottom row (near / far: the processor's 0.1 / 100).
        skip_empty: True / False sets the processor's emptySpaceSkipping property first (cpmh_render_ex; with it on the rays are clipped to
        the tracer's clip box); None leaves it as it is."""
        cam = (C.c_float * 11)(*look_from, *look_to, *look_up, fov_deg, width / height if aspect is None else aspect)
        out = np.empty((height, width, 4), np.float32)
        if skip_empty is None:
            rc = self.lib.cpmh_render(self.h, width, height, C.byref(cam), sampling_rate, out.ctypes.data)
        else:
            rc = self.lib.cpmh_render_ex(self.h, width, height, C.byref(cam), sampling_rate, int(bool(skip_empty)), out.ctypes.data)
        if rc != 0:
            raise RuntimeError("cpmh_render failed")
        return out

    def last_render_matrix(self):
        """ndc -> texture matrix (16 float32, column-major) of the last render()."""
        m = np.empty(16, np.float32)
        self.lib.cpmh_last_render_matrix(self.h, m.ctypes.data)
        return m

    def set_volume_matrices(self, model=None, world=None):
        """The volume's model and world matrices, 4x4 in numpy convention (M @ p; None: identity): the raycaster's texture -> world is
        world @ model."""
        m, w = (np.ascontiguousarray((np.eye(4) if x is None else np.asarray(x, np.float64).reshape(4, 4)).T, np.float32) for x in (model, world))
        self.lib.cpmh_set_volume_matrices(self.h, m.ctypes.data, w.ctypes.data)

    def last_render_texture_to_world(self):
        """texture -> world matrix (16 float32, column-major) of the volume the last render() saw."""
        m = np.empty(16, np.float32)
        self.lib.cpmh_last_render_texture_to_world(self.h, m.ctypes.data)
        return m

    def add_light(self, light_position, light_direction):
        return int(self.lib.cpmh_add_light(self.h, C.byref((C.c_float * 3)(*light_position)), C.byref((C.c_float * 3)(*light_direction))))

    def set_clip(self, x0, x1, y0, y1, z0, z1):
        self.lib.cpmh_set_clip(self.h, x0, x1, y0, y1, z0, z1)

    def close(self):
        if self.h:
            self.lib.cpmh_destroy(self.h)
            self.h = None


class HostSequence:
    def __init__(self, lib, volumes_u8, region=8):
        self.lib = lib
        v = np.ascontiguousarray(volumes_u8)
        self.h = lib.cpmh_sequence_create(v.ctypes.data, B._np_dtype_code(v.dtype), v.shape[3], v.shape[2], v.shape[1], v.shape[0], region)
        if not self.h:
            raise RuntimeError("cpmh_sequence_create failed")

    def attach(self, net: HostNetwork):
        if self.lib.cpmh_attach_sequence(net.h, self.h) != 0:
            raise RuntimeError("cpmh_attach_sequence failed")

    def step(self, net: HostNetwork, time: float):
        t = (C.c_double * 2)()
        n = self.lib.cpmh_sequence_step(net.h, self.h, float(time), C.byref(t))
        if n < -1:
            raise RuntimeError("cpmh_sequence_step failed")
        return n, t[0], t[1]

    def step_total(self, net: HostNetwork, time: float):
        """One displayed time, everything enqueued back to back, one synchronisation: (photons re-traced, ms)."""
        t = C.c_double(0)
        n = self.lib.cpmh_sequence_step_total(net.h, self.h, float(time), C.byref(t))
        if n < -1:
            raise RuntimeError("cpmh_sequence_step_total failed")
        return n, t.value

    def keep_on_device(self, keep: bool):
        """False: the elements stay in host memory and are streamed through the player's ring of device volumes (cpm_volume_stream)."""
        self.lib.cpmh_sequence_keep_on_device(self.h, int(bool(keep)))

    def stream_stats(self):
        """{"uploads", "upload_ms", "bytes_per_step", "uploads_at_acquire"} of the streaming player, or None when it keeps the sequence resident."""
        out = (C.c_double * 4)()
        if self.lib.cpmh_sequence_stream_stats(self.h, out) != 0:
            return None
        return {"uploads": int(out[0]), "upload_ms": float(out[1]), "bytes_per_step": int(out[2]), "uploads_at_acquire": int(out[3])}

    def upload_changes_only(self, on: bool):
        """With keep_on_device(False): compare the elements once and upload only what changed since the element before when that element is
        in the player's ring (cpm_sequence_delta)."""
        self.lib.cpmh_sequence_upload_changes_only(self.h, int(bool(on)))

    def delta_stats(self):
        """{"delta_uploads", "full_uploads", "delta_bytes", "analysis_ms"} of a player that uploads changes only, or None."""
        out = (C.c_double * 4)()
        if self.lib.cpmh_sequence_delta_stats(self.h, out) != 0:
            return None
        return {"delta_uploads": int(out[0]), "full_uploads": int(out[1]), "delta_bytes": int(out[2]), "analysis_ms": float(out[3])}

    def close(self):
        if self.h:
            self.lib.cpmh_sequence_destroy(self.h)
            self.h = None
