"""The CPU oracle in libm = glibc-2.35 mode: oracle/*.c with -DORACLE_USE_LIBM, linked with tests/glibc_shim.c, whose hidden sinf / cosf /
sincosf / acosf / cos come from include/ssx_glibc_math.h.  simple_spectral_amd/build.py build_glibc_oracle (called by __graft_entry__.build())
writes it as oracle/libssx_oracle_glibc.so, i.e. tests/oracle_lib.py's variant "glibc": oracle_lib.Oracle(..., variant="glibc") and
oracle_lib.load("glibc") bind it as they bind the other variants.  Its results do not depend on the C library of the machine the tests run on.
Missing library: an error, not a skip (the GPU tests of the mode have no other reference)."""
import ctypes as C
import os

import numpy as np

import oracle_lib as ol

VARIANT = "glibc"


def library_path():
    from simple_spectral_amd import build as b
    return b.GLIBC_ORACLE


def load():
    path = library_path()
    if not os.path.exists(path):
        raise FileNotFoundError("%s is missing: build it with __graft_entry__.build() (simple_spectral_amd/build.py build_glibc_oracle)" % path)
    return ol.load(VARIANT)


def Oracle(*args, **kw):
    load()
    return ol.Oracle(*args, variant=VARIANT, **kw)


def custom_oracle(c):
    """The shim oracle over orc_scene_create_custom of a tests/custom_scene.py CustomScene: what CustomScene.oracle() makes for the default
    oracle, from the same public description (spectra, materials, textures, quads, kinds, camera)."""
    load()

    def make(lib, color):
        keep = []
        sp = (ol.SpectrumIn * len(c.spectra))()
        for i, (data, low, high) in enumerate(c.spectra):
            keep.append(np.ascontiguousarray(data, dtype=np.float32))
            sp[i].n = len(data); sp[i].low = low; sp[i].high = high
            sp[i].data = keep[-1].ctypes.data_as(C.POINTER(C.c_float))
        mt = (ol.MaterialIn * len(c.materials))()
        for i, m in enumerate(c.materials):
            mt[i].kind = m["kind"]; mt[i].albedo_mode = m["albedo_mode"]; mt[i].albedo_spectrum = m["albedo_spectrum"]
            mt[i].texture = m["albedo_texture"]; mt[i].emission_spectrum = m["emission_spectrum"]
        tx = (ol.TextureIn * max(1, len(c.textures)))()
        for i, t in enumerate(c.textures):
            keep.append(np.ascontiguousarray(t, dtype=np.uint8))
            tx[i].w = t.shape[1]; tx[i].h = t.shape[0]; tx[i].rgb = keep[-1].ctypes.data_as(C.POINTER(C.c_uint8))
        qs = (ol.QuadIn * len(c.quads))()
        for i, (pos, st, m) in enumerate(c.quads):
            for v in range(4):
                for k in range(3):
                    qs[i].pos[v][k] = float(pos[v][k])
                for k in range(2):
                    qs[i].st[v][k] = float(st[v][k])
            qs[i].material = m
            qs[i].kind = 1 if c.kinds.get(i) == "tri" else 0
        pv = (C.c_double * 16)(*[float(x) for x in c.pv_inv])
        cp = (C.c_float * 3)(*[float(x) for x in c.cam_pos])
        sc = lib.orc_scene_create_custom(color, pv, cp, sp, len(c.spectra), mt, len(c.materials), tx, len(c.textures), qs, len(c.quads))
        if sc:
            lib.orc_scene_set_camera_dir(sc, (C.c_float * 3)(*[float(x) for x in c.cam_dir]))
        return sc
    return ol.Oracle(observer=c.observer, custom=make, variant=VARIANT)
