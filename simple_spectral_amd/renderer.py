"""Host-side mirror of the reference's Renderer (src/renderer.hpp:14-82) over the C ABI.

    opts = Options(scene_name="cornell-srgb", res=(512, 512), spp=256)
    r = Renderer(opts)            # builds tables + scene on the host, uploads to the GPU
    r.render_start(); r.render_wait()
    r.framebuffer                 # sRGB+A float32 [H, W, 4], row 0 = bottom (src/framebuffer.hpp:26-34)
    r.xyza                        # the XYZ+alpha means the kernel produced (parity metric)

Everything numeric happens in libssx_hip.so / libssx_host.so; there is no Python or PyTorch
implementation of the integrator to fall back to.
"""
import ctypes as C
import os
from dataclasses import dataclass, field
from typing import Optional, Tuple

import numpy as np

from . import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT_DATA_DIR = os.path.join(ROOT, "data")


class SsxError(RuntimeError):
    def __init__(self, code, message):
        super().__init__("ssx error %d: %s" % (code, message))
        self.code = code


def _host(fn, *args):
    """libssx_host.so's `fn`(*args); SsxError with the library's reason unless it returns 0."""
    host = _capi.host_lib()
    rc = getattr(host, fn)(*args)
    if rc != 0:
        raise SsxError(rc, host.ssh_last_error().decode())


def _same_shape(what, names, ndim, arrays, dtypes):
    """The arrays, C-contiguous in their dtypes; ValueError "`what`: `names`" unless all of them have one shape of ndim dimensions."""
    arrays = [np.ascontiguousarray(a, dtype=t) for a, t in zip(arrays, dtypes)]
    if arrays[0].ndim != ndim or any(a.shape != arrays[0].shape for a in arrays):
        raise ValueError("%s: %s" % (what, names))
    return arrays


_F8, _U8 = np.float64, np.uint64
_PROBE_SUMS = ("SS, NN, VV, UU must all have shape [R, B]", 2)
_NOISE_TOTALS = ("EV, EM, PP, PU must all have shape [B]", 1)
_COMPARE_SUMS = ("DD, VV, X2, CC, NC, EX must all have shape [R, B]", 2)


@dataclass
class Options:
    """Renderer::Options (src/renderer.hpp:16-29) plus the additive options of this build."""
    scene_name: str = "cornell-srgb"
    res: Tuple[int, int] = (512, 512)
    spp: int = 16
    indirect_only: bool = False
    output_path: str = ""
    # additive (defaults = the reference's compile-time defaults)
    observer: int = 1931                 # CIE_OBSERVER
    seed: int = 0
    texture: Optional[str] = None        # PNG path; default per scene below
    light_scale: float = 30.0            # lightsc (src/scene.cpp:291-293)
    explicit_light_sampling: bool = True  # EXPLICIT_LIGHT_SAMPLING (src/stdafx.hpp:44); False also makes
    #                                       plane-srgb's textured quad a mirror (src/scene.cpp:346-355)
    flat_field_correction: bool = True   # FLAT_FIELD_CORRECTION (src/stdafx.hpp:55); False: flux = radiance * dot(ray dir, camera.dir)
    render_mode: str = "spectral"        # "spectral" (RENDER_MODE_SPECTRAL) | "rgb" (RENDER_MODE_RGB, src/stdafx.hpp:91-93:
    #                                       no spectra; `xyza` then holds linear RGB + alpha, `uplift`/`observer` are unused)
    uplift: str = "ours"                 # RENDER_MODE_SPECTRAL_ALGNUM: "ours" (1) | "meng" (2, Meng et al. 2015) | "jh" (3, Jakob-Hanika 2019)
    meng_grid_path: Optional[str] = None  # "SSXMENG1" file converted from the authors' header (simple_spectral_amd/meng.py)
    jh_res: int = 64                     # resolution of the fitted JH model when no coefficient file exists
    jh_coeff_path: Optional[str] = None  # data/jakob-and-hanika-2019-srgb.coeff in the reference (missing blob)
    jit_pass1: Optional[bool] = None     # ssx_set_jit: kernels compiled for the mesh topology of a scene that matches no built-in one (hipRTC).
    #                                       None: in the background, when the scene has rendered enough (the library's default);
    #                                       True: at upload, on the calling thread; False: never (generic kernel)
    device: int = 0
    tile_first: int = 0
    tile_stride: int = 1
    tile_skew: int = 0                   # ssx_render_params.tile_skew: rotate tile row ty of the shared-out list by ty * tile_skew columns (diagonal instead of vertical stripes)
    spp_per_launch: int = 0
    tile_major: bool = False             # ssx_render_params.tile_major: walk through the tiles like the reference (a stopped render keeps
    #                                       finished tiles at full sample count, the rest untouched) instead of through the samples
    libm: str = "build"                  # ssx_render_params.libm: "build" (include/ssx_fmath.h's sinf / cosf / acosf, the same on every
    #                                       platform) | "glibc-2.35" (glibc 2.35's x86-64 functions: the image of the reference as built on a stock
    #                                       x86-64 glibc 2.35 system)
    data_dir: str = field(default=DEFAULT_DATA_DIR)


def default_texture(data_dir):
    """The reference opens data/scenes/crystal-lizard-4096.png (src/scene.cpp:292,357), a blob
    missing from the repository; like the reference's own commented alternatives we fall back to
    the 512^2 version when it is absent."""
    for name in ("crystal-lizard-4096.png", "crystal-lizard-512.png", "test-img.png"):
        p = os.path.join(data_dir, "scenes", name)
        if os.path.exists(p):
            return p
    return None


class Scene:
    """Host-prepared scene + colour tables (libssx_host.so)."""

    def __init__(self, name, observer=1931, texture=None, light_scale=30.0, data_dir=DEFAULT_DATA_DIR,
                 uplift="ours", jh_res=64, jh_coeff_path=None, explicit_light_sampling=True, meng_grid_path=None, render_mode="spectral"):
        lib = _capi.host_lib()
        self._lib = lib
        self._h = C.c_void_p()
        tex_path = None
        self._tex = None
        if name != "cornell":
            if isinstance(texture, np.ndarray):
                self._tex = np.ascontiguousarray(texture, dtype=np.uint8)
            else:
                tex_path = texture or default_texture(data_dir)
                if tex_path and not tex_path.startswith("procedural:") and not os.path.isabs(tex_path) and not os.path.exists(tex_path):
                    tex_path = os.path.join(data_dir, "scenes", tex_path)
        tp, tw, th = (self._tex.ctypes.data, self._tex.shape[1], self._tex.shape[0]) if self._tex is not None else (None, 0, 0)
        if uplift not in ("ours", "meng", "jh"):
            raise SsxError(_capi.SSX_ERR_SCENE, "unsupported uplift %r (ours | meng | jh)" % (uplift,))
        if render_mode not in ("spectral", "rgb"):
            raise SsxError(_capi.SSX_ERR_SCENE, "unsupported render mode %r (spectral | rgb)" % (render_mode,))
        code = {"ours": _capi.SSX_UPLIFT_OURS, "meng": _capi.SSX_UPLIFT_MENG, "jh": _capi.SSX_UPLIFT_JH}[uplift]
        table_path = (meng_grid_path or os.path.join(data_dir, "meng-et-al-2015-grid.bin")) if uplift == "meng" else jh_coeff_path
        _host("ssh_scene_create_ex", name.encode(), data_dir.encode(), observer, tp, tw, th,
              tex_path.encode() if tex_path else None, C.c_float(light_scale),
              code | (0 if explicit_light_sampling else 0x100) | (0x200 if render_mode == "rgb" else 0),
              table_path.encode() if table_path else None, jh_res, C.byref(self._h))
        self.name = name

    @property
    def desc(self):
        return self._lib.ssh_scene_desc(self._h)

    def jh_model(self):
        """(res, scale[res], data[3*res^3*3]) of the Jakob-Hanika model in use, or None."""
        d = self.desc.contents
        if d.uplift != _capi.SSX_UPLIFT_JH:
            return None
        res = int(d.jh_res)
        return (res, np.ctypeslib.as_array(d.jh_scale, shape=(res,)).copy(),
                np.ctypeslib.as_array(d.jh_data, shape=(3 * res ** 3 * 3,)).copy())

    def xyza_to_srgba(self, xyza):
        xyza = np.ascontiguousarray(xyza, dtype=np.float32)
        out = np.empty_like(xyza)
        _host("ssh_xyza_to_srgba", self._h, xyza.ctypes.data, out.ctypes.data, xyza.size // 4)
        return out

    def color_values(self, name):
        buf = (C.c_float * 16)()
        n = self._lib.ssh_color_values(self._h, name.encode(), buf, 16)
        if n < 0:
            raise SsxError(n, "unknown colour table %r" % name)
        return np.array(buf[:n], dtype=np.float32)

    def close(self):
        if self._h:
            self._lib.ssh_scene_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def spectral_bin_index(lambda_0, lambda_min, lambda_step, bins):
    """The m of include/ssx.h's spectral output for first hero wavelengths lambda_0 (float32 array or scalar): component i of the sample falls
    into bin i * M + m, M = bins / 4.  t = (lambda_0 - lambda_min) / lambda_step and t * M in binary32, truncated, clamped to M - 1."""
    M = np.float32(bins // 4)
    t = (np.asarray(lambda_0, dtype=np.float32) - np.float32(lambda_min)) / np.float32(lambda_step)
    return np.minimum((t * M).astype(np.uint32), np.uint32(bins // 4 - 1))


PROBE_NO_REGION, PROBE_MAX_REGIONS = 255, 32   # include/ssx.h "Spectral moments and region probes"


def labels_from_rects(res, rects):
    """Labels for Renderer.probe: uint8 [H, W] (row 0 = bottom), region r = the half-open rectangle rects[r] = (x0, y0, x1, y1), PROBE_NO_REGION elsewhere;
    where two overlap the later one wins.  ValueError for an empty rectangle, one that leaves the image of res = (W, H), or more than 32."""
    W, H = res
    if not 1 <= len(rects) <= PROBE_MAX_REGIONS:
        raise ValueError("labels_from_rects: need 1..%d rectangles" % PROBE_MAX_REGIONS)
    labels = np.full((H, W), PROBE_NO_REGION, dtype=np.uint8)
    for r, (x0, y0, x1, y1) in enumerate(rects):
        if not (0 <= x0 < x1 <= W and 0 <= y0 < y1 <= H):
            raise ValueError("labels_from_rects: rectangle %d = %r is empty or leaves the %d x %d image" % (r, (x0, y0, x1, y1), W, H))
        labels[y0:y1, x0:x1] = r
    return labels


def labels_from_prim(prim, prims):
    """Labels for Renderer.probe from the guides' "prim" [H, W] (Renderer.guides): region r = the pixels whose first hit is primitive prims[r] (or any of
    prims[r], when that is a sequence -- a wall made of two primitives), PROBE_NO_REGION elsewhere."""
    prim = np.asarray(prim)
    if not 1 <= len(prims) <= PROBE_MAX_REGIONS:
        raise ValueError("labels_from_prim: need 1..%d regions" % PROBE_MAX_REGIONS)
    labels = np.full(prim.shape, PROBE_NO_REGION, dtype=np.uint8)
    for r, which in enumerate(prims):
        labels[np.isin(prim, np.atleast_1d(which))] = r
    return labels


def probe_derive(SS, NN, VV, UU):
    """ssh_probe_derive: (mean, stderr) float64 of the probes' four arrays -- mean = NN ? SS / NN : 0, stderr = sqrt(VV * NN / (NN - UU)) / NN (NaN when NN == UU)."""
    SS, NN, VV, UU = _same_shape("probe_derive", *_PROBE_SUMS, (SS, NN, VV, UU), (_F8, _U8, _F8, _U8))
    mean, err = np.zeros_like(SS), np.zeros_like(SS)
    _host("ssh_probe_derive", SS.shape[0], SS.shape[1], SS.ctypes.data, NN.ctypes.data, VV.ctypes.data, UU.ctypes.data, mean.ctypes.data, err.ctypes.data)
    return mean, err


def save_probe_csv(path, lambda_min, bin_width, SS, NN, VV, UU):
    """ssh_probe_save_csv (libssx_host.so), the writer the CLI's --probe-output uses: the line "region,bin,wavelength,mean,stderr,samples,unestimated", then one
    line per region and bin."""
    SS, NN, VV, UU = _same_shape("save_probe_csv", *_PROBE_SUMS, (SS, NN, VV, UU), (_F8, _U8, _F8, _U8))
    _host("ssh_probe_save_csv", os.fsencode(path), SS.shape[0], SS.shape[1], C.c_float(lambda_min), C.c_float(bin_width), SS.ctypes.data, NN.ctypes.data, VV.ctypes.data, UU.ctypes.data)


def spectral_noise_derive(EV, EM, PP, PU):
    """ssh_spectral_noise_derive: (noise, coverage, rel float64 [B]) of the spectral noise figure's totals (include/ssx.h "Spectral noise figure") -- noise =
    sqrt(sum EV / P) / (sum EM / P), coverage = P / (P + U), rel[b] = sqrt(EV[b] / PP[b]) / (EM[b] / PP[b]); NaN where nothing is estimable or a mean is 0."""
    EV, EM, PP, PU = _same_shape("spectral_noise_derive", *_NOISE_TOTALS, (EV, EM, PP, PU), (_F8, _F8, _U8, _U8))
    noise, coverage, rel = C.c_double(), C.c_double(), np.zeros_like(EV)
    _host("ssh_spectral_noise_derive", EV.shape[0], EV.ctypes.data, EM.ctypes.data, PP.ctypes.data, PU.ctypes.data, C.addressof(noise), C.addressof(coverage), rel.ctypes.data)
    return noise.value, coverage.value, rel


def save_spectral_noise_csv(path, lambda_min, bin_width, EV, EM, PP, PU):
    """ssh_spectral_noise_save_csv (libssx_host.so), the writer the CLI's --spectral-noise-output uses: the line "bin,wavelength,rel,EV,EM,estimable,unestimated",
    then one line per bin."""
    EV, EM, PP, PU = _same_shape("save_spectral_noise_csv", *_NOISE_TOTALS, (EV, EM, PP, PU), (_F8, _F8, _U8, _U8))
    _host("ssh_spectral_noise_save_csv", os.fsencode(path), EV.shape[0], C.c_float(lambda_min), C.c_float(bin_width), EV.ctypes.data, EM.ctypes.data, PP.ctypes.data, PU.ctypes.data)


COMPARE_FIGURES = ("mean_diff", "stderr", "z", "chi2", "exceed", "coverage")


def compare_derive(DD, VV, X2, CC, NC, EX):
    """ssh_compare_derive: a dict of float64 [R, B] arrays from the comparison's six sums (include/ssx.h "Comparing two spectral renders") -- mean_diff = DD / CC,
    stderr = sqrt(VV) / CC, z = DD / sqrt(VV), chi2 = X2 / CC, exceed = EX / CC, coverage = CC / (CC + NC); each NaN where its denominator is 0."""
    sums = _same_shape("compare_derive", *_COMPARE_SUMS, (DD, VV, X2, CC, NC, EX), (_F8,) * 3 + (_U8,) * 3)
    out = [np.zeros_like(sums[0]) for _ in COMPARE_FIGURES]
    _host("ssh_compare_derive", sums[0].shape[0], sums[0].shape[1], *[a.ctypes.data for a in sums], *[a.ctypes.data for a in out])
    return dict(zip(COMPARE_FIGURES, out))


def compare_zmap(diff, var):
    """The comparison's signed per-pixel map, float32: diff / sqrt(var), 0 where var is +inf (a cell that is not comparable)."""
    diff, var = np.asarray(diff, dtype=np.float32), np.asarray(var, dtype=np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(np.isposinf(var), np.float32(0.0), diff / np.sqrt(var)).astype(np.float32)


def save_compare_csv(path, lambda_min, bin_width, DD, VV, X2, CC, NC, EX):
    """ssh_compare_save_csv (libssx_host.so), the writer the CLI's --compare-output uses: the line
    "region,bin,wavelength,mean_diff,stderr,z,chi2,exceed,comparable,not_comparable", then one line per region and bin."""
    sums = _same_shape("save_compare_csv", *_COMPARE_SUMS, (DD, VV, X2, CC, NC, EX), (_F8,) * 3 + (_U8,) * 3)
    _host("ssh_compare_save_csv", os.fsencode(path), sums[0].shape[0], sums[0].shape[1], C.c_float(lambda_min), C.c_float(bin_width), *[a.ctypes.data for a in sums])


DELTA_E_FIGURES = ("mean", "rms", "max", "exceed", "coverage")
DELTA_E_THRESHOLDS = (2.3, 1.0)   # the customary just-noticeable differences of dE*ab and dE00: user parameters
_DELTA_E_SUMS = ("SUM, SSQ, MAX, NF, NX, EX must all have shape [R, 2]", 2)
_DELTA_E_TYPES = (np.float64, np.float64, np.float32, np.uint64, np.uint64, np.uint64)


def delta_e_derive(SUM, SSQ, MAX, NF, NX, EX):
    """ssh_delta_e_derive: a dict of float64 [R, 2] arrays (metric 0 dE*ab, 1 dE00) from the colour difference's six region arrays (include/ssx.h "Colour difference
    of two developments") -- mean = SUM / NF, rms = sqrt(SSQ / NF), max = MAX, exceed = EX / NF, coverage = NF / (NF + NX); each NaN where its denominator is 0."""
    sums = _same_shape("delta_e_derive", *_DELTA_E_SUMS, (SUM, SSQ, MAX, NF, NX, EX), _DELTA_E_TYPES)
    if sums[0].shape[1] != 2:
        raise ValueError("delta_e_derive: " + _DELTA_E_SUMS[0])
    out = [np.zeros(sums[0].shape, dtype=np.float64) for _ in DELTA_E_FIGURES]
    _host("ssh_delta_e_derive", sums[0].shape[0], *[a.ctypes.data for a in sums], *[a.ctypes.data for a in out])
    return dict(zip(DELTA_E_FIGURES, out))


def save_delta_e_csv(path, SUM, SSQ, MAX, NF, NX, EX):
    """ssh_delta_e_save_csv (libssx_host.so): the line "region,metric,mean,rms,max,exceed,coverage,finite,nonfinite", then one line per region and metric."""
    sums = _same_shape("save_delta_e_csv", *_DELTA_E_SUMS, (SUM, SSQ, MAX, NF, NX, EX), _DELTA_E_TYPES)
    if sums[0].shape[1] != 2:
        raise ValueError("save_delta_e_csv: " + _DELTA_E_SUMS[0])
    _host("ssh_delta_e_save_csv", os.fsencode(path), sums[0].shape[0], *[a.ctypes.data for a in sums])


def develop_white(weights, lambda_min, lambda_step, illuminant=None):
    """ssh_develop_white: the reference white float64 [3] that weights [3, B] (develop_weights, xyz space) give the illuminant (samples, low, high) -- the
    development of its mean over every bin; None: equal energy.  Which white a comparison uses, and at which scale, is a viewing decision like exposure: it sets
    the absolute size of every dE."""
    w = np.ascontiguousarray(weights, dtype=np.float32)
    if w.ndim != 2 or w.shape[0] != 3:
        raise ValueError("develop_white: weights must have shape [3, B]")
    spec, keep = (None, None) if illuminant is None else _spectrum_arg(illuminant)
    out = np.zeros(3, dtype=np.float64)
    _host("ssh_develop_white", w.ctypes.data, w.shape[1], C.c_float(lambda_min), C.c_float(lambda_step), None if spec is None else C.byref(spec), out.ctypes.data)
    return out


def compare_other(other):
    """What a comparison takes of another render: `other` is what load_checkpoint_file_moments returns (nine values), or (SsxSpectralInfo, S, N, Q) -> (SsxSpectralInfo,
    S float64 [H, W, B], Q float64 [H, W, B], N uint32 [H, W, B / 4]).  ValueError when it carries no bins or no second moments."""
    info, S, N, Q = other[5:9] if len(other) == 9 else other
    if not info.bins or S is None or N is None or Q is None:
        raise ValueError("compare: the other render carries no wavelength bins with their second moments (a checkpoint written with the moments on has them)")
    S, Q, N = np.ascontiguousarray(S, dtype=np.float64), np.ascontiguousarray(Q, dtype=np.float64), np.ascontiguousarray(N, dtype=np.uint32)
    shape = (info.height, info.width, info.bins)
    if S.shape != shape or Q.shape != shape or N.shape != shape[:2] + (info.bins // 4,):
        raise ValueError("compare: the other render's S and Q must have shape [H, W, B] = %r of its info, N [H, W, B / 4]" % (shape,))
    return info, S, Q, N


def save_npy(path, array):
    """ssh_save_npy_f32 (libssx_host.so): `array` as a float32 .npy file, the writer the CLI's --spectral-output uses."""
    a = np.ascontiguousarray(array, dtype=np.float32)
    shape = (C.c_uint32 * a.ndim)(*a.shape)
    _host("ssh_save_npy_f32", os.fsencode(path), a.ctypes.data, shape, a.ndim)


def _spectrum_arg(spec):
    """(samples, low, high) -> (SshSpectrum, the array that keeps its samples alive)"""
    samples, low, high = spec
    a = np.ascontiguousarray(samples, dtype=np.float32)
    if a.ndim != 1 or a.size < 2:
        raise ValueError("a spectrum is (samples [n >= 2], low, high)")
    return _capi.SshSpectrum(a.ctypes.data_as(C.POINTER(C.c_float)), a.size, float(low), float(high)), a


def load_spectrum_csv(path):
    """A file in the format of data/*.csv -> (samples float32 [n], low, high) of its first column; the range is in the name: NAME-LOW+STEP+HIGH.csv."""
    import re
    m = re.search(r"-([0-9.]+)\+([0-9.]+)\+([0-9.]+)\.csv$", os.path.basename(path))
    if not m:
        raise ValueError("%r: a spectrum file names its range, NAME-LOW+STEP+HIGH.csv" % (path,))
    low, step, high = (float(x) for x in m.groups())
    rows = [ln.replace(",", " ").split() for ln in open(path) if ln.strip()]
    samples = np.array([float(r[0]) for r in rows], dtype=np.float32)
    if samples.size != (high - low) / step + 1:
        raise ValueError("%r: %d rows do not match the range in the file's name" % (path, samples.size))
    return samples, low, high


def develop_weights(bins, lambda_min, lambda_step, observer=1931, responses=None, filter=None, gain=None, space="xyz", data_dir=DEFAULT_DATA_DIR, return_float64=False):
    """ssh_develop_weights (include/ssx.h "Developing the spectral bins"): the float32 [C, bins] matrix that Renderer.develop / develop_images apply to bins of
    a render with this lambda_min and lambda_step (Scene.desc.contents).  responses: a list of (samples, low, high) response curves, or None for the x-bar,
    y-bar, z-bar of `observer` (1931 | 2006); filter: an optional (samples, low, high) spectrum in front of the lens; gain: an optional float64 [bins] factor
    per bin (relight_gain); space: "xyz" or "lrgb" (three rows taken to linear BT.709 with `observer`'s matrix).  Integrated exactly in binary64 and rounded
    once; with return_float64: (float32, float64 before the rounding)."""
    if space not in ("xyz", "lrgb"):
        raise ValueError("develop_weights: space must be 'xyz' or 'lrgb'")
    keep, resp, n_ch = [], None, 3
    if responses is not None:
        n_ch = len(responses)
        resp = (_capi.SshSpectrum * max(1, n_ch))()
        for k, spec in enumerate(responses):
            resp[k], a = _spectrum_arg(spec)
            keep.append(a)
    flt = None
    if filter is not None:
        flt, a = _spectrum_arg(filter)
        keep.append(a)
    g = None if gain is None else np.ascontiguousarray(gain, dtype=np.float64)
    if g is not None and g.shape != (bins,):
        raise ValueError("develop_weights: gain must have shape [bins]")
    w = np.zeros((n_ch, bins), dtype=np.float32)
    w64 = np.zeros((n_ch, bins), dtype=np.float64)
    _host("ssh_develop_weights", os.fsencode(data_dir), int(observer), resp, n_ch, None if flt is None else C.byref(flt), None if g is None else g.ctypes.data,
          _capi.SSH_SPACE_LRGB if space == "lrgb" else _capi.SSH_SPACE_XYZ, int(bins), C.c_float(lambda_min), C.c_float(lambda_step), w.ctypes.data, w64.ctypes.data)
    return (w, w64) if return_float64 else w


def relight_gain(old, new, bins, lambda_min, lambda_step):
    """ssh_relight_gain: float64 [bins], the integral of `new` over each bin divided by that of `old` (both (samples, low, high)), 0 where the latter is 0.  Passed
    as develop_weights' gain it turns a render lit by `old` into one lit by `new` -- exactly only when every emitter of the scene carries `old` up to a scale."""
    a, ka = _spectrum_arg(old)
    b, kb = _spectrum_arg(new)
    g = np.zeros(bins, dtype=np.float64)
    _host("ssh_relight_gain", C.byref(a), C.byref(b), int(bins), C.c_float(lambda_min), C.c_float(lambda_step), g.ctypes.data)
    return g


def lens_optics(bins, lambda_min, lambda_step, lateral=0.0, sigma=0.0, axial=0.0, lambda_ref=550.0, max_radius=8, centre=None):
    """ssh_optics_lens (include/ssx_host.h): the lens Renderer.develop(..., optics=) and Renderer.optics_images put in front of the bins of a render with this
    lambda_min and lambda_step, as a dict {cx, cy, max_radius, scale [B], radius [B], taps [B, 2 R + 1]} -- what include/ssx.h's ssx_optics_params carries; any
    dict of that form is a lens.  lateral: the magnification's relative change per relative wavelength offset from lambda_ref (lateral chromatic aberration);
    sigma: the blur's standard deviation in pixels at lambda_ref, growing in proportion to the wavelength; axial: pixels of defocus blur per relative wavelength
    offset.  centre (cx, cy) in pixel units; None: the middle of whatever image the lens is applied to."""
    R = int(max_radius)
    scale, radius, taps = np.zeros(bins, dtype=np.float32), np.zeros(bins, dtype=np.uint32), np.zeros((bins, 2 * max(R, 0) + 1), dtype=np.float32)
    _host("ssh_optics_lens", int(bins), C.c_float(lambda_min), C.c_float(lambda_step), float(lambda_ref), float(lateral), float(sigma), float(axial), R,
          scale.ctypes.data, radius.ctypes.data, taps.ctypes.data)
    cx, cy = (None, None) if centre is None else centre
    return {"cx": cx, "cy": cy, "max_radius": R, "scale": scale, "radius": radius, "taps": taps}


def _optics_arg(optics, W, H):
    """A lens dict (lens_optics) -> (SsxOpticsParams, the arrays that keep its tables alive).  The tables' shapes are the caller's business as far as the library
    can check them itself; here only what would make it read past an array."""
    R = int(optics["max_radius"])
    scale = np.ascontiguousarray(optics["scale"], dtype=np.float32)
    radius = np.ascontiguousarray(optics["radius"], dtype=np.uint32)
    taps = np.ascontiguousarray(optics["taps"], dtype=np.float32)
    B = scale.size
    if scale.ndim != 1 or radius.shape != (B,) or (0 <= R <= _capi.SSX_OPTICS_MAX_RADIUS and taps.size != B * (2 * R + 1)):
        raise ValueError("optics: scale and radius must have shape [B], taps [B, 2 * max_radius + 1]")
    p = _capi.SsxOpticsParams()
    p.struct_size = C.sizeof(_capi.SsxOpticsParams)
    p.cx = W / 2.0 if optics.get("cx") is None else float(optics["cx"])
    p.cy = H / 2.0 if optics.get("cy") is None else float(optics["cy"])
    p.max_radius = R & 0xFFFFFFFF
    p.scale, p.radius, p.taps = scale.ctypes.data, radius.ctypes.data, taps.ctypes.data
    return p, (scale, radius, taps)


def thin_lens_defocus(scene, height, bins, aperture, focus_distance, axial=0.0, lambda_ref=550.0, max_radius=8):
    """ssh_defocus_thin_lens (include/ssx_host.h): the aperture Renderer.develop(..., defocus=) and Renderer.defocus_images put in front of the bins of a render
    of `scene` (a Scene) with `height` rows, as a dict {max_radius, gain, focus [B]} -- what include/ssx.h's ssx_defocus_params carries; any dict of that form
    is an aperture.  aperture: the lens's diameter and focus_distance: the distance in focus at lambda_ref, both in scene units; axial: the shift of the
    inverse focus distance per unit of relative wavelength offset (longitudinal chromatic aberration); max_radius: the largest circle of confusion in pixels.
    The depth is a ray length: the surface in focus is a sphere about the eye."""
    vfov, gain, focus = C.c_float(), C.c_float(), np.zeros(bins, dtype=np.float32)
    _host("ssh_scene_vfov", scene._h, C.byref(vfov))
    d = scene.desc.contents
    _host("ssh_defocus_thin_lens", vfov, int(height), int(bins), C.c_float(d.lambda_min), C.c_float(d.lambda_step), float(aperture), float(focus_distance), float(axial),
          float(lambda_ref), C.byref(gain), focus.ctypes.data)
    return {"max_radius": int(max_radius), "gain": float(gain.value), "focus": focus}


def _defocus_arg(defocus):
    """An aperture dict (thin_lens_defocus) -> (SsxDefocusParams, the array that keeps its table alive)."""
    focus = np.ascontiguousarray(defocus["focus"], dtype=np.float32)
    if focus.ndim != 1:
        raise ValueError("defocus: focus must have shape [B]")
    p = _capi.SsxDefocusParams()
    p.struct_size = C.sizeof(_capi.SsxDefocusParams)
    p.max_radius = int(defocus["max_radius"]) & 0xFFFFFFFF
    p.gain = float(defocus["gain"])
    p.focus = focus.ctypes.data
    return p, (focus,)


def glare_plan(width, height, radius):
    """ssh_glare_plan: (px, py), the padded extents ssx_glare_params needs for an image of width x height and a psf of this radius."""
    px, py = C.c_uint32(), C.c_uint32()
    _host("ssh_glare_plan", int(width), int(height), int(radius), C.byref(px), C.byref(py))
    return px.value, py.value


def glare_twiddles(P):
    """ssh_glare_twiddles: the forward twiddles T[m] = (cos, -sin)(2 pi m / P) as float32 [P / 2, 2]."""
    t = np.zeros((max(int(P) // 2, 1), 2), dtype=np.float32)
    _host("ssh_glare_twiddles", int(P), t.ctypes.data)
    return t


def glare_aperture(bins, lambda_min, lambda_step, width, height, blades=6, ring_px=1.5, strength=0.1, rotation=0.0, lambda_ref=550.0, radius=64):
    """ssh_glare_aperture, ssh_glare_plan and ssh_glare_twiddles (include/ssx_host.h): the glare Renderer.develop(..., glare=) and Renderer.glare_images put behind
    the lens for bins of a render with this lambda_min and lambda_step and an image of width x height, as a dict {radius, px, py, on [B], psf [B, K, K],
    twiddle_x [px / 2, 2], twiddle_y [py / 2, 2]} -- what include/ssx.h's ssx_glare_params carries; any dict of that form is a glare.  blades: the iris's
    straight blades (fewer than 3: a disc); ring_px: where a disc's first dark ring lies at lambda_ref, in pixels; strength: the share of the light that leaves
    the geometric image; rotation in radians."""
    R = int(radius)
    K = 2 * max(R, 0) + 1
    psf, on = np.zeros((bins, K, K), dtype=np.float32), np.zeros(bins, dtype=np.uint8)
    _host("ssh_glare_aperture", int(bins), C.c_float(lambda_min), C.c_float(lambda_step), float(lambda_ref), int(blades), float(rotation), float(ring_px), float(strength),
          R, psf.ctypes.data, on.ctypes.data)
    px, py = glare_plan(width, height, R)
    return {"radius": R, "px": px, "py": py, "on": on, "psf": psf, "twiddle_x": glare_twiddles(px), "twiddle_y": glare_twiddles(py)}


def _glare_arg(glare):
    """A glare dict (glare_aperture) -> (SsxGlareParams, the arrays that keep its tables alive).  Here only what would make the library read past an array."""
    R, px, py = int(glare["radius"]), int(glare["px"]), int(glare["py"])
    on = np.ascontiguousarray(glare["on"], dtype=np.uint8)
    psf = np.ascontiguousarray(glare["psf"], dtype=np.float32)
    tx = np.ascontiguousarray(glare["twiddle_x"], dtype=np.float32)
    ty = np.ascontiguousarray(glare["twiddle_y"], dtype=np.float32)
    if on.ndim != 1 or (0 <= R <= _capi.SSX_GLARE_MAX_RADIUS and psf.size != on.size * (2 * R + 1) ** 2):
        raise ValueError("glare: on must have shape [B], psf [B, 2 * radius + 1, 2 * radius + 1]")
    if (0 < px <= _capi.SSX_GLARE_MAX_EXTENT and tx.size != px) or (0 < py <= _capi.SSX_GLARE_MAX_EXTENT and ty.size != py):
        raise ValueError("glare: twiddle_x must have shape [px / 2, 2], twiddle_y [py / 2, 2]")
    p = _capi.SsxGlareParams()
    p.struct_size = C.sizeof(_capi.SsxGlareParams)
    p.radius, p.px, p.py = R & 0xFFFFFFFF, px & 0xFFFFFFFF, py & 0xFFFFFFFF
    p.on, p.psf, p.twiddle_x, p.twiddle_y = on.ctypes.data, psf.ctypes.data, tx.ctypes.data, ty.ctypes.data
    return p, (on, psf, tx, ty)


def sensor_bayer(pattern, method="mhc"):
    """ssh_sensor_bayer (include/ssx_host.h): {"cfa": uint32 [4], "taps": float32 [4, 3, 25]} for a Bayer pattern "RGGB", "BGGR", "GRBG" or "GBRG" -- the first
    two letters are row 0, THE BOTTOM ROW -- and the demosaic `method`, "mhc" (Malvar-He-Cutler) or "bilinear".  Merged with sensor_exposure's dict, "weights"
    (develop_weights(responses=) of the camera's three curves) and "ccm" (sensor_ccm) it is a sensor for Renderer.develop(sensor=)."""
    if method not in ("mhc", "bilinear"):
        raise ValueError("sensor_bayer: method must be 'mhc' or 'bilinear'")
    cfa, taps = np.zeros(4, dtype=np.uint32), np.zeros((4, 3, 25), dtype=np.float32)
    _host("ssh_sensor_bayer", str(pattern).encode(), _capi.SSH_DEMOSAIC_MHC if method == "mhc" else _capi.SSH_DEMOSAIC_BILINEAR, cfa.ctypes.data, taps.ctypes.data)
    return {"cfa": cfa, "taps": taps}


_SENSOR_SCALES = ("exposure", "inv_exposure", "read_var", "dn_per_e", "e_per_dn", "black", "white")


def sensor_exposure(full_well, white_level, bits=0, black=0.0, read_e=0.0):
    """ssh_sensor_exposure: the scales of a sensor whose well of `full_well` electrons is filled by a development of `white_level`, read with `read_e` electrons
    of noise through an ADC of `bits` bits above `black` (bits 0: no ADC), as a dict {exposure, inv_exposure, read_var, dn_per_e, e_per_dn, black, white}."""
    out = np.zeros(7, dtype=np.float32)
    _host("ssh_sensor_exposure", float(full_well), float(white_level), int(bits), float(black), float(read_e), out.ctypes.data)
    return {k: float(v) for k, v in zip(_SENSOR_SCALES, out)}


def sensor_ccm(cam, target):
    """ssh_sensor_ccm: float32 [3, 3], the least-squares matrix target * cam^T * (cam * cam^T)^-1 that takes a camera's channels (cam [3, B], its weights) to a
    target's (target [3, B], e.g. develop_weights(space="lrgb")); SsxError where the camera's curves are linearly dependent over the bins."""
    cam, target = np.ascontiguousarray(cam, dtype=np.float32), np.ascontiguousarray(target, dtype=np.float32)
    if cam.ndim != 2 or cam.shape[0] != 3 or target.shape != cam.shape:
        raise ValueError("sensor_ccm: cam and target must have shape [3, B]")
    ccm = np.zeros((3, 3), dtype=np.float32)
    _host("ssh_sensor_ccm", cam.ctypes.data, target.ctypes.data, cam.shape[1], ccm.ctypes.data)
    return ccm


def sensor_standin_curves():
    """ssh_sensor_standin_curve: the three stand-in response curves [(samples, low, high)] x 3 the CLI's --develop-sensor uses when no curves are given -- Gaussians
    peaking at 600, 540 and 460 nm with a standard deviation of 35 nm.  THEY ARE NO CAMERA'S.  For develop_weights(responses=)."""
    out = []
    for ch in range(3):
        s, low, high = np.zeros(71, dtype=np.float32), C.c_float(), C.c_float()
        _host("ssh_sensor_standin_curve", ch, s.ctypes.data, C.byref(low), C.byref(high))
        out.append((s, float(low.value), float(high.value)))
    return out


def tone_curve_len(lo, hi, shift):
    """curve_len of ssx_tone_params (include/ssx.h): ((bits(hi) - bits(lo)) >> shift) + 2."""
    b = np.array([lo, hi], dtype=np.float32).view(np.uint32)
    return ((int(b[1]) - int(b[0])) >> int(shift)) + 2


def meter_derive(hist, special, key=0.18, white_percentile=0.99, percentiles=()):
    """ssh_meter_derive (include/ssx_host.h): what a metering (Renderer.meter_images) says -- {"log_average", "exposure" (puts the log-average on `key`), "white" (the
    luminance's white_percentile, a key's lower edge), "white_exposed", "pivot" (L of `key`, for LOCAL), "grey" and "patch" (float32 [3]: grey-world and white-patch
    channel gains), "count", "percentiles" (float32 [4, len(percentiles)]: the channels' and the luminance's)}."""
    hist = np.ascontiguousarray(hist, dtype=np.uint32)
    special = np.ascontiguousarray(special, dtype=np.uint32)
    if hist.shape != (4, _capi.SSX_METER_KEYS) or special.shape != (4, 4):
        raise ValueError("meter_derive: hist must have shape [4, 4096], special [4, 4]")
    pc = np.ascontiguousarray(percentiles, dtype=np.float64).reshape(-1)
    po = np.zeros((4, pc.size), dtype=np.float32)
    out = np.zeros(_capi.SSH_METER_OUT, dtype=np.float32)
    _host("ssh_meter_derive", hist.ctypes.data, special.ctypes.data, float(key), float(white_percentile), pc.ctypes.data if pc.size else None, pc.size,
          po.ctypes.data if pc.size else None, out.ctypes.data)
    return {"log_average": out[_capi.SSH_METER_LOG_AVERAGE], "exposure": out[_capi.SSH_METER_EXPOSURE], "white": out[_capi.SSH_METER_WHITE],
            "white_exposed": out[_capi.SSH_METER_WHITE_EXPOSED], "pivot": out[_capi.SSH_METER_PIVOT], "grey": out[_capi.SSH_METER_GREY:_capi.SSH_METER_GREY + 3].copy(),
            "patch": out[_capi.SSH_METER_PATCH:_capi.SSH_METER_PATCH + 3].copy(), "count": out[_capi.SSH_METER_COUNT], "percentiles": po}


TONE_CURVES = {"clip": _capi.SSH_TONE_CLIP, "reinhard": _capi.SSH_TONE_REINHARD, "filmic": _capi.SSH_TONE_FILMIC}


def tone_curve(kind, lo, hi, shift, white=1.0):
    """ssh_tone_curve: float32 [tone_curve_len(lo, hi, shift)], the tone curve `kind` ("clip", "reinhard" with its white point, "filmic") composed with the sRGB
    transfer function, one entry per node of ssx_tone_params' table."""
    if kind not in TONE_CURVES:
        raise ValueError("tone_curve: kind must be one of %s" % ", ".join(sorted(TONE_CURVES)))
    n = tone_curve_len(lo, hi, shift)
    out = np.zeros(max(n, 0), dtype=np.float32)
    _host("ssh_tone_curve", TONE_CURVES[kind], float(white), float(lo), float(hi), int(shift), out.ctypes.data, n & 0xFFFFFFFF)
    return out


def display_matrix(observer=1931, data_dir=DEFAULT_DATA_DIR):
    """ssh_display_matrix: float32 [3, 3], XYZ -> linear sRGB: ssx_tone_params.matrix for a development in CIE XYZ."""
    out = np.zeros((3, 3), dtype=np.float32)
    _host("ssh_display_matrix", data_dir.encode(), int(observer), out.ctypes.data)
    return out


DISPLAY_LO, DISPLAY_HI, DISPLAY_SHIFT = 2.0 ** -12, 16.0, 19   # the finish's own table: sixteen nodes per octave over sixteen octaves, 258 entries
DISPLAY_Y_LO, DISPLAY_Y_HI = 2.0 ** -20, 2.0 ** 20             # LOCAL's range of exposed luminance
DISPLAY_LOCAL_EPS = 0.25                                       # (half an octave)^2


def display_luma(matrix):
    """float32 [3]: the BT.709 luminance of what `matrix` [3, 3] makes of an image's channels, (0.2126 row 0 + 0.7152 row 1) + 0.0722 row 2 in binary64, rounded once -- for the
    project's XYZ -> linear sRGB that is Y up to its radiometric scale, so that a metered exposure lands where the display sees it."""
    m = np.asarray(matrix, dtype=np.float64).reshape(3, 3)
    return ((0.2126 * m[0] + 0.7152 * m[1]) + 0.0722 * m[2]).astype(np.float32)


def _display_arg(display, observer=1931, data_dir=DEFAULT_DATA_DIR):
    """A display dict with its defaults filled in: "curve" ("reinhard"), "key" (0.18), "white_percentile" (0.99), "wb" ("none", "grey" or "white-patch"), "local" (None, or
    {"radius", "compress", "boost" (1), "eps" (0.25)}), "space" ("xyz": the matrix is display_matrix; "lrgb": the identity),
    "matrix" and "luma" (override the space's matrix and display_luma(matrix)), "lo", "hi", "shift" (the table: 2^-12, 16, 19), "mask" (uint8 [H, W]: what is metered)."""
    d = dict(display)
    unknown = set(d) - {"curve", "key", "white_percentile", "wb", "local", "space", "matrix", "luma", "lo", "hi", "shift", "mask"}
    if unknown:
        raise ValueError("display: unknown entries %s" % ", ".join(sorted(unknown)))
    d.setdefault("curve", "reinhard"); d.setdefault("key", 0.18); d.setdefault("white_percentile", 0.99); d.setdefault("wb", "none"); d.setdefault("local", None)
    d.setdefault("space", "xyz"); d.setdefault("lo", DISPLAY_LO); d.setdefault("hi", DISPLAY_HI); d.setdefault("shift", DISPLAY_SHIFT); d.setdefault("mask", None)
    if d["curve"] not in TONE_CURVES:
        raise ValueError("display: curve must be one of %s" % ", ".join(sorted(TONE_CURVES)))
    if d["wb"] not in ("none", "grey", "white-patch"):
        raise ValueError("display: wb must be 'none', 'grey' or 'white-patch'")
    if d["space"] not in ("xyz", "lrgb"):
        raise ValueError("display: space must be 'xyz' or 'lrgb'")
    if d.get("matrix") is None:
        d["matrix"] = display_matrix(observer, data_dir) if d["space"] == "xyz" else np.eye(3, dtype=np.float32)
    if d.get("luma") is None:
        d["luma"] = display_luma(d["matrix"])
    if d["local"] is not None:
        loc = dict(d["local"])
        if "radius" not in loc or "compress" not in loc:
            raise ValueError("display: local needs radius and compress")
        loc.setdefault("boost", 1.0); loc.setdefault("eps", DISPLAY_LOCAL_EPS)
        d["local"] = loc
    return d


def _sensor_arg(sensor):
    """A sensor dict -> (SsxSensorParams, the arrays that keep its tables alive: weights, taps, ccm, each None where the dict has none).  cfa is required; the
    scales default to a sensor that counts in the units of the develop (exposure 1, no noise, no ADC)."""
    p = _capi.SsxSensorParams()
    p.struct_size = C.sizeof(_capi.SsxSensorParams)
    cfa = [int(v) & 0xFFFFFFFF for v in sensor["cfa"]]
    if len(cfa) != 4:
        raise ValueError("sensor: cfa must hold four entries")
    p.cfa = (C.c_uint32 * 4)(*cfa)
    p.noise, p.seed, p.frame = int(bool(sensor.get("noise", 0))), int(sensor.get("seed", 0)) & 0xFFFFFFFF, int(sensor.get("frame", 0)) & 0xFFFFFFFF
    for k, default in zip(_SENSOR_SCALES, (1.0, 1.0, 0.0, 1.0, 1.0, 0.0, 0.0)):
        setattr(p, k, float(sensor.get(k, default)))
    keep = []
    for k, shape in (("weights", None), ("taps", (4, 3, 25)), ("ccm", (3, 3))):
        a = sensor.get(k)
        if a is not None:
            a = np.ascontiguousarray(a, dtype=np.float32)
            if (shape is not None and a.shape != shape) or (shape is None and (a.ndim != 2 or a.shape[0] != 3)):
                raise ValueError("sensor: %s must have shape %s" % (k, "[3, B]" if shape is None else list(shape)))
            setattr(p, k, a.ctypes.data)
        keep.append(a)
    return p, tuple(keep)


def emitter_spectrum(desc):
    """ssh_emitter_spectrum: the index (in desc.spectra) of the emission spectrum all emissive materials share up to a scale; SsxError SSX_ERR_SCENE otherwise."""
    idx = C.c_uint32()
    _host("ssh_emitter_spectrum", desc if hasattr(desc, "contents") else C.byref(desc), C.byref(idx))
    return idx.value


def _load_checkpoint(fn, path, extra):
    """The one body of the three loaders below: libssx_host.so's `fn` with the out-pointers of the pixel sums and of `extra` (0, 2 or 3) of bins, counts and Q."""
    host = _capi.host_lib()
    info, sinfo = _capi.SsxSumsInfo(), _capi.SsxSpectralInfo()
    name, text = C.create_string_buffer(256), C.create_string_buffer(4096)
    ptrs = [C.POINTER(t)() for t in (C.c_double, C.c_double, C.c_double, C.c_uint32, C.c_double)[:2 + extra]]
    tail = [C.byref(sinfo)] + [C.byref(p) for p in ptrs[2:]] if extra else []
    _host(fn, os.fsencode(path), C.byref(info), name, len(name), text, len(text), C.byref(ptrs[0]), C.byref(ptrs[1]), *tail)
    try:
        H, W, B = info.height, info.width, sinfo.bins
        shapes = ((H, W, 4), (H, W), (H, W, B), (H, W, B // 4), (H, W, B))
        arrays = [np.ctypeslib.as_array(p, shape=s).copy() if p else None for p, s in zip(ptrs, shapes)]
    finally:
        for p in ptrs:
            if p:
                host.ssh_free(p)
    return (info, arrays[0], arrays[1], name.value.decode(), text.value.decode()) + ((sinfo,) + tuple(arrays[2:]) if extra else ())


def load_checkpoint_file(path):
    """ssh_checkpoint_load -> (SsxSumsInfo, sums [H, W, 4], S2 [H, W] or None, scene name, options text)."""
    return _load_checkpoint("ssh_checkpoint_load", path, 0)


def load_checkpoint_file_spectral(path):
    """ssh_checkpoint_load_spectral -> load_checkpoint_file's five values and (SsxSpectralInfo, sums float64 [H, W, B], counts uint32 [H, W, B / 4]) of the
    wavelength bins; from a checkpoint without them (magic SSXCKPT1) the info's bins is 0 and both arrays are None."""
    return _load_checkpoint("ssh_checkpoint_load_spectral", path, 2)


def load_checkpoint_file_moments(path):
    """ssh_checkpoint_load_moments -> load_checkpoint_file_spectral's eight values and Q float64 [H, W, B], the bins' second moments; None from a checkpoint
    without them (magic SSXCKPT1 or SSXCKPT2)."""
    return _load_checkpoint("ssh_checkpoint_load_moments", path, 3)


def merge_moments(dst_q, src_q, src_info):
    """ssh_moments_merge: merge_sums' rule for the bins' second moments -- Q float64 [H, W, B] of the pixels src_info's exporter owns (an SsxSumsInfo: export_sums'
    of the same context), bit for bit."""
    assert dst_q.dtype == np.float64 and dst_q.flags.c_contiguous and src_q.dtype == np.float64 and src_q.flags.c_contiguous and dst_q.shape == src_q.shape
    _host("ssh_moments_merge", dst_q.ctypes.data, src_q.ctypes.data, src_q.shape[2], C.byref(src_info))


def merge_spectral(dst_sums, dst_counts, src_sums, src_counts, src_info):
    """ssh_spectral_merge: merge_sums' rule for the wavelength bins -- sums float64 [H, W, B] and counts uint32 [H, W, B / 4] of the pixels src_info's exporter
    owns (an SsxSumsInfo: export_sums' of the same context), bit for bit."""
    assert dst_sums.dtype == np.float64 and dst_sums.flags.c_contiguous and src_sums.dtype == np.float64 and src_sums.flags.c_contiguous
    assert dst_counts.dtype == np.uint32 and dst_counts.flags.c_contiguous and src_counts.dtype == np.uint32 and src_counts.flags.c_contiguous
    assert dst_sums.shape == src_sums.shape and dst_counts.shape == src_counts.shape and src_sums.shape[2] == 4 * src_counts.shape[2]
    _host("ssh_spectral_merge", dst_sums.ctypes.data, dst_counts.ctypes.data, src_sums.ctypes.data, src_counts.ctypes.data, src_sums.shape[2], C.byref(src_info))


def merge_sums(dst, dst_s2, src, src_s2, src_info):
    """ssh_sums_merge: dst's pixels that src_info's exporter owns <- src's, bit for bit (by ownership mask, not by adding)."""
    assert dst.dtype == np.float64 and dst.flags.c_contiguous and src.dtype == np.float64 and src.flags.c_contiguous
    _host("ssh_sums_merge", dst.ctypes.data, None if dst_s2 is None or src_s2 is None else dst_s2.ctypes.data, src.ctypes.data,
          None if dst_s2 is None or src_s2 is None else src_s2.ctypes.data, C.byref(src_info))


class Renderer:
    """Renderer (src/renderer.hpp:14-82): render_start / render_stop / render_wait / is_rendering,
    public `framebuffer` and `scene`."""

    def __init__(self, options: Options):
        self.options = options
        self.scene = Scene(options.scene_name, options.observer, options.texture, options.light_scale, options.data_dir,
                           options.uplift, options.jh_res, options.jh_coeff_path, options.explicit_light_sampling, options.meng_grid_path, options.render_mode)
        self._lib = _capi.hip_lib()
        self._ctx = C.c_void_p()
        rc = self._lib.ssx_create(options.device, C.byref(self._ctx))
        if rc != 0:
            raise SsxError(rc, self._lib.ssx_last_error(None).decode())
        if options.jit_pass1 is not None:
            self._check(self._lib.ssx_set_jit(self._ctx, _capi.SSX_JIT_AT_UPLOAD if options.jit_pass1 else _capi.SSX_JIT_OFF))
        self._check(self._lib.ssx_upload_scene(self._ctx, self.scene.desc))
        W, H = options.res
        self.xyza = np.zeros((H, W, 4), dtype=np.float32)
        self.framebuffer = np.zeros((H, W, 4), dtype=np.float32)
        self._spectral_bins, self._spectral_moments = 0, False   # what set_spectral_bins / set_spectral_moments last set

    def _check(self, rc):
        if rc != 0:
            raise SsxError(rc, self._lib.ssx_last_error(self._ctx).decode())

    def params(self, **over):
        o = self.options
        p = _capi.SsxRenderParams()
        p.struct_size = C.sizeof(_capi.SsxRenderParams)
        p.width, p.height = o.res
        p.spp = o.spp
        p.indirect_only = int(o.indirect_only)
        p.no_explicit_light_sampling = int(not o.explicit_light_sampling)
        p.no_flat_field_correction = int(not o.flat_field_correction)
        p.tile_first, p.tile_stride = o.tile_first, o.tile_stride
        p.tile_skew = o.tile_skew
        p.spp_per_launch = o.spp_per_launch
        p.tile_major = int(o.tile_major)
        p.seed = o.seed
        if o.libm not in _capi.LIBM_MODES:
            raise ValueError("Options.libm: %r is not one of %s" % (o.libm, ", ".join(sorted(_capi.LIBM_MODES))))
        p.libm = _capi.LIBM_MODES[o.libm]
        for k, v in over.items():
            setattr(p, k, v)
        return p

    def render_start(self):
        self._check(self._lib.ssx_render_start(self._ctx, C.byref(self.params())))

    def render_stop(self):
        self._check(self._lib.ssx_render_stop(self._ctx))

    def is_rendering(self):
        return bool(self._lib.ssx_is_rendering(self._ctx))

    def progress(self):
        return float(self._lib.ssx_progress(self._ctx))

    def done_spp(self):
        """Samples per pixel accumulated so far (after render_stop: what the partial image is the mean of)."""
        return int(self._lib.ssx_done_spp(self._ctx))

    def done_tiles(self):
        """ssx_done_tiles: this device's tiles (ascending tile order) finished so far."""
        return int(self._lib.ssx_done_tiles(self._ctx))

    def render_wait(self):
        self._check(self._lib.ssx_render_wait(self._ctx, self.xyza.ctypes.data))
        self.framebuffer = self.scene.xyza_to_srgba(self.xyza)  # src/renderer.cpp:298
        if self.options.output_path:
            self.save(self.options.output_path)
        return self.framebuffer

    # ---- progressive rendering (include/ssx.h: continue, checkpoint / resume, noise estimate) ----

    def render_continue(self, spp):
        """ssx_render_continue: `spp` more samples per pixel onto the existing sums (asynchronous: then render_wait).  The image is
        bit for bit the one a single render of done_spp() + spp samples gives."""
        self._check(self._lib.ssx_render_continue(self._ctx, int(spp)))

    def read_framebuffer(self):
        """The image the context holds (after load_checkpoint / import_sums: the checkpointed one) -> self.xyza, self.framebuffer."""
        self._check(self._lib.ssx_read_framebuffer(self._ctx, self.xyza.ctypes.data))
        self.framebuffer = self.scene.xyza_to_srgba(self.xyza)
        return self.framebuffer

    def scene_digest(self):
        return int(self._lib.ssx_scene_digest(self._ctx))

    def set_noise_estimate(self, enable=True):
        self._check(self._lib.ssx_set_noise_estimate(self._ctx, int(bool(enable))))

    def export_sums(self):
        """ssx_sums_export -> (SsxSumsInfo, sums float64 [H, W, 4], S2 float64 [H, W] or None when the noise estimate holds nothing)."""
        W, H = self.options.res
        info = _capi.SsxSumsInfo()
        sums = np.zeros((H, W, 4), dtype=np.float64)
        s2 = np.zeros((H, W), dtype=np.float64)
        self._check(self._lib.ssx_sums_export(self._ctx, C.byref(info), sums.ctypes.data, s2.ctypes.data))
        return info, sums, (s2 if info.noise_batches else None)

    def import_sums(self, info, sums, s2=None, **over):
        """ssx_sums_import: the context keeps the tiles it owns under its own options (tile_first / tile_stride / tile_skew) and is
        continuable at info.done_spp; self.xyza is the checkpointed image."""
        sums = np.ascontiguousarray(sums, dtype=np.float64)
        s2 = None if s2 is None else np.ascontiguousarray(s2, dtype=np.float64)
        if sums.size != info.width * info.height * 4 or (s2 is not None and s2.size != info.width * info.height):
            raise ValueError("import_sums: sums must have shape [info.height, info.width, 4], S2 [info.height, info.width]")
        p = self.params(**over)
        self._check(self._lib.ssx_sums_import(self._ctx, C.byref(p), C.byref(info), sums.ctypes.data, None if s2 is None else s2.ctypes.data))
        self.read_framebuffer()

    def holds_spectral(self):
        """Whether the context holds valid wavelength bins of exactly the samples behind its sums (what export_spectral and save_checkpoint need)."""
        if not self._spectral_bins:
            return False
        return self._lib.ssx_spectral_read(self._ctx, C.byref(_capi.SsxSpectralInfo()), None, None, None) == 0

    def export_spectral(self):
        """ssx_spectral_read's raw state -> (SsxSpectralInfo, sums float64 [H, W, B], counts uint32 [H, W, B / 4]): what import_spectral takes back and a
        checkpoint keeps; zeros for pixels the context does not own (merge_spectral combines the ranks')."""
        info, _, counts, sums = self.spectral_read(sums=True)
        return info, sums, counts

    def import_spectral(self, info, sums, counts):
        """ssx_spectral_import, directly on top of import_sums: the context takes the bins of the tiles it owns from the whole-image arrays and then stands where a
        render of info.done_spp samples with spectral output would have left it -- render_continue carries the bins on; spectral_read, denoise_spectral and
        develop work from them.  SsxError with the library's reason when they do not belong to the imported sums."""
        sums = np.ascontiguousarray(sums, dtype=np.float64)
        counts = np.ascontiguousarray(counts, dtype=np.uint32)
        if sums.size != info.width * info.height * info.bins or counts.size * 4 != sums.size:
            raise ValueError("import_spectral: sums must have shape [info.height, info.width, info.bins], counts [info.height, info.width, info.bins / 4]")
        self._check(self._lib.ssx_spectral_import(self._ctx, C.byref(info), sums.ctypes.data, counts.ctypes.data))

    def holds_moments(self):
        """Whether the context holds valid second moments of exactly the samples behind its bins (what export_moments needs, and save_checkpoint to keep them)."""
        if not self._spectral_bins:
            return False
        return self._lib.ssx_spectral_variance(self._ctx, C.byref(_capi.SsxSpectralInfo()), None, None) == 0

    def export_moments(self):
        """ssx_spectral_variance's raw state -> (SsxSpectralInfo, Q float64 [H, W, B]): what import_moments takes back and a checkpoint keeps; zeros for pixels the
        context does not own (merge_moments combines the ranks')."""
        info, _, q = self.spectral_variance(q=True)
        return info, q

    def import_moments(self, info, q):
        """ssx_spectral_moments_import, directly on top of import_spectral (set_spectral_moments before or after the two imports): the context takes the second
        moments of the tiles it owns from the whole-image array and then stands where a render of info.done_spp samples with the moments on would have left it --
        render_continue carries Q on; spectral_variance, probe and spectral_noise work.  SsxError with the library's reason -- the field, or the rule of the
        consistency check -- when they do not belong to the imported bins; the moments are invalid then, bins and sums untouched."""
        q = np.ascontiguousarray(q, dtype=np.float64)
        if q.size != info.width * info.height * info.bins:
            raise ValueError("import_moments: q must have shape [info.height, info.width, info.bins]")
        self._check(self._lib.ssx_spectral_moments_import(self._ctx, C.byref(info), q.ctypes.data))

    def save_checkpoint(self, path):
        """The sums (and the noise estimate's S2) into one file (libssx_host.so ssh_checkpoint_save_moments; host/checkpoint.hpp has the format); with them
        the wavelength bins when the context holds valid ones, and behind those their second moments when it holds valid ones -- otherwise the file is the one it
        always was."""
        info, sums, s2 = self.export_sums()
        sinfo, bins, counts = self.export_spectral() if self.holds_spectral() else (None, None, None)
        q = self.export_moments()[1] if sinfo is not None and self.holds_moments() else None
        o = self.options
        text = "observer=%d\ntexture=%s\nlight_scale=%r\nuplift=%s\nrender_mode=%s\nexplicit_light_sampling=%d\n" % (
            o.observer, o.texture if isinstance(o.texture, str) else "", o.light_scale, o.uplift, o.render_mode, int(o.explicit_light_sampling))
        _host("ssh_checkpoint_save_moments", os.fsencode(path), C.byref(info), o.scene_name.encode(), text.encode(), sums.ctypes.data, None if s2 is None else s2.ctypes.data,
              None if sinfo is None else C.byref(sinfo), None if bins is None else bins.ctypes.data,
              None if counts is None else counts.ctypes.data, None if q is None else q.ctypes.data)

    def load_checkpoint(self, path):
        """Reads a checkpoint and imports it (SsxError SSX_ERR_DATA for a damaged file, SSX_ERR_ARG with the library's reason for one
        of another scene, size, seed or set of flags).  Returns its SsxSumsInfo.  A file with wavelength bins, read while set_spectral_bins(its count) is in
        force: the bins are taken up too (import_spectral); self.spectral_resumed says whether.  A file with their second moments, read with
        set_spectral_moments(True) in force and the bins taken up: Q is taken up too (import_moments); self.moments_resumed says whether."""
        info, sums, s2, _, _, sinfo, bins, counts, q = load_checkpoint_file_moments(path)
        self.import_sums(info, sums, s2)
        self.spectral_resumed = bool(sinfo.bins) and sinfo.bins == self._spectral_bins
        self.moments_resumed = self.spectral_resumed and q is not None and self._spectral_moments
        if self.spectral_resumed:
            self.import_spectral(sinfo, bins, counts)
        if self.moments_resumed:
            self.import_moments(sinfo, q)
        return info

    def noise(self):
        """ssx_noise_info -> (noise, v_map): noise = sqrt(sum v / n) / (sum A/N / n), the RMS standard error of the pixel means relative to
        the mean luminance; v_map float64 [H, W], the variance of each pixel's mean.  self.noise_summary keeps {sum v, sum A/N, n, B}."""
        W, H = self.options.res
        v = np.zeros((H, W), dtype=np.float64)
        s = (C.c_double * 4)()
        self._check(self._lib.ssx_noise_info(self._ctx, v.ctypes.data, s))
        self.noise_summary = [float(x) for x in s]
        return float(np.sqrt(s[0] / s[2]) / (s[1] / s[2])), v

    def render_until(self, target, step, max_spp):
        """Renders `step` samples per pixel at a time (one launch = one batch of the estimate) until noise() <= target -- checked after every
        step from the second on -- or done_spp() >= max_spp.  Returns (done_spp, noise).  Deterministic: the decision reads only the sums."""
        if step < 1 or max_spp < 1:
            raise ValueError("render_until: step and max_spp must be positive")
        self.set_noise_estimate(True)
        self._check(self._lib.ssx_render_start(self._ctx, C.byref(self.params(spp=int(step), spp_per_launch=int(step)))))
        self.render_wait()
        level = float("inf")
        while self.done_spp() < max_spp:
            self.render_continue(step)
            self.render_wait()
            level, _ = self.noise()
            if level <= target:
                break
        return self.done_spp(), level

    # ---- spectral radiance output (include/ssx.h: per-pixel wavelength bins) ----

    def set_spectral_bins(self, n):
        """ssx_set_spectral_bins: n wavelength bins per pixel (a multiple of 4 up to 64) for the renders that follow; 0 switches it off."""
        self._check(self._lib.ssx_set_spectral_bins(self._ctx, int(n)))
        self._spectral_bins = int(n)
        if not n:
            self._spectral_moments = False   # (the library switches the moments off with the bins)

    def spectral_read(self, sums=False):
        """ssx_spectral_read -> (SsxSpectralInfo, mean float32 [H, W, B], counts uint32 [H, W, B/4], sums float64 [H, W, B] or None)."""
        info = _capi.SsxSpectralInfo()
        self._check(self._lib.ssx_spectral_read(self._ctx, C.byref(info), None, None, None))
        H, W, B = info.height, info.width, info.bins
        mean = np.zeros((H, W, B), dtype=np.float32)
        counts = np.zeros((H, W, B // 4), dtype=np.uint32)
        s = np.zeros((H, W, B), dtype=np.float64) if sums else None
        self._check(self._lib.ssx_spectral_read(self._ctx, C.byref(info), mean.ctypes.data, None if s is None else s.ctypes.data, counts.ctypes.data))
        return info, mean, counts, s

    def spectral_image(self):
        """(mean [H, W, B] float32, counts [H, W, B/4] uint32, centres [B] float32) of the last render: mean[j, i, b] is the mean flux of the samples of
        pixel (i, j) (row 0 = bottom) whose wavelength fell into bin b, centres[b] = lambda_min + (b + 0.5) * bin_width the bin's middle wavelength."""
        info, mean, counts, _ = self.spectral_read()
        centres = np.float32(info.lambda_min) + (np.arange(info.bins, dtype=np.float32) + np.float32(0.5)) * np.float32(info.bin_width)
        return mean, counts, centres.astype(np.float32)

    # ---- error bars for the bins (include/ssx.h: second moments, variances, region probes) ----

    def set_spectral_moments(self, enable=True):
        """ssx_set_spectral_moments: keep the second moments of the hero fluxes beside the bins, for the renders that follow (after set_spectral_bins)."""
        self._check(self._lib.ssx_set_spectral_moments(self._ctx, int(bool(enable))))
        self._spectral_moments = bool(enable)

    def spectral_variance(self, q=False):
        """ssx_spectral_variance -> (SsxSpectralInfo, var float32 [H, W, B], Q float64 [H, W, B] or None): the variance of every bin mean (+inf where a sub-bin holds
        fewer than two samples; 0 for pixels the context does not own) and the raw second moments."""
        info = _capi.SsxSpectralInfo()
        self._check(self._lib.ssx_spectral_variance(self._ctx, C.byref(info), None, None))
        H, W, B = info.height, info.width, info.bins
        var = np.zeros((H, W, B), dtype=np.float32)
        Q = np.zeros((H, W, B), dtype=np.float64) if q else None
        self._check(self._lib.ssx_spectral_variance(self._ctx, C.byref(info), var.ctypes.data, None if Q is None else Q.ctypes.data))
        return info, var, Q

    @staticmethod
    def _regions(labels, shape, regions):
        """(labels uint8 of `shape`, R): `regions`, or for None the largest label + 1"""
        labels = np.ascontiguousarray(labels, dtype=np.uint8)
        if labels.shape != shape:
            raise ValueError("probe: labels must have shape [H, W] = %r" % (shape,))
        if regions is not None:
            return labels, int(regions)
        named = labels[labels != PROBE_NO_REGION]
        return labels, (int(named.max()) + 1 if named.size else 1)

    def probe_raw(self, labels, regions=None):
        """ssx_spectral_probe -> (SS float64, NN uint64, VV float64, UU uint64), each [R, B]: the four sums of include/ssx.h over the pixels of every region of
        labels (uint8 [H, W], row 0 = bottom: 0..R-1 a region, 255 none; labels_from_rects, labels_from_prim).  regions None: the largest label + 1."""
        W, H = self.options.res
        labels, R = self._regions(labels, (H, W), regions)
        B = self._spectral_bins or 4
        SS, VV = np.zeros((R, B), dtype=np.float64), np.zeros((R, B), dtype=np.float64)
        NN, UU = np.zeros((R, B), dtype=np.uint64), np.zeros((R, B), dtype=np.uint64)
        self._check(self._lib.ssx_spectral_probe(self._ctx, labels.ctypes.data, R, SS.ctypes.data, NN.ctypes.data, VV.ctypes.data, UU.ctypes.data))
        return SS, NN, VV, UU

    def probe(self, labels, regions=None):
        """The pooled spectrum of every region of labels with its error bar -> (mean float64 [R, B], stderr float64 [R, B], samples uint64 [R, B], unestimated
        uint64 [R, B]): the mean weights samples, not pixels; stderr is NaN where no sub-bin of the region holds two samples."""
        SS, NN, VV, UU = self.probe_raw(labels, regions)
        mean, err = probe_derive(SS, NN, VV, UU)
        return mean, err, NN, UU

    def probe_arrays(self, sums, q, counts, labels, regions=None):
        """ssx_probe_arrays: probe_raw as a pure function of row-major arrays -- sums and q float64 [H, W, B], counts uint32 [H, W, B / 4] (e.g. several contexts'
        exports merged by ownership) -> (SS, NN, VV, UU)."""
        sums, q = np.ascontiguousarray(sums, dtype=np.float64), np.ascontiguousarray(q, dtype=np.float64)
        counts = np.ascontiguousarray(counts, dtype=np.uint32)
        if sums.ndim != 3 or q.shape != sums.shape or counts.shape != sums.shape[:2] + (sums.shape[2] // 4,) or sums.shape[2] % 4:
            raise ValueError("probe_arrays: sums and q must have shape [H, W, B], counts [H, W, B / 4]")
        H, W, B = sums.shape
        labels, R = self._regions(labels, (H, W), regions)
        SS, VV = np.zeros((R, B), dtype=np.float64), np.zeros((R, B), dtype=np.float64)
        NN, UU = np.zeros((R, B), dtype=np.uint64), np.zeros((R, B), dtype=np.uint64)
        self._check(self._lib.ssx_probe_arrays(self._ctx, W, H, B, sums.ctypes.data, q.ctypes.data, counts.ctypes.data, labels.ctypes.data, R,
                                               SS.ctypes.data, NN.ctypes.data, VV.ctypes.data, UU.ctypes.data))
        return SS, NN, VV, UU

    # ---- comparing two spectral renders (include/ssx.h "Comparing two spectral renders") ----

    @staticmethod
    def _compare_outputs(R, shape, maps):
        sums = [np.zeros((R, shape[2]), dtype=np.float64) for _ in range(3)] + [np.zeros((R, shape[2]), dtype=np.uint64) for _ in range(3)]
        diff, var = (np.zeros(shape, dtype=np.float32), np.zeros(shape, dtype=np.float32)) if maps else (None, None)
        return sums, diff, var

    def compare_spectral_raw(self, other, labels, regions=None, threshold=3.0, maps=True):
        """ssx_spectral_compare: this context's render (A) against another (B) -> ((DD float64, VV float64, X2 float64, CC uint64, NC uint64, EX uint64), each [R, B],
        diff float32 [H, W, B], var float32 [H, W, B]); the maps are None with maps=False.  other: what load_checkpoint_file_moments returns, or (SsxSpectralInfo, S,
        N, Q); labels as probe_raw takes them; threshold: the z beyond which a comparable cell counts into EX (the library takes its square)."""
        info, S, Q, N = compare_other(other)
        W, H = self.options.res
        labels, R = self._regions(labels, (H, W), regions)
        B = self._spectral_bins or 4
        sums, diff, var = self._compare_outputs(R, (H, W, B), maps)
        self._check(self._lib.ssx_spectral_compare(self._ctx, C.byref(info), S.ctypes.data, Q.ctypes.data, N.ctypes.data, labels.ctypes.data, R, float(threshold) * float(threshold),
                                                   *[a.ctypes.data for a in sums], None if diff is None else diff.ctypes.data, None if var is None else var.ctypes.data))
        return tuple(sums), diff, var

    def compare_spectral(self, other, labels, regions=None, threshold=3.0):
        """The comparison's derived figures -> a dict of float64 [R, B] arrays mean_diff, stderr, z, chi2, exceed, coverage (compare_derive), with "comparable" and
        "not_comparable" (uint64 [R, B]) and "zmap" (float32 [H, W, B]: diff / sqrt(var), 0 where a cell is not comparable).  The two renders must have independent
        samples (different seeds); with few samples per sub-bin chi2 is to be held against nu / (nu - 2), not 1."""
        sums, diff, var = self.compare_spectral_raw(other, labels, regions, threshold)
        out = compare_derive(*sums)
        out.update(comparable=sums[3], not_comparable=sums[4], zmap=compare_zmap(diff, var))
        return out

    def compare_arrays(self, SA, QA, NA, SB, QB, NB, labels, regions=None, threshold=3.0, maps=True, t2=None):
        """ssx_spectral_compare_arrays: compare_spectral_raw as a pure function of two row-major array sets -- S and Q float64 [H, W, B], N uint32 [H, W, B / 4] each
        (e.g. two checkpoints', or several contexts' exports merged by ownership).  t2, when given, is passed as it is instead of threshold squared."""
        SA, QA, SB, QB = (np.ascontiguousarray(a, dtype=np.float64) for a in (SA, QA, SB, QB))
        NA, NB = np.ascontiguousarray(NA, dtype=np.uint32), np.ascontiguousarray(NB, dtype=np.uint32)
        if SA.ndim != 3 or SA.shape[2] % 4 or not (QA.shape == SB.shape == QB.shape == SA.shape) or not (NA.shape == NB.shape == SA.shape[:2] + (SA.shape[2] // 4,)):
            raise ValueError("compare_arrays: S and Q of both sets must have shape [H, W, B], N [H, W, B / 4]")
        H, W, B = SA.shape
        labels, R = self._regions(labels, (H, W), regions)
        sums, diff, var = self._compare_outputs(R, (H, W, B), maps)
        self._check(self._lib.ssx_spectral_compare_arrays(self._ctx, W, H, B, SA.ctypes.data, QA.ctypes.data, NA.ctypes.data, SB.ctypes.data, QB.ctypes.data, NB.ctypes.data,
                                                          labels.ctypes.data, R, float(threshold) * float(threshold) if t2 is None else float(t2),
                                                          *[a.ctypes.data for a in sums], None if diff is None else diff.ctypes.data, None if var is None else var.ctypes.data))
        return tuple(sums), diff, var

    # ---- the colour difference of two developments (include/ssx.h "Colour difference of two developments") ----

    def _delta_e_args(self, what, shape, white_a, white_b, labels, regions, thresholds, maps, lab):
        H, W = shape
        wa, wb = np.ascontiguousarray(white_a, dtype=np.float64), np.ascontiguousarray(white_b, dtype=np.float64)
        t = np.ascontiguousarray(thresholds, dtype=np.float64)
        if wa.shape != (3,) or wb.shape != (3,) or t.shape != (2,):
            raise ValueError("%s: the whites must have shape [3], the thresholds [2]" % what)
        if labels is None:
            R = 1 if regions is None else int(regions)
        else:
            labels, R = self._regions(labels, (H, W), regions)
        sums = [np.zeros((R, 2), dtype=d) for d in _DELTA_E_TYPES]
        de = np.zeros((H, W, 2), dtype=np.float32) if maps else None
        lab6 = np.zeros((H, W, 6), dtype=np.float32) if lab else None
        ptr = lambda a: None if a is None else a.ctypes.data
        return (wa, wb, labels, t, sums, de, lab6), [wa.ctypes.data, wb.ctypes.data, ptr(labels), R, t.ctypes.data, ptr(de), ptr(lab6)] + [a.ctypes.data for a in sums]

    def delta_e_images(self, xyz_a, xyz_b, white_a, white_b, labels=None, regions=None, thresholds=DELTA_E_THRESHOLDS, maps=True, lab=False):
        """ssx_delta_e_images: two XYZ images float32 [H, W, 3] (develop with xyz weights) under their whites float64 [3] -> ((SUM float64, SSQ float64, MAX float32,
        NF uint64, NX uint64, EX uint64), each [R, 2] -- metric 0 dE*ab, 1 dE00 --, de float32 [H, W, 2] or None with maps=False, lab float32 [H, W, 6] or None).
        labels as probe_raw takes them, None: the whole image is region 0.  thresholds: (ab, 00), what EX counts the pixels beyond."""
        xa, xb = np.ascontiguousarray(xyz_a, dtype=np.float32), np.ascontiguousarray(xyz_b, dtype=np.float32)
        if xa.ndim != 3 or xa.shape[2] != 3 or xb.shape != xa.shape:
            raise ValueError("delta_e_images: xyz_a and xyz_b must have one shape [H, W, 3]")
        keep, args = self._delta_e_args("delta_e_images", xa.shape[:2], white_a, white_b, labels, regions, thresholds, maps, lab)
        self._check(self._lib.ssx_delta_e_images(self._ctx, xa.shape[1], xa.shape[0], xa.ctypes.data, xb.ctypes.data, *args))
        return tuple(keep[4]), keep[5], keep[6]

    def delta_e_raw(self, weights_a, weights_b, white_a, white_b, labels=None, regions=None, thresholds=DELTA_E_THRESHOLDS, denoise=None, denoised=(False, False),
                    maps=True, lab=False):
        """ssx_spectral_delta_e: the bins the context holds developed twice on the device, by weights_a and weights_b [3, B], side x raw or -- denoised[x] -- filtered
        with `denoise`'s parameters (a dict as Renderer.develop takes it), and compared where they lie -> delta_e_images' result, the same bits.  Nothing the
        context holds changes."""
        W, H = self.options.res
        wa, wb = np.ascontiguousarray(weights_a, dtype=np.float32), np.ascontiguousarray(weights_b, dtype=np.float32)
        if wa.ndim != 2 or wa.shape[0] != 3 or wb.shape != wa.shape:
            raise ValueError("delta_e: weights_a and weights_b must have one shape [3, B]")
        if self._spectral_bins not in (0, wa.shape[1]):
            raise ValueError("delta_e: weights for %d bins, the context holds %d" % (wa.shape[1], self._spectral_bins))
        p = None if denoise is None else self._denoise_params(denoise.get("levels", 5), denoise.get("sigma_l", 1.0), denoise.get("sigma_a", 0.1))
        keep, args = self._delta_e_args("delta_e", (H, W), white_a, white_b, labels, regions, thresholds, maps, lab)
        self._check(self._lib.ssx_spectral_delta_e(self._ctx, None if p is None else C.byref(p), int(bool(denoised[0])), int(bool(denoised[1])),
                                                   wa.ctypes.data, wb.ctypes.data, *args))
        return tuple(keep[4]), keep[5], keep[6]

    def delta_e(self, weights_a, weights_b, white_a, white_b, labels=None, regions=None, thresholds=DELTA_E_THRESHOLDS, denoise=None, denoised=(False, False)):
        """The colour difference's derived figures -> a dict of float64 [R, 2] arrays mean, rms, max, exceed, coverage (delta_e_derive), with "finite" and
        "nonfinite" (uint64 [R, 2]) and "map" (float32 [H, W, 2]: dE*ab, dE00)."""
        sums, de, _ = self.delta_e_raw(weights_a, weights_b, white_a, white_b, labels, regions, thresholds, denoise, denoised)
        out = delta_e_derive(*sums)
        out.update(finite=sums[3], nonfinite=sums[4], map=de)
        return out

    # ---- the spectral noise figure and the render loop that stops on it (include/ssx.h "Spectral noise figure") ----

    def _noise_mask(self, mask):
        if mask is None:
            return None
        W, H = self.options.res
        mask = np.asarray(mask)
        mask = np.ascontiguousarray(mask if mask.dtype == np.uint8 else mask != 0, dtype=np.uint8)   # (uint8 goes to the library as it is: any nonzero value is in)
        if mask.shape != (H, W):
            raise ValueError("spectral_noise: mask must have shape [H, W] = %r" % ((H, W),))
        return mask

    def spectral_noise_raw(self, mask=None):
        """ssx_spectral_noise -> ((EV float64, EM float64, PP uint64, PU uint64), each [B], (tEV float64, tEM float64, tPP uint32, tPU uint32), each [tiles, B]):
        the totals and the per-tile partials (tile t = ty * tiles_x + tx; +0.0 and 0 for tiles the context does not own).  mask: [H, W] (row 0 = bottom, nonzero =
        in) or None for every pixel."""
        W, H = self.options.res
        mask = self._noise_mask(mask)
        B = self._spectral_bins or 4
        tiles = ((W + 7) // 8) * ((H + 7) // 8)
        EV, EM, PP, PU = np.zeros(B), np.zeros(B), np.zeros(B, dtype=np.uint64), np.zeros(B, dtype=np.uint64)
        tEV, tEM = np.zeros((tiles, B)), np.zeros((tiles, B))
        tPP, tPU = np.zeros((tiles, B), dtype=np.uint32), np.zeros((tiles, B), dtype=np.uint32)
        self._check(self._lib.ssx_spectral_noise(self._ctx, None if mask is None else mask.ctypes.data, EV.ctypes.data, EM.ctypes.data, PP.ctypes.data, PU.ctypes.data,
                                                 tEV.ctypes.data, tEM.ctypes.data, tPP.ctypes.data, tPU.ctypes.data))
        return (EV, EM, PP, PU), (tEV, tEM, tPP, tPU)

    def spectral_noise(self, mask=None):
        """The spectral noise figure -> (noise, coverage, (EV, EM, PP, PU)): noise is the RMS standard error of the pixels' bin means relative to the mean bin
        flux, over the sub-bins that hold two samples; coverage is their share.  NaN when nothing is estimable, or with a non-finite flux."""
        totals, _ = self.spectral_noise_raw(mask)
        noise, coverage, _ = spectral_noise_derive(*totals)
        return noise, coverage, totals

    def spectral_noise_reduce(self, tEV, tEM, tPP, tPU):
        """ssx_spectral_noise_reduce: the totals of uploaded tile partials [tiles, B] (e.g. several contexts' partials merged by ownership) -> (EV, EM, PP, PU)."""
        tEV, tEM, tPP, tPU = _same_shape("spectral_noise_reduce", "the four partials must all have shape [tiles, B]", 2, (tEV, tEM, tPP, tPU), (_F8, _F8, np.uint32, np.uint32))
        tiles, B = tEV.shape
        EV, EM, PP, PU = np.zeros(B), np.zeros(B), np.zeros(B, dtype=np.uint64), np.zeros(B, dtype=np.uint64)
        self._check(self._lib.ssx_spectral_noise_reduce(self._ctx, tiles, B, tEV.ctypes.data, tEM.ctypes.data, tPP.ctypes.data, tPU.ctypes.data,
                                                        EV.ctypes.data, EM.ctypes.data, PP.ctypes.data, PU.ctypes.data))
        return EV, EM, PP, PU

    def render_until_spectral(self, target, step, max_spp, mask=None, min_coverage=0.99, resume=False):
        """Renders `step` samples per pixel at a time, with the moments on (set_spectral_bins first), until spectral_noise(mask) gives noise <= target and coverage
        >= min_coverage -- checked after EVERY step, the first included -- or done_spp() >= max_spp.  Returns (done_spp, noise, coverage).  min_coverage is the
        user's parameter, not a tolerance: it keeps a render with many bins from stopping on the few sub-bins that hold two samples after one step; 1.0 is legal
        but slow to reach (two samples in every sub-bin of every pixel).  A NaN figure never stops the render.  Deterministic: the decision reads only S, Q, N.
        resume=True: the render goes on from what the context holds (a load_checkpoint that took the moments up, or an earlier run of this loop) instead of
        starting over -- no ssx_render_start; valid moments are required (SsxError SSX_ERR_STATE otherwise); the figure is read FIRST, so a resumed render that
        already meets the target renders nothing; then `step` at a time as above."""
        if step < 1 or max_spp < 1:
            raise ValueError("render_until_spectral: step and max_spp must be positive")
        mask = self._noise_mask(mask)
        if resume:
            while True:
                noise, coverage, _ = self.spectral_noise(mask)
                if (noise <= target and coverage >= min_coverage) or self.done_spp() >= max_spp:
                    return self.done_spp(), noise, coverage
                self.render_continue(step)
                self.render_wait()
        self.set_spectral_moments(True)
        self._check(self._lib.ssx_render_start(self._ctx, C.byref(self.params(spp=int(step), spp_per_launch=int(step)))))
        while True:
            self.render_wait()
            noise, coverage, _ = self.spectral_noise(mask)
            if (noise <= target and coverage >= min_coverage) or self.done_spp() >= max_spp:
                return self.done_spp(), noise, coverage
            self.render_continue(step)

    # ---- denoising (include/ssx.h: guide buffers and the variance-guided a-trous filter) ----

    def guides(self, res=None):
        """ssx_guides -> {"prim": uint32 [H, W] (0xFFFFFFFF: miss), "depth": float32 [H, W], "normal": float32 [H, W, 3], "albedo": float32 [H, W, 4]}:
        the first hit of the ray through each pixel centre (row 0 = bottom), at the options' resolution or `res` = (W, H)."""
        W, H = res if res is not None else self.options.res
        g = {"prim": np.zeros((H, W), dtype=np.uint32), "depth": np.zeros((H, W), dtype=np.float32),
             "normal": np.zeros((H, W, 3), dtype=np.float32), "albedo": np.zeros((H, W, 4), dtype=np.float32)}
        self._check(self._lib.ssx_guides(self._ctx, W, H, g["prim"].ctypes.data, g["depth"].ctypes.data, g["normal"].ctypes.data, g["albedo"].ctypes.data))
        return g

    @staticmethod
    def _denoise_params(levels, sigma_l, sigma_a):
        p = _capi.SsxDenoiseParams()
        p.struct_size = C.sizeof(_capi.SsxDenoiseParams)
        p.levels, p.sigma_l, p.sigma_a = int(levels), float(sigma_l), float(sigma_a)
        return p

    def denoise(self, levels=5, sigma_l=1.0, sigma_a=0.1, return_variance=False):
        """ssx_denoise: the image the context holds, filtered on the device with the noise estimate's variance and the scene's guide buffers -> xyza
        float32 [H, W, 4] (with return_variance: and the filtered variance float32 [H, W]).  Needs set_noise_estimate(True) before the render, at least
        two launches (batches) and the whole image on this device; nothing the context holds changes."""
        W, H = self.options.res
        out = np.zeros((H, W, 4), dtype=np.float32)
        var = np.zeros((H, W), dtype=np.float32) if return_variance else None
        p = self._denoise_params(levels, sigma_l, sigma_a)
        self._check(self._lib.ssx_denoise(self._ctx, C.byref(p), out.ctypes.data, None if var is None else var.ctypes.data))
        return (out, var) if return_variance else out

    def denoise_images(self, xyza, var, prim, albedo, levels=5, sigma_l=1.0, sigma_a=0.1, return_variance=False):
        """ssx_denoise_images: the same filter as a pure function of its arguments: xyza [H, W, 4], var [H, W] (image units), prim [H, W] uint32,
        albedo [H, W, 4]."""
        xyza = np.ascontiguousarray(xyza, dtype=np.float32)
        if xyza.ndim != 3 or xyza.shape[2] != 4:
            raise ValueError("denoise_images: xyza must have shape [H, W, 4]")
        H, W = xyza.shape[:2]
        var = np.ascontiguousarray(var, dtype=np.float32)
        prim = np.ascontiguousarray(prim, dtype=np.uint32)
        albedo = np.ascontiguousarray(albedo, dtype=np.float32)
        if var.shape != (H, W) or prim.shape != (H, W) or albedo.shape != (H, W, 4):
            raise ValueError("denoise_images: var and prim must have shape [H, W], albedo [H, W, 4]")
        out = np.zeros((H, W, 4), dtype=np.float32)
        vout = np.zeros((H, W), dtype=np.float32) if return_variance else None
        p = self._denoise_params(levels, sigma_l, sigma_a)
        self._check(self._lib.ssx_denoise_images(self._ctx, C.byref(p), W, H, xyza.ctypes.data, var.ctypes.data, prim.ctypes.data, albedo.ctypes.data,
                                                 out.ctypes.data, None if vout is None else vout.ctypes.data))
        return (out, vout) if return_variance else out

    def denoise_channels(self, xyza, var, prim, albedo, extra, levels=5, sigma_l=1.0, sigma_a=0.1, return_image=False):
        """ssx_denoise_channels: the filter of denoise_images applied, with the weights it computes from xyza, var, prim and albedo, to `extra` [H, W, E]
        (1 <= E <= 80) -> float32 [H, W, E]; with return_image: (extra, xyza, var), the last two those of denoise_images."""
        xyza = np.ascontiguousarray(xyza, dtype=np.float32)
        if xyza.ndim != 3 or xyza.shape[2] != 4:
            raise ValueError("denoise_channels: xyza must have shape [H, W, 4]")
        H, W = xyza.shape[:2]
        var = np.ascontiguousarray(var, dtype=np.float32)
        prim = np.ascontiguousarray(prim, dtype=np.uint32)
        albedo = np.ascontiguousarray(albedo, dtype=np.float32)
        extra = np.ascontiguousarray(extra, dtype=np.float32)
        if var.shape != (H, W) or prim.shape != (H, W) or albedo.shape != (H, W, 4) or extra.ndim != 3 or extra.shape[:2] != (H, W):
            raise ValueError("denoise_channels: var and prim must have shape [H, W], albedo [H, W, 4], extra [H, W, E]")
        E = extra.shape[2]
        eout = np.zeros((H, W, E), dtype=np.float32)
        out = np.zeros((H, W, 4), dtype=np.float32) if return_image else None
        vout = np.zeros((H, W), dtype=np.float32) if return_image else None
        p = self._denoise_params(levels, sigma_l, sigma_a)
        self._check(self._lib.ssx_denoise_channels(self._ctx, C.byref(p), W, H, xyza.ctypes.data, var.ctypes.data, prim.ctypes.data, albedo.ctypes.data, E,
                                                   extra.ctypes.data, None if out is None else out.ctypes.data,
                                                   None if vout is None else vout.ctypes.data, eout.ctypes.data))
        return (eout, out, vout) if return_image else eout

    def albedo_bins(self, bins, supersample=_capi.SSX_DEMOD_DEFAULT_SUPERSAMPLE, res=None):
        """ssx_albedo_bins -> float32 [H, W, bins]: the first-hit albedo per wavelength bin, averaged over supersample x supersample rays per pixel (1, 2 or 4),
        at the options' resolution or `res` = (W, H).  At supersample 1 and 4 bins it is guides()["albedo"]."""
        W, H = res if res is not None else self.options.res
        rho = np.zeros((H, W, int(bins)), dtype=np.float32)
        self._check(self._lib.ssx_albedo_bins(self._ctx, W, H, int(bins), int(supersample), rho.ctypes.data))
        return rho

    def _demod_args(self, demodulate, bins):
        """(ssx_demod_params, weights_xyz float32 [3, bins]) from demodulate = True (the defaults) or a dict with any of supersample, albedo_floor, weights_xyz;
        the weights default to develop_weights of the render's own observer."""
        d = {} if demodulate is True else dict(demodulate)
        p = _capi.SsxDemodParams()
        p.struct_size = C.sizeof(_capi.SsxDemodParams)
        p.supersample = int(d.pop("supersample", _capi.SSX_DEMOD_DEFAULT_SUPERSAMPLE))
        p.albedo_floor = float(d.pop("albedo_floor", _capi.SSX_DEMOD_DEFAULT_FLOOR))
        w = d.pop("weights_xyz", None)
        if d:
            raise ValueError("demodulate: unknown key(s) %s" % sorted(d))
        if w is None:
            desc = self.scene.desc.contents
            w = develop_weights(bins, float(desc.lambda_min), float(desc.lambda_step), observer=self.options.observer, data_dir=self.options.data_dir)
        w = np.ascontiguousarray(w, dtype=np.float32)
        if w.shape != (3, bins):
            raise ValueError("demodulate: weights_xyz must have shape [3, %d]" % bins)
        return p, w

    def denoise_spectral(self, levels=5, sigma_l=None, sigma_a=0.1, return_image=False, demodulate=None):
        """ssx_denoise_spectral: the wavelength bins the context holds, filtered on the device with the weights denoise() applies to the image -> float32
        [H, W, B], the ratio of the filtered per-bin sums to the filtered sample counts (include/ssx.h); with return_image: (bins, xyza, var), the last
        two those of denoise().  Needs what denoise() needs, and set_spectral_bins before the render; nothing the context holds changes.
        demodulate (True, or a dict: _demod_args): ssx_denoise_spectral_demod -- bins, image and variance are divided by the first-hit albedo before the filter
        and multiplied by it afterwards; sigma_a is ignored.  sigma_l None: 1.0, or the demodulated mode's own default."""
        W, H = self.options.res
        B = self._spectral_bins                                     # what set_spectral_bins set; 0: off, and ssx_denoise_spectral says so
        mean = np.zeros((H, W, B), dtype=np.float32)
        out = np.zeros((H, W, 4), dtype=np.float32) if return_image else None
        var = np.zeros((H, W), dtype=np.float32) if return_image else None
        if sigma_l is None:
            sigma_l = _capi.SSX_DEMOD_DEFAULT_SIGMA_L if demodulate else 1.0
        p = self._denoise_params(levels, sigma_l, sigma_a)
        if demodulate:
            dm, w = self._demod_args(demodulate, B if B else 4)
            self._check(self._lib.ssx_denoise_spectral_demod(self._ctx, C.byref(p), C.byref(dm), w.ctypes.data, mean.ctypes.data if B else None,
                                                             None if out is None else out.ctypes.data, None if var is None else var.ctypes.data))
            return (mean, out, var) if return_image else mean
        self._check(self._lib.ssx_denoise_spectral(self._ctx, C.byref(p), mean.ctypes.data if B else None, None if out is None else out.ctypes.data,
                                                   None if var is None else var.ctypes.data))
        return (mean, out, var) if return_image else mean

    # ---- developing the bins (include/ssx.h: observers, filters, sensors) ----

    def _develop_sensor(self, sensor, denoise, demodulate, optics, defocus, return_raw):
        """develop(sensor=): ssx_spectral_develop_sensor, or for a demodulated source the pure entries by way of the host."""
        W, H = self.options.res
        sp, keep = _sensor_arg(sensor)
        if keep[0] is None:
            raise ValueError("develop: a sensor needs weights [3, B]")
        B = keep[0].shape[1]
        if self._spectral_bins not in (0, B):
            raise ValueError("develop: a sensor for %d bins, the context holds %d" % (B, self._spectral_bins))
        if demodulate and denoise is None:
            denoise = {}
        p = None if denoise is None else self._denoise_params(denoise.get("levels", 5), denoise.get("sigma_l", _capi.SSX_DEMOD_DEFAULT_SIGMA_L if demodulate else 1.0),
                                                              denoise.get("sigma_a", 0.1))
        adc = sp.white > 0
        if demodulate:
            q = self.denoise_spectral(levels=p.levels, sigma_l=p.sigma_l, sigma_a=p.sigma_a, demodulate=demodulate)
            if defocus is not None:
                q = self.defocus_images(q, self.guides()["depth"], defocus)
            if optics is not None:
                q = self.optics_images(q, optics)
            raw, dn = self.sensor_images(q, sensor, return_dn=True) if adc else (self.sensor_images(q, sensor), None)
            out = self.demosaic_images(raw, sensor)
            return (out, raw, dn) if return_raw else out
        df, keep_f = _defocus_arg(defocus) if defocus is not None else (None, None)
        op, keep_o = _optics_arg(optics, W, H) if optics is not None else (None, None)
        if (keep_f is not None and keep_f[0].size != B) or (keep_o is not None and keep_o[0].size != B):
            raise ValueError("develop: the aperture, the lens and the sensor must be made for the same number of bins")
        out = np.zeros((H, W, 3), dtype=np.float32)
        raw = np.zeros((H, W), dtype=np.float32) if return_raw else None
        dn = np.zeros((H, W), dtype=np.float32) if return_raw and adc else None
        self._check(self._lib.ssx_spectral_develop_sensor(self._ctx, None if p is None else C.byref(p), None if df is None else C.byref(df), None if op is None else C.byref(op),
                                                          C.byref(sp), out.ctypes.data, None if raw is None else raw.ctypes.data, None if dn is None else dn.ctypes.data))
        return (out, raw, dn) if return_raw else out

    def sensor_images(self, q, sensor, return_dn=False):
        """ssx_sensor_images: SENSOR (include/ssx.h "Developing onto a sensor") as a pure function: q [H, W, B] -> the mosaic raw float32 [H, W], one filter of
        the sensor's colour filter array per photosite, in the units of a develop with sensor["weights"]; with return_dn (needs an ADC): (raw, the ADC's numbers
        float32 [H, W])."""
        q = np.ascontiguousarray(q, dtype=np.float32)
        if q.ndim != 3:
            raise ValueError("sensor_images: q must have shape [H, W, B]")
        H, W, B = q.shape
        sp, keep = _sensor_arg(sensor)
        if keep[0] is not None and keep[0].shape[1] != B:
            raise ValueError("sensor_images: a sensor for %d bins, q has %d" % (keep[0].shape[1], B))
        raw = np.zeros((H, W), dtype=np.float32)
        dn = np.zeros((H, W), dtype=np.float32) if return_dn else None
        self._check(self._lib.ssx_sensor_images(self._ctx, W, H, B, q.ctypes.data, C.byref(sp), raw.ctypes.data, None if dn is None else dn.ctypes.data))
        return (raw, dn) if return_dn else raw

    def demosaic_images(self, raw, sensor):
        """ssx_demosaic_images: DEMOSAIC as a pure function: raw [H, W] -> float32 [H, W, 3] by the sensor's taps [4, 3, 25] and ccm [3, 3]."""
        raw = np.ascontiguousarray(raw, dtype=np.float32)
        if raw.ndim != 2:
            raise ValueError("demosaic_images: raw must have shape [H, W]")
        H, W = raw.shape
        sp, keep = _sensor_arg(sensor)
        out = np.zeros((H, W, 3), dtype=np.float32)
        self._check(self._lib.ssx_demosaic_images(self._ctx, W, H, raw.ctypes.data, C.byref(sp), out.ctypes.data))
        return out

    def _develop_glare(self, weights, denoise, demodulate, optics, defocus, glare, sensor, return_bins, return_raw):
        """develop(glare=): ssx_spectral_develop_glare; a sensor or a demodulated source by way of the bins behind the glare and the pure entries."""
        W, H = self.options.res
        gp, keep_g = _glare_arg(glare)
        B = keep_g[0].size
        if self._spectral_bins not in (0, B):
            raise ValueError("develop: a glare for %d bins, the context holds %d" % (B, self._spectral_bins))
        if sensor is not None and return_bins:
            raise ValueError("develop: return_bins is not offered with a sensor (return_raw is)")
        if sensor is None and return_raw:
            raise ValueError("develop: return_raw needs a sensor")
        if demodulate and denoise is None:
            denoise = {}
        p = None if denoise is None else self._denoise_params(denoise.get("levels", 5), denoise.get("sigma_l", _capi.SSX_DEMOD_DEFAULT_SIGMA_L if demodulate else 1.0),
                                                              denoise.get("sigma_a", 0.1))
        w = None
        if sensor is None:
            w = np.ascontiguousarray(weights, dtype=np.float32)
            if w.ndim != 2 or w.shape[1] != B:
                raise ValueError("develop: weights must have shape [C, B], B that of the glare")
        if demodulate:
            q = self.denoise_spectral(levels=p.levels, sigma_l=p.sigma_l, sigma_a=p.sigma_a, demodulate=demodulate)
            if defocus is not None:
                q = self.defocus_images(q, self.guides()["depth"], defocus)
            if optics is not None:
                q = self.optics_images(q, optics)
            q = self.glare_images(q, glare)
        else:
            df, keep_f = _defocus_arg(defocus) if defocus is not None else (None, None)
            op, keep_o = _optics_arg(optics, W, H) if optics is not None else (None, None)
            if (keep_f is not None and keep_f[0].size != B) or (keep_o is not None and keep_o[0].size != B):
                raise ValueError("develop: the aperture, the lens and the glare must be made for the same number of bins")
            out = None if sensor is not None else np.zeros((H, W, w.shape[0]), dtype=np.float32)
            q = np.zeros((H, W, B), dtype=np.float32) if sensor is not None or return_bins else None
            self._check(self._lib.ssx_spectral_develop_glare(self._ctx, None if p is None else C.byref(p), None if df is None else C.byref(df), None if op is None else C.byref(op),
                                                             C.byref(gp), None if w is None else w.ctypes.data, 0 if w is None else w.shape[0],
                                                             None if out is None else out.ctypes.data, None if q is None else q.ctypes.data))
            if sensor is None:
                return (out, q) if return_bins else out
        if sensor is None:
            out = self.develop_images(q, w)
            return (out, q) if return_bins else out
        sp, _keep = _sensor_arg(sensor)
        adc = sp.white > 0
        raw, dn = self.sensor_images(q, sensor, return_dn=True) if adc else (self.sensor_images(q, sensor), None)
        out = self.demosaic_images(raw, sensor)
        return (out, raw, dn) if return_raw else out

    def glare_images(self, q, glare):
        """ssx_glare_images: the glare (glare_aperture) as a pure function: q [H, W, B] -> float32 [H, W, B], every `on` bin convolved with its own point spread
        function by a padded FFT (include/ssx.h "Glare: per-bin convolution by FFT"), the other bins copied."""
        q = np.ascontiguousarray(q, dtype=np.float32)
        if q.ndim != 3:
            raise ValueError("glare_images: q must have shape [H, W, B]")
        H, W, B = q.shape
        gp, keep = _glare_arg(glare)
        if keep[0].size != B:
            raise ValueError("glare_images: a glare for %d bins, q has %d" % (keep[0].size, B))
        out = np.zeros((H, W, B), dtype=np.float32)
        self._check(self._lib.ssx_glare_images(self._ctx, W, H, B, q.ctypes.data, C.byref(gp), out.ctypes.data))
        return out

    # ---- finishing a development for a display (include/ssx.h: meter, local tone map, tone curve) ----

    @staticmethod
    def _display_image(what, image):
        image = np.ascontiguousarray(image, dtype=np.float32)
        if image.ndim != 3 or image.shape[2] != 3:
            raise ValueError("%s: the image must have shape [H, W, 3]" % what)
        return image

    def meter_images(self, image, luma, mask=None):
        """ssx_meter_images: METER (include/ssx.h "Finishing a development for a display") as a pure function: image [H, W, 3], luma [3], mask uint8 [H, W] or None (0:
        not counted) -> (hist uint32 [4, 4096], special uint32 [4, 4]): the channels' and the luminance's counts in sixteen keys per octave, and of +-0, negative, +inf
        and NaN values."""
        image = self._display_image("meter_images", image)
        H, W, _ = image.shape
        luma = np.ascontiguousarray(luma, dtype=np.float32)
        if luma.shape != (3,):
            raise ValueError("meter_images: luma must hold three entries")
        if mask is not None:
            mask = np.ascontiguousarray(mask, dtype=np.uint8)
            if mask.shape != (H, W):
                raise ValueError("meter_images: mask must have shape [H, W]")
        hist = np.zeros((4, _capi.SSX_METER_KEYS), dtype=np.uint32)
        special = np.zeros((4, 4), dtype=np.uint32)
        self._check(self._lib.ssx_meter_images(self._ctx, W, H, image.ctypes.data, luma.ctypes.data, None if mask is None else mask.ctypes.data, hist.ctypes.data,
                                               special.ctypes.data))
        return hist, special

    def local_images(self, image, luma, radius, compress, boost=1.0, eps=DISPLAY_LOCAL_EPS, exposure=1.0, pivot=0.0, y_lo=DISPLAY_Y_LO, y_hi=DISPLAY_Y_HI, return_base=False):
        """ssx_local_images: LOCAL as a pure function: image [H, W, 3] -> the gain float32 [H, W] that compresses the base layer of the integer log-luminance (a
        self-guided filter of radius `radius`, flatness `eps`) about `pivot` by `compress` and scales the detail by `boost`; with return_base: (gain, base [H, W])."""
        image = self._display_image("local_images", image)
        H, W, _ = image.shape
        luma = np.ascontiguousarray(luma, dtype=np.float32)
        if luma.shape != (3,):
            raise ValueError("local_images: luma must hold three entries")
        p = _capi.SsxLocalParams()
        p.struct_size = C.sizeof(_capi.SsxLocalParams)
        p.radius = int(radius) & 0xFFFFFFFF
        p.exposure, p.y_lo, p.y_hi, p.eps, p.pivot, p.compress, p.boost = float(exposure), float(y_lo), float(y_hi), float(eps), float(pivot), float(compress), float(boost)
        gain = np.zeros((H, W), dtype=np.float32)
        base = np.zeros((H, W), dtype=np.float32) if return_base else None
        self._check(self._lib.ssx_local_images(self._ctx, W, H, image.ctypes.data, luma.ctypes.data, C.byref(p), gain.ctypes.data, None if base is None else base.ctypes.data))
        return (gain, base) if return_base else gain

    def tone_images(self, image, curve, lo=DISPLAY_LO, hi=DISPLAY_HI, shift=DISPLAY_SHIFT, gains=(1.0, 1.0, 1.0), matrix=None, local=None):
        """ssx_tone_images: TONE as a pure function: image [H, W, 3] -> float32 [H, W, 3]: channel gains, the local gain [H, W] if there is one, the matrix [3, 3]
        (None: identity), then the table `curve` (tone_curve) over [lo, hi] with 2^(23 - shift) nodes per octave."""
        image = self._display_image("tone_images", image)
        H, W, _ = image.shape
        curve = np.ascontiguousarray(curve, dtype=np.float32)
        matrix = np.eye(3, dtype=np.float32) if matrix is None else np.ascontiguousarray(matrix, dtype=np.float32)
        gains = np.ascontiguousarray(gains, dtype=np.float32)
        if curve.ndim != 1 or matrix.shape != (3, 3) or gains.shape != (3,):
            raise ValueError("tone_images: curve must have shape [n], matrix [3, 3], gains [3]")
        if local is not None:
            local = np.ascontiguousarray(local, dtype=np.float32)
            if local.shape != (H, W):
                raise ValueError("tone_images: local must have shape [H, W]")
        p = _capi.SsxToneParams()
        p.struct_size = C.sizeof(_capi.SsxToneParams)
        p.shift, p.curve_len, p.lo, p.hi = int(shift) & 0xFFFFFFFF, curve.size, float(lo), float(hi)
        p.gains = (C.c_float * 3)(*gains.tolist())
        p.matrix = (C.c_float * 9)(*matrix.reshape(-1).tolist())
        p.curve = curve.ctypes.data
        out = np.zeros((H, W, 3), dtype=np.float32)
        self._check(self._lib.ssx_tone_images(self._ctx, W, H, image.ctypes.data, None if local is None else local.ctypes.data, C.byref(p), out.ctypes.data))
        return out

    def finish(self, image, display, return_meter=False):
        """A development finished for a display: METER, ssh_meter_derive, LOCAL where display["local"] asks for it, TONE.  image [H, W, 3] (in display["space"]) ->
        float32 [H, W, 3], display-encoded (the curve holds the sRGB transfer function): nothing further is to be applied.  display: see _display_arg; {} gives an
        extended Reinhard curve whose white point is the luminance's 99th percentile, exposed for a log-average of 0.18.  With return_meter: (image, (hist, special))."""
        d = _display_arg(display, self.options.observer, self.options.data_dir)
        image = self._display_image("finish", image)
        hist, special = self.meter_images(image, d["luma"], d["mask"])
        m = meter_derive(hist, special, key=d["key"], white_percentile=d["white_percentile"])
        wb = {"none": np.ones(3, dtype=np.float32), "grey": m["grey"], "white-patch": m["patch"]}[d["wb"]]
        gains = np.float32(m["exposure"]) * wb.astype(np.float32)
        local = None
        if d["local"] is not None:
            loc = d["local"]
            local = self.local_images(image, d["luma"], loc["radius"], loc["compress"], boost=loc["boost"], eps=loc["eps"], exposure=m["exposure"], pivot=m["pivot"])
        white = float(m["white_exposed"]) if m["white_exposed"] > 0 else 1.0
        curve = tone_curve(d["curve"], d["lo"], d["hi"], d["shift"], white=white)
        out = self.tone_images(image, curve, lo=d["lo"], hi=d["hi"], shift=d["shift"], gains=gains, matrix=d["matrix"], local=local)
        return (out, (hist, special)) if return_meter else out

    def develop(self, weights, denoise=None, demodulate=None, optics=None, return_bins=False, defocus=None, sensor=None, return_raw=False, glare=None, display=None):
        """_develop (below: every argument but `display` is its own) and, with a display dict, finish() on the image it returns (three channels: in display["space"]);
        what else it returns (return_bins, return_raw) stays as it is.  display None: _develop's result."""
        r = self._develop(weights, denoise=denoise, demodulate=demodulate, optics=optics, return_bins=return_bins, defocus=defocus, sensor=sensor, return_raw=return_raw,
                          glare=glare)
        if display is None:
            return r
        if isinstance(r, tuple):
            return (self.finish(r[0], display),) + tuple(r[1:])
        return self.finish(r, display)

    def _develop(self, weights, denoise=None, demodulate=None, optics=None, return_bins=False, defocus=None, sensor=None, return_raw=False, glare=None):
        """ssx_spectral_develop: the bins the context holds, mapped on the device by weights [C, B] (develop_weights) -> float32 [H, W, C], row 0 = bottom.
        denoise None: the raw source, q = S * M / n; a dict of denoise_spectral's parameters (levels, sigma_l, sigma_a; {} for the defaults): the filtered bins,
        developed without leaving the device.  demodulate (True or a dict, as in denoise_spectral; denoise None counts as {}): ssx_spectral_develop_demod, the
        bins filtered in the demodulated mode.  optics (a lens: lens_optics): ssx_spectral_develop_optics, the source through the lens before it is developed,
        still on the device; with return_bins: (image, the bins behind the lens float32 [H, W, B]).  A demodulated source goes through the lens by way of the
        host: denoise_spectral(demodulate=), optics_images, develop_images.  defocus (an aperture: thin_lens_defocus): ssx_spectral_develop_lens, the source
        defocused with the context's own depth guide, then through the lens if there is one, then developed, still on the device; return_bins as with optics; a
        demodulated source by way of the host again (defocus_images with guides()["depth"]).  sensor (a dict: sensor_bayer's and sensor_exposure's entries,
        "weights" [3, B], "ccm" [3, 3], and "noise", "seed", "frame"): ssx_spectral_develop_sensor -- behind the aperture and the lens the bins fall on a colour
        filter array, are counted, digitised and demosaiced on the device; `weights` is then not used (None will do), the result is float32 [H, W, 3], and with
        return_raw: (image, the mosaic [H, W], the ADC's numbers [H, W] or None).  glare (a dict: glare_aperture): ssx_spectral_develop_glare -- behind the
        aperture and the lens every bin is convolved with its own point spread function, then developed, still on the device; return_bins gives the bins behind
        the glare; with a sensor, or a demodulated source, the bins go by way of the host and the pure entries.  Nothing the context holds changes."""
        if glare is not None:
            return self._develop_glare(weights, denoise, demodulate, optics, defocus, glare, sensor, return_bins, return_raw)
        if sensor is not None:
            if return_bins:
                raise ValueError("develop: return_bins is not offered with a sensor (return_raw is)")
            return self._develop_sensor(sensor, denoise, demodulate, optics, defocus, return_raw)
        if return_raw:
            raise ValueError("develop: return_raw needs a sensor")
        W, H = self.options.res
        w = np.ascontiguousarray(weights, dtype=np.float32)
        if w.ndim != 2:
            raise ValueError("develop: weights must have shape [C, B]")
        out = np.zeros((H, W, w.shape[0]), dtype=np.float32)
        if demodulate and denoise is None:
            denoise = {}
        p = None if denoise is None else self._denoise_params(denoise.get("levels", 5), denoise.get("sigma_l", _capi.SSX_DEMOD_DEFAULT_SIGMA_L if demodulate else 1.0),
                                                              denoise.get("sigma_a", 0.1))
        if self._spectral_bins not in (0, w.shape[1]):
            raise ValueError("develop: weights for %d bins, the context holds %d" % (w.shape[1], self._spectral_bins))
        if return_bins and optics is None and defocus is None:
            raise ValueError("develop: return_bins needs optics or defocus")
        if defocus is not None and demodulate:
            q = self.defocus_images(self.denoise_spectral(levels=p.levels, sigma_l=p.sigma_l, sigma_a=p.sigma_a, demodulate=demodulate), self.guides()["depth"], defocus)
            if optics is not None:
                q = self.optics_images(q, optics)
            out = self.develop_images(q, w)
            return (out, q) if return_bins else out
        if defocus is not None:
            df, keep_f = _defocus_arg(defocus)
            if keep_f[0].size != w.shape[1]:
                raise ValueError("develop: an aperture for %d bins, weights for %d" % (keep_f[0].size, w.shape[1]))
            op, keep = _optics_arg(optics, W, H) if optics is not None else (None, None)
            if keep is not None and keep[0].size != w.shape[1]:
                raise ValueError("develop: a lens for %d bins, weights for %d" % (keep[0].size, w.shape[1]))
            bins_out = np.zeros((H, W, w.shape[1]), dtype=np.float32) if return_bins else None
            self._check(self._lib.ssx_spectral_develop_lens(self._ctx, None if p is None else C.byref(p), C.byref(df), None if op is None else C.byref(op), w.ctypes.data,
                                                            w.shape[0], out.ctypes.data, None if bins_out is None else bins_out.ctypes.data))
            return (out, bins_out) if return_bins else out
        if optics is not None and demodulate:
            q = self.optics_images(self.denoise_spectral(levels=p.levels, sigma_l=p.sigma_l, sigma_a=p.sigma_a, demodulate=demodulate), optics)
            out = self.develop_images(q, w)
            return (out, q) if return_bins else out
        if optics is not None:
            op, keep = _optics_arg(optics, W, H)
            if keep[0].size != w.shape[1]:
                raise ValueError("develop: a lens for %d bins, weights for %d" % (keep[0].size, w.shape[1]))
            bins_out = np.zeros((H, W, w.shape[1]), dtype=np.float32) if return_bins else None
            self._check(self._lib.ssx_spectral_develop_optics(self._ctx, None if p is None else C.byref(p), C.byref(op), w.ctypes.data, w.shape[0], out.ctypes.data,
                                                              None if bins_out is None else bins_out.ctypes.data))
            return (out, bins_out) if return_bins else out
        if demodulate:
            dm, wx = self._demod_args(demodulate, w.shape[1])
            self._check(self._lib.ssx_spectral_develop_demod(self._ctx, C.byref(p), C.byref(dm), wx.ctypes.data, w.ctypes.data, w.shape[0], out.ctypes.data))
            return out
        self._check(self._lib.ssx_spectral_develop(self._ctx, None if p is None else C.byref(p), w.ctypes.data, w.shape[0], out.ctypes.data))
        return out

    def develop_images(self, q, weights):
        """ssx_develop_images: the same map as a pure function: q [H, W, B], weights [C, B] -> float32 [H, W, C]."""
        q = np.ascontiguousarray(q, dtype=np.float32)
        w = np.ascontiguousarray(weights, dtype=np.float32)
        if q.ndim != 3 or w.ndim != 2 or w.shape[1] != q.shape[2]:
            raise ValueError("develop_images: q must have shape [H, W, B], weights [C, B]")
        H, W, B = q.shape
        out = np.zeros((H, W, w.shape[0]), dtype=np.float32)
        self._check(self._lib.ssx_develop_images(self._ctx, W, H, B, q.ctypes.data, w.ctypes.data, w.shape[0], out.ctypes.data))
        return out

    def optics_images(self, q, optics):
        """ssx_optics_images: the lens (lens_optics) as a pure function: q [H, W, B] -> float32 [H, W, B], each bin resampled about the optical centre with its
        own magnification and blurred with its own separable kernel (include/ssx.h "Developing through a lens")."""
        q = np.ascontiguousarray(q, dtype=np.float32)
        if q.ndim != 3:
            raise ValueError("optics_images: q must have shape [H, W, B]")
        H, W, B = q.shape
        op, keep = _optics_arg(optics, W, H)
        if keep[0].size != B:
            raise ValueError("optics_images: a lens for %d bins, q has %d" % (keep[0].size, B))
        out = np.zeros((H, W, B), dtype=np.float32)
        self._check(self._lib.ssx_optics_images(self._ctx, W, H, B, q.ctypes.data, C.byref(op), out.ctypes.data))
        return out

    def defocus_images(self, q, depth, defocus):
        """ssx_defocus_images: the aperture (thin_lens_defocus) as a pure function: q [H, W, B], depth [H, W] -> float32 [H, W, B], every (pixel, bin) gathered
        over its neighbours' circles of confusion (include/ssx.h "Depth of field after the render")."""
        q = np.ascontiguousarray(q, dtype=np.float32)
        depth = np.ascontiguousarray(depth, dtype=np.float32)
        if q.ndim != 3 or depth.shape != q.shape[:2]:
            raise ValueError("defocus_images: q must have shape [H, W, B], depth [H, W]")
        H, W, B = q.shape
        df, keep = _defocus_arg(defocus)
        if keep[0].size != B:
            raise ValueError("defocus_images: an aperture for %d bins, q has %d" % (keep[0].size, B))
        out = np.zeros((H, W, B), dtype=np.float32)
        self._check(self._lib.ssx_defocus_images(self._ctx, W, H, B, q.ctypes.data, depth.ctypes.data, C.byref(df), out.ctypes.data))
        return out

    def debug_sample_flux(self, **over):
        """ssx_debug_sample_flux (spectral output on): per-sample (flux [H, W, spp, 4] float32, lambda_0 [H, W, spp] float32)."""
        p = self.params(**over)
        flux = np.zeros((p.height, p.width, p.spp, 4), dtype=np.float32)
        lambda_0 = np.zeros((p.height, p.width, p.spp), dtype=np.float32)
        self._check(self._lib.ssx_debug_sample_flux(self._ctx, C.byref(p), flux.ctypes.data, lambda_0.ctypes.data))
        return flux, lambda_0

    def render_device(self, d_ptr, stream=0, **over):
        """Enqueue the render on `stream` into the device buffer at d_ptr (W*H float4)."""
        p = self.params(**over)
        self._check(self._lib.ssx_render_device(self._ctx, C.byref(p), C.c_void_p(d_ptr), C.c_void_p(stream)))

    def render_device_wait(self):
        """ssx_render_device_wait: host wait for what render_device has queued for this context."""
        self._check(self._lib.ssx_render_device_wait(self._ctx))

    def set_jit(self, mode=_capi.SSX_JIT_AT_UPLOAD):
        """ssx_set_jit: SSX_JIT_OFF / SSX_JIT_AT_UPLOAD / SSX_JIT_BACKGROUND (True / False: at upload / off)."""
        self._check(self._lib.ssx_set_jit(self._ctx, int(mode)))

    def jit_status(self, wait_ms=0):
        """ssx_jit_status -> (state, message): SSX_JIT_STATE_NONE / _GENERIC_MEANWHILE / _SPECIALISED / _FAILED.  wait_ms != 0 asks
        for the compilation now and waits for it (< 0: until done)."""
        buf = C.create_string_buffer(1024)
        st = self._lib.ssx_jit_status(self._ctx, int(wait_ms), buf, len(buf))
        if st < -1:
            self._check(st)
        return st, buf.value.decode(errors="replace")

    def upload_scene_desc(self, desc):
        """Replace the scene by an arbitrary ssx_scene_desc (the flat description the C ABI takes)."""
        self._check(self._lib.ssx_upload_scene(self._ctx, C.byref(desc) if not hasattr(desc, "contents") else desc))

    def debug_eval(self, op, inputs, out_words):
        """ssx_debug_eval: `inputs` is an [n, in_words] array of 32-bit words (float32 or uint32 views);
        returns a uint32 array [n, out_words] (view it as float32 where the op returns floats)."""
        x = np.ascontiguousarray(inputs)
        assert x.ndim == 2 and x.dtype.itemsize == 4
        out = np.zeros((x.shape[0], out_words), dtype=np.uint32)
        self._check(self._lib.ssx_debug_eval(self._ctx, op, x.ctypes.data, x.shape[1], out.ctypes.data, out_words, x.shape[0]))
        return out

    def debug_sweep(self, op, lo=0, count=1 << 32):
        """ssx_debug_sweep -> (mismatches, op-specific maximum, [mismatching input bit patterns])"""
        res = (C.c_uint64 * 11)()
        self._check(self._lib.ssx_debug_sweep(self._ctx, op, lo, count, res))
        return int(res[0]), int(res[1]), [int(res[3 + k]) for k in range(min(int(res[2]), 8))]

    def debug_samples(self, **over):
        """ssx_debug_samples: per-sample (xyza [H, W, spp, 4], final PCG32 state [H, W, spp] uint64, levels [H, W, spp])."""
        p = self.params(**over)
        xyza = np.zeros((p.height, p.width, p.spp, 4), dtype=np.float32)
        state = np.zeros((p.height, p.width, p.spp), dtype=np.uint64)
        levels = np.zeros((p.height, p.width, p.spp), dtype=np.uint32)
        self._check(self._lib.ssx_debug_samples(self._ctx, C.byref(p), xyza.ctypes.data, state.ctypes.data, levels.ctypes.data))
        return xyza, state, levels

    def debug_tile_mask(self, **over):
        """ssx_debug_tile_mask: uint32 [slots, 4], the primitives ssx_tile_mask_kernel leaves to the camera rays of each of the device's tile slots (slot s =
        tile tile_first + s * tile_stride of the skewed tile list; bit q & 31 of word q >> 5 = primitive q), for a render with these options."""
        p = self.params(**over)
        tx, ty = (p.width + 7) // 8, (p.height + 7) // 8
        slots = (tx * ty - p.tile_first + p.tile_stride - 1) // p.tile_stride if tx * ty > p.tile_first else 0
        out = np.zeros((slots, 4), dtype=np.uint32)
        self._check(self._lib.ssx_debug_tile_mask(self._ctx, C.byref(p), out.ctypes.data))
        return out

    def debug_generate(self, k0=0, n_k=1, pre_hits=-1, **over):
        """ssx_debug_generate: ssx_generate_kernel's records for samples [k0, k0 + n_k) of the device's tiles, in the kernel's own order -> (ray, st, hit), each
        uint32 [slots, n_k, 64, 4] (float32 words as their bits; lane = 8 * row + column of the tile).  pre_hits: 0 / 1 / -1 (the context's own choice).  Words no
        lane wrote hold _capi.SSX_GENERATE_FILL_BYTE in every byte: all of hit without pre_hits, and the lanes outside a ragged image."""
        p = self.params(**over)
        tx, ty = (p.width + 7) // 8, (p.height + 7) // 8
        slots = (tx * ty - p.tile_first + p.tile_stride - 1) // p.tile_stride if tx * ty > p.tile_first else 0
        ray, st, hit = (np.zeros((slots, int(n_k), 64, 4), dtype=np.uint32) for _ in range(3))
        self._check(self._lib.ssx_debug_generate(self._ctx, C.byref(p), int(k0), int(n_k), int(pre_hits), ray.ctypes.data, st.ctypes.data, hit.ctypes.data))
        return ray, st, hit

    def generate_info(self):
        """ssx_generate_info: launches of this context's renders in front of which the generate kernel ran, and launches whose path kernel made its samples itself."""
        a, b = C.c_uint64(), C.c_uint64()
        self._check(self._lib.ssx_generate_info(self._ctx, C.byref(a), C.byref(b)))
        return {"generate_launches": a.value, "fused_launches": b.value}

    def debug_fold(self, levels, spp, order_seed=0, parked=False, flux=False, **over):
        """ssx_debug_fold: the path kernel's fold on `levels`, uint32 [n_pixels * spp, SSX_FOLD_ROW_WORDS] rows in [pixel][k] order (n_pixels a multiple of 64)
        -> (flux uint32 [n, 4] or None, xyza uint32 [n, 4], sums float64 [n_pixels, 4]): the float32 results as their bits."""
        x = np.ascontiguousarray(levels, dtype=np.uint32)
        if x.ndim != 2 or x.shape[1] != _capi.SSX_FOLD_ROW_WORDS or spp < 1 or x.shape[0] % spp:
            raise ValueError("debug_fold: levels must be [n_pixels * spp, %d] words" % _capi.SSX_FOLD_ROW_WORDS)
        n, n_pixels = x.shape[0], x.shape[0] // spp
        fl = np.zeros((n, 4), dtype=np.uint32) if flux else None
        xyza, sums = np.zeros((n, 4), dtype=np.uint32), np.zeros((n_pixels, 4), dtype=np.float64)
        self._check(self._lib.ssx_debug_fold(self._ctx, C.byref(self.params(**over)), n_pixels, int(spp), x.ctypes.data, int(order_seed) & 0xFFFFFFFF, int(bool(parked)),
                                             None if fl is None else fl.ctypes.data, xyza.ctypes.data, sums.ctypes.data))
        return fl, xyza, sums

    def debug_step(self, rows, n_rounds, **over):
        """ssx_debug_step: one iteration of the path loop per round on `rows`, uint32 [n_tiles * n_rounds * 64, SSX_STEP_ROW_WORDS] in [tile][round][lane] order
        -> uint32 [n, SSX_STEP_OUT_WORDS] (float32 results as their bits); `over`: fields of ssx_render_params (no_explicit_light_sampling, indirect_only, libm)."""
        x = np.ascontiguousarray(rows, dtype=np.uint32)
        if x.ndim != 2 or x.shape[1] != _capi.SSX_STEP_ROW_WORDS:
            raise ValueError("debug_step: rows must be [n, %d] words" % _capi.SSX_STEP_ROW_WORDS)
        out = np.zeros((x.shape[0], _capi.SSX_STEP_OUT_WORDS), dtype=np.uint32)
        self._check(self._lib.ssx_debug_step(self._ctx, C.byref(self.params(**over)), x.shape[0], int(n_rounds), x.ctypes.data, out.ctypes.data))
        return out

    def debug_spectral_accumulate(self, flux, lambda_0, bins, lambda_min, lambda_step, n_k=None, tile_first=0, tile_stride=1, tile_skew=0, moments=True):
        """ssx_debug_spectral_accumulate: the render's bin and moment kernels on the caller's records -- flux float32 [H, W, K, 4], lambda_0 float32 [H, W, K],
        given to the kernels as len(n_k) launches of n_k[l] samples per pixel (None: one launch of K) -> (sums float64 [H, W, B], counts uint32 [H, W, B / 4],
        q float64 [H, W, B] or None without moments); +0.0 / 0 for pixels the tile list of tile_first / tile_stride / tile_skew does not own.  The arrays go to
        the library as they are: their bits, NaN payloads included, are what the kernels read."""
        flux, lambda_0 = np.ascontiguousarray(flux, dtype=np.float32), np.ascontiguousarray(lambda_0, dtype=np.float32)
        if flux.ndim != 4 or flux.shape[3] != 4 or lambda_0.shape != flux.shape[:3]:
            raise ValueError("debug_spectral_accumulate: flux must have shape [H, W, K, 4], lambda_0 [H, W, K]")
        H, W, K = lambda_0.shape
        n_k = np.ascontiguousarray([K] if n_k is None else n_k, dtype=np.uint32)
        if n_k.ndim != 1 or int(n_k.astype(np.uint64).sum()) != K:
            raise ValueError("debug_spectral_accumulate: the launch lengths n_k must add up to K = %d" % K)
        B = int(bins)
        sums, counts = np.zeros((H, W, B), dtype=np.float64), np.zeros((H, W, max(B // 4, 1)), dtype=np.uint32)
        q = np.zeros((H, W, B), dtype=np.float64) if moments else None
        self._check(self._lib.ssx_debug_spectral_accumulate(self._ctx, W, H, B, int(tile_first), int(tile_stride), int(tile_skew), float(lambda_min), float(lambda_step),
                                                            len(n_k), n_k.ctypes.data, flux.ctypes.data, lambda_0.ctypes.data, sums.ctypes.data, counts.ctypes.data,
                                                            None if q is None else q.ctypes.data))
        return sums, counts, q

    def set_timing(self, enable=True):
        self._check(self._lib.ssx_set_timing(self._ctx, int(enable)))

    def get_timing(self):
        """Summed ms {generate, path, resolve, accumulate} of the launches since the last call."""
        ms = (C.c_float * 4)()
        self._check(self._lib.ssx_get_timing(self._ctx, ms))
        return dict(zip(("generate", "path", "resolve", "accumulate"), [float(x) for x in ms]))

    def kernel_info(self):
        v = [C.c_int() for _ in range(5)]
        self._check(self._lib.ssx_kernel_info(self._ctx, *[C.byref(x) for x in v]))
        return dict(zip(("vgprs", "sgprs", "lds_bytes", "scratch_bytes", "max_blocks_per_cu"), [x.value for x in v]))

    def plan_info(self):
        """What the calibration render at scene upload found: frames per sample, and where the fold runs."""
        f, k = C.c_float(), C.c_int()
        self._check(self._lib.ssx_plan_info(self._ctx, C.byref(f), C.byref(k)))
        variant = {0: "generic", 1: "cornell topology", 2: "plane topology", 3: "scene topology (compiled at upload)"}.get(self._lib.ssx_kernel_variant(self._ctx), "?")
        name = self._lib.ssx_kernel_name(self._ctx)
        left, pre = C.c_float(), C.c_int()
        if hasattr(self._lib, "ssx_calibration_info"):  # (an older build loaded through SSX_HIP_LIB_OVERRIDE for an A/B run has neither)
            self._check(self._lib.ssx_calibration_info(self._ctx, None, C.byref(left), C.byref(pre)))
        # where a sample's stream / camera ray / lambda_0 are made: the generate kernel, or -- kernels of the plane topology whose camera rays are
        # traced in the path loop (csrc/ssx_api.hip fuses_generate: fuse_gen) -- the path kernel's refill
        fused = (not pre.value) and variant == "plane topology" and not (os.environ.get("SSX_DEBUG_ENV") == "1" and os.environ.get("SSX_FUSE_GEN", "")[:1] == "0")
        return {"frames_per_sample": round(f.value, 3), "fold": "path kernel", "pass1": variant,
                "rays_left_per_sample": round(left.value, 3), "camera_rays": "pre-traced (generate kernel)" if pre.value else "path loop",
                "samples_made_in": "path kernel (refill)" if fused else "generate kernel",
                "kernel": name.decode() if name else None,
                # the render switches (explicit light sampling, indirect_only, mirror / triangle-light scene, uplift, RGB mode, flat field): compiled into
                # the kernel the current (or last) render ran -- its "_plain" twin, named as "kernel" above -- or tested at run time (ssx_switches_info)
                "switches": "compiled in" if hasattr(self._lib, "ssx_switches_info") and self._lib.ssx_switches_info(self._ctx) == 1 else "run time"}

    def scratch_info(self):
        """Device scratch held: bytes of per-sample arrays (largest launch so far) and of the persistent waves' level logs."""
        a, b = C.c_uint64(), C.c_uint64()
        if hasattr(self._lib, "ssx_scratch_info"):
            self._check(self._lib.ssx_scratch_info(self._ctx, C.byref(a), C.byref(b)))
        return {"sample_bytes": a.value, "log_bytes": b.value}

    def sums_info(self):
        """ssx_sums_info: work units that parked their samples instead of waiting for their tile's turn, and how many of those the
        wave in front of them added (cumulative since the context was created)."""
        a, b = C.c_uint64(), C.c_uint64()
        if hasattr(self._lib, "ssx_sums_info"):
            self._check(self._lib.ssx_sums_info(self._ctx, C.byref(a), C.byref(b)))
        u = C.c_uint64()
        if hasattr(self._lib, "ssx_units_info"):
            self._check(self._lib.ssx_units_info(self._ctx, C.byref(u)))
        return {"units_parked": a.value, "units_chained": b.value, "units": u.value}

    def save(self, path):
        fb = np.ascontiguousarray(self.framebuffer, dtype=np.float32)
        _host("ssh_save_image", path.encode(), fb.ctypes.data, fb.shape[1], fb.shape[0])

    def close(self):
        if self._ctx:
            self._lib.ssx_destroy(self._ctx)
            self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
