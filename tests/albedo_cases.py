"""Cases for the albedo device function (csrc/ssx_kernels.hip material_albedo, debug op SSX_DBG_ALBEDO) and the
oracle's orc_quad_albedo: scenes both sides accept, and per scene the items (quad, st, lambda_0).  Pure numpy, no
GPU: tests/test_albedo_units_cpu.py proves on the oracle alone which branches the items reach,
tests/test_albedo_units_gpu.py compares the device function with the oracle on them.  TEST INFRASTRUCTURE.

The numpy restatements below (texel index, table index, Jakob-Hanika tie, Meng cell) classify items; they never
produce an expected value."""
import ctypes as C
import os
import tempfile

import numpy as np

import custom_scene as cs
import oracle_lib as ol
import ref_lib
from simple_spectral_amd.renderer import Scene

F = np.float32
UP, DOWN = F(np.inf), F(-np.inf)

# ------------------------------------------------------------------------------------------- textures ----
SMALL = {"1x1": (1, 1), "1x7": (1, 7), "7x1": (7, 1), "5x3": (5, 3)}        # name -> (w, h)


def small_texture(w, h):
    """[h, w, 3] with a different colour in every texel, none black: a wrong row or column shows"""
    j, i = np.mgrid[0:h, 0:w]
    return np.stack([16 + 32 * i, 25 + 32 * j, 250 - 11 * i - 3 * j], axis=-1).astype(np.uint8)


def ramp_texture():
    """256 x 3: row c holds byte x in channel c at column x, 0 elsewhere -- every entry of the sRGB8 table in every channel"""
    t = np.zeros((3, 256, 3), dtype=np.uint8)
    for c in range(3):
        t[c, :, c] = np.arange(256)
    return t


def lattice_texture():
    """64 x 64: all 16^3 colours with channel values in {0, 17, ..., 255}: black, white, the primaries, every kind of tie"""
    k = np.arange(4096)
    rgb = np.stack([k >> 8, (k >> 4) & 15, k & 15], axis=-1) * 17
    return rgb.astype(np.uint8).reshape(64, 64, 3)


def textures():
    t = {name: small_texture(w, h) for name, (w, h) in SMALL.items()}
    t["ramp"] = ramp_texture()
    t["lattice"] = lattice_texture()
    return t


# spectra shorter than the sampled range, so that the table index leaves the table on both sides (spectrum.cpp:39-60).
# Two samples is the shortest spectrum there is: the reference (spectrum.cpp:17-20), the oracle and ssx_upload_scene refuse n = 1.
SHORT = {"short3": ([0.25, 0.75, 0.5], 500.0, 520.0), "short2": ([0.625, 0.375], 500.0, 520.0)}


# ------------------------------------------------------------------------------------------- st values ----
def axis_values(n):
    """st values along an axis of n texels: centres; every boundary k/n with its two float neighbours (that covers +0, 1 and
    their neighbours); -0; a little and far outside [0, 1]"""
    nf = F(n)
    v = [(F(k) + F(0.5)) / nf for k in range(n)]
    for k in range(n + 1):
        b = F(k) / nf
        v += [b, np.nextafter(b, DOWN), np.nextafter(b, UP)]
    v += [F(-0.0), F(-1e-3), F(1) + F(1e-3), F(3.5), F(-3.5), F(1e6), F(-1e6)]
    return np.array(v, dtype=F)


def centres(w, h):
    """st of every texel centre, [h * w, 2]; row j of the image is at st.y = 1 - (j + 0.5) / h (material.cpp:70-72)"""
    j, i = np.mgrid[0:h, 0:w]
    return np.stack([(i.ravel().astype(F) + F(0.5)) / F(w), (F(h) - (j.ravel().astype(F) + F(0.5))) / F(h)], axis=-1).astype(F)


def texel_index(w, h, st):
    """material.cpp:65-97 restated: (column i, row j) of the texel st selects, clamped to the image"""
    st = np.asarray(st, dtype=F)
    ix = np.floor(st[:, 0] * F(w))
    iy = np.floor(F(h) - st[:, 1] * F(h))
    assert (np.abs(ix) < 2.0 ** 31).all() and (np.abs(iy) < 2.0 ** 31).all()     # (int)floorf(x) is defined
    return np.clip(ix.astype(np.int64), 0, w - 1), np.clip(iy.astype(np.int64), 0, h - 1)


# ------------------------------------------------------------------------------------------- lambda_0 values ----
def common_lambdas(lambda_min, lambda_step, seed=7):
    """the sampler's range [lambda_min, lambda_min + lambda_step] (renderer.cpp:134-143): both ends, their inner neighbours, 5 seeded values"""
    lo, hi = F(lambda_min), F(lambda_min) + F(lambda_step)
    g = np.random.default_rng(seed)
    mid = (lo + (hi - lo) * g.uniform(0.02, 0.98, size=5)).astype(F)
    return np.concatenate([np.array([lo, np.nextafter(lo, UP), hi, np.nextafter(hi, DOWN)], dtype=F), mid])


def delta_recip(low, high, n):
    """spectrum.cpp:22-25 in float arithmetic"""
    return F(n - 1) / (F(high) - F(low))


def node_lambda(low, high, n, i):
    """(wavelength, exact): a wavelength whose table position (lambda - low) * delta_recip is exactly the integer i -- low + i /
    delta_recip or a float next to it -- or, where the product steps over i (exact = False), the float nearest to the node"""
    dr = delta_recip(low, high, n)
    near = [F(low) + F(i) / dr]
    for _ in range(3):
        near = [np.nextafter(near[0], DOWN)] + near + [np.nextafter(near[-1], UP)]
    for x in near + ([F(high)] if i == n - 1 else []):
        if (x - F(low)) * dr == F(i):
            return x, True
    return near[3], False


def table_lambdas(low, high, n, lambda_step):
    """lambda_0 for a table lookup: hero wavelengths 0 and 1 exactly on nodes (first, second, middle, last two), and wavelengths
    below, at and beyond both ends, so that the clamped index takes each of -2, -1, n - 1, n"""
    d = F(1) / delta_recip(low, high, n)
    nodes = [node_lambda(low, high, n, i)[0] for i in sorted({0, 1, n // 2, n - 2, n - 1})]
    v = nodes + [x - F(lambda_step) for x in nodes]
    v += [F(low) + F(k) * d for k in (-3, -2, -1.5, -1, -0.5)] + [F(high) + F(k) * d for k in (-0.5, 0.5, 1, 1.5, 5)]
    v += [F(100), F(2000)]
    return np.array(v, dtype=F)


def table_index(low, high, n, lam):
    """csrc/ssx_kernels.hip hero_index restated from the table's (low, delta_recip, n): per hero wavelength x, floor(x) and the
    index clamped to [-2, n] that reads the blob's zero padding; lam = the hero wavelengths, any shape"""
    x = (np.asarray(lam, dtype=F) - F(low)) * delta_recip(low, high, n)
    i0 = np.floor(x)
    return x, i0, np.clip(i0, -2, n).astype(np.int64)


def hero_wavelengths(lam0, lambda_step):
    """lambda_0 + float(i) * LAMBDA_STEP (spectrum.cpp:63), [n, 4]"""
    return (np.asarray(lam0, dtype=F)[:, None] + (np.arange(4, dtype=F) * F(lambda_step))[None, :]).astype(F)


# ------------------------------------------------------------------------------------------- uplift restatements ----
def jh_tie(lrgb):
    """which components share the maximum-deciding comparisons of rgb2spec.c:82-86: "", "rg", "gb", "rb" or "rgb" """
    r, g, b = (F(v) for v in lrgb)
    if r == g == b:
        return "rgb"
    return "rg" if r == g else "gb" if g == b else "rb" if r == b else ""


def meng_branch(table, lrgb):
    """spectrum_grid.h:13-134 restated as far as the branch goes (no spectrum is read): "black" (norm not finite), "offgrid",
    "inside", ("fan", accepted triangle, triangles in the fan), "notfound" (no triangle of the fan accepts) or "empty" (no points)"""
    r, g, b = (F(v) for v in lrgb)
    rows = [[0.41231515, 0.3576, 0.1805], [0.2126, 0.7152, 0.0722], [0.01932727, 0.1192, 0.95063333]]
    X, Y, Z = (((F(m[0]) * F(100)) * r + (F(m[1]) * F(100)) * g) + (F(m[2]) * F(100)) * b for m in rows)   # color.cpp:189-193
    with np.errstate(divide="ignore", invalid="ignore"):
        norm = F(np.float64(1.0) / np.float64((X + Y) + Z))
        if not norm < np.finfo(F).max:
            return "black"
        m = np.asarray(table["xy_to_uv"], dtype=F)
        x, y = X * norm, Y * norm
        u0, v0 = (m[0] * x + m[1] * y) + m[2], (m[3] * x + m[4] * y) + m[5]
        gw, gh = table["grid_w"], table["grid_h"]
        if u0 < 0 or u0 >= F(gw) or v0 < 0 or v0 >= F(gh):
            return "offgrid"
        cell = np.asarray(table["cells"]).reshape(-1, 8)[int(u0) + gw * int(v0)]
        inside, num, idx = int(cell[0]), int(cell[1]), cell[2:]
        if inside:
            return "inside"
        if num <= 0:
            return "empty"
        uv = np.asarray(table["points"], dtype=F)[:, 2:4]
        p0 = uv[idx[0]]
        ex, ey = u0 - p0[0], v0 - p0[1]
        e0x, e0y = uv[idx[1]][0] - p0[0], uv[idx[1]][1] - p0[1]
        uu = e0x * ey - ex * e0y
        for i in range(num - 1):
            pn = uv[idx[1]] if i == num - 2 else uv[idx[i + 2]]
            e1x, e1y = pn[0] - p0[0], pn[1] - p0[1]
            vv = ex * e1y - e1x * ey
            area = e0x * e1y - e1x * e0y
            u, v = uu / area, vv / area
            w = F(1) - u - v
            if u < 0 or v < 0 or w < 0:
                uu, e0x, e0y = -vv, e1x, e1y
                continue
            return ("fan", i, num - 1)
        return "notfound"


# ------------------------------------------------------------------------------------------- items ----
class Items:
    """rows (quad, st.x, st.y, lambda_0) with the name of the group each row belongs to"""

    def __init__(self):
        self._q, self._st, self._lam, self._group = [], [], [], []

    def add(self, group, quad, st, lam):
        """st [n, 2] and lam [n], or one of them a single value for all rows"""
        st, lam = np.atleast_2d(np.asarray(st, dtype=F)), np.atleast_1d(np.asarray(lam, dtype=F))
        n = max(len(st), len(lam))
        self._q.append(np.full(n, quad, dtype=np.int64))
        self._st.append(np.broadcast_to(st, (n, 2)))
        self._lam.append(np.broadcast_to(lam, (n,)))
        self._group += [group] * n

    def done(self):
        self.quad, self.st, self.lam = np.concatenate(self._q), np.concatenate(self._st).astype(F), np.concatenate(self._lam).astype(F)
        self.group = np.array(self._group)
        assert np.isfinite(self.st).all() and np.isfinite(self.lam).all()
        return self

    def words(self):
        """the [n, 4] input words of SSX_DBG_ALBEDO"""
        w = np.empty((len(self.quad), 4), dtype=np.uint32)
        w[:, 0] = self.quad
        w[:, 1:3] = self.st.view(np.uint32)
        w[:, 3] = self.lam.view(np.uint32)
        return w

    def of(self, group):
        return np.flatnonzero(self.group == group)


def cycle(values, n, start=0):
    return np.asarray(values)[(start + np.arange(n)) % len(values)]


def texture_items(items, quad_of, lams, extra_lams=()):
    """the textured quads' items.  Small textures: the cross product of axis_values in both directions, the lambda_0 list cycled
    through them, and every lambda_0 at every centre; ramp and lattice: texel centres (the lattice twice, with different lambda_0)"""
    lams = np.concatenate([lams, np.asarray(extra_lams, dtype=F)])
    for name, (w, h) in SMALL.items():
        sx, sy = np.meshgrid(axis_values(w), axis_values(h), indexing="ij")
        st = np.stack([sx.ravel(), sy.ravel()], axis=-1)
        items.add(name, quad_of[name], st, cycle(lams, len(st)))
        c = centres(w, h)
        items.add(name, quad_of[name], np.repeat(c, len(lams), axis=0), np.tile(lams, len(c)))
    items.add("ramp", quad_of["ramp"], centres(256, 3), cycle(lams, 768))
    for start in (0, 4):
        items.add("lattice", quad_of["lattice"], centres(64, 64), cycle(lams, 4096, start))


def spectrum_of_quad(desc, quad):
    """(samples, low, high) of the constant albedo of a quad of an ssx_scene_desc"""
    m = desc.materials[desc.quads[quad].material]
    assert m.albedo_mode == 0
    sp = desc.spectra[m.albedo_spectrum]
    return np.array(desc.samples[sp.offset:sp.offset + sp.n], dtype=F), float(sp.low), float(sp.high)


class OrcSpectrum(C.Structure):
    """orc_spectrum (oracle/oracle.h), for orc_spectrum_hero on a table the test builds itself"""
    _fields_ = [("data", C.POINTER(C.c_float)), ("n", C.c_int), ("low", C.c_float), ("high", C.c_float),
                ("delta_lambda", C.c_float), ("delta_lambda_recip", C.c_float)]

    @classmethod
    def make(cls, data, low, high):
        data = np.ascontiguousarray(data, dtype=F)
        s = cls(data.ctypes.data_as(C.POINTER(C.c_float)), len(data), low, high,
                (F(high) - F(low)) / F(len(data) - 1), delta_recip(low, high, len(data)))
        s._keep = data
        return s


# ------------------------------------------------------------------------------------------- variants ----
class Variant:
    """One build of the albedo function with its scene and items.  uplift: "ours" | "jh" | "meng" | "rgb"; scene: a
    cs.CustomScene (quad_of: name -> quad) or the name of a built-in scene (texture: its image)."""

    def __init__(self, name, observer=1931, uplift="ours", jh_res=0):
        self.name, self.observer, self.uplift, self.jh_res = name, observer, uplift, jh_res
        self.texture, self.quad_of = None, {}
        self.textures = {}           # group -> image of the textured groups
        self.spectra = {}            # group -> (samples, low, high) of the groups with a constant albedo
        builtin = name.startswith("cornell") or uplift == "rgb"
        if uplift == "rgb":
            # custom scenes are spectral on the oracle's side: the lattice on plane-srgb's textured quad, the light box (albedo 0) next to it
            self.scene, self.texture = "plane-srgb", lattice_texture()
            self.lambda_min, self.lambda_step = 0.0, 1.0
        elif builtin:
            self.scene = "cornell"
        else:
            self.scene = self._texture_scene()
        if uplift != "rgb":
            self._host = self.scene._base if not builtin else Scene("cornell", observer=observer)   # (kept: its description is read below)
            d = self._host.desc.contents
            self.lambda_min, self.lambda_step = float(d.lambda_min), float(d.lambda_step)
        self.items = self._items().done()

    def _texture_scene(self):
        """the Cornell box (its light is the scene's light) plus, out of its way, one quad per texture and per short spectrum"""
        c = cs.CustomScene("cornell", observer=self.observer)

        def quad(material):
            z = -3000.0 - 10.0 * len(c.quads)
            return c.add_quad((0, 0, z), (1, 0, z), (1, 1, z), (0, 1, z), material)
        for name, tex in textures().items():
            c.textures.append(tex)
            self.quad_of[name] = quad(c.add_material(albedo_texture=len(c.textures) - 1))
            self.textures[name] = tex
        for name, (data, low, high) in SHORT.items():
            self.quad_of[name] = quad(c.add_material(albedo_spectrum=c.add_spectrum(data, low, high)))
            self.spectra[name] = (np.asarray(data, dtype=F), low, high)
        return c

    def _items(self):
        it = Items()
        lams = common_lambdas(self.lambda_min, self.lambda_step)
        if self.uplift == "rgb":
            # the RGB build has no wavelengths: lambda_0 = 0 (include/ssx.h); st: centres, and the edges of a 64-texel axis
            self.quad_of, self.textures = {"lattice": 0}, {"lattice": self.texture}
            it.add("lattice", 0, centres(64, 64), 0.0)
            a = axis_values(64)
            it.add("lattice", 0, np.stack([a, a[::-1]], axis=-1), 0.0)
            it.add("lattice", 0, np.stack([a, np.roll(a, 17)], axis=-1), 0.0)
            for q in range(1, 7):
                it.add("box", q, (0.5, 0.5), 0.0)
            return it
        if isinstance(self.scene, str):      # cornell: every quad's constant albedo
            d = self._host.desc.contents
            for q in range(d.n_quads):
                data, low, high = spectrum_of_quad(d, q)
                self.spectra["quad%d" % q] = (data, low, high)
                it.add("quad%d" % q, q, (0.25, 0.75), np.concatenate([lams, table_lambdas(low, high, len(data), self.lambda_step)]))
            return it
        extra = ()
        if self.uplift == "ours":            # the texel weights three table lookups on the basis spectra's grid
            low, high, n = self.basis_grid()
            extra = table_lambdas(low, high, n, self.lambda_step)
        texture_items(it, self.quad_of, lams, extra)       # Meng and Jakob-Hanika: the sampler's range only (Meng's sample index has no lower clamp)
        for name, (data, low, high) in self.spectra.items():
            it.add(name, self.quad_of[name], (0.5, 0.5), np.concatenate([lams, table_lambdas(low, high, len(data), self.lambda_step)]))
        return it

    def basis_grid(self):
        """(low, high, n) of the basis spectra (one grid for the three: one CSV file per observer)"""
        d = self._host.desc.contents
        g = {(float(s.low), float(s.high), int(s.n)) for s in (d.spectra[i] for i in (d.spec_basis_r, d.spec_basis_g, d.spec_basis_b))}
        assert len(g) == 1
        return g.pop()

    def uplift_scene(self):
        """the host library's Cornell scene built with this variant's uplift: it holds the fitted Jakob-Hanika model / the Meng grid"""
        if "_uplift_scene" not in self.__dict__:
            self._uplift_scene = None
            if self.uplift == "jh":
                self._uplift_scene = Scene("cornell", uplift="jh", jh_res=self.jh_res)
            elif self.uplift == "meng":
                from simple_spectral_amd import meng
                with tempfile.TemporaryDirectory() as tmp:
                    path = os.path.join(tmp, "grid.bin")
                    meng.save_table(path, ref_lib.meng_table())
                    self._uplift_scene = Scene("cornell", uplift="meng", meng_grid_path=path)
        return self._uplift_scene

    def oracle(self):
        if self.uplift == "rgb":
            return ol.Oracle(self.scene, texture=self.texture, rgb=True)
        if isinstance(self.scene, str):
            return ol.Oracle(self.scene, observer=self.observer)
        kw = {"jh": self.uplift_scene().jh_model()} if self.uplift == "jh" else {"meng": ref_lib.meng_table()} if self.uplift == "meng" else {}
        return self.scene.oracle(**kw)

    def desc(self, orc):
        """ssx_scene_desc of a custom-scene variant, with the uplift's tables"""
        d = self.scene.desc(orc)
        if self.uplift_scene() is not None:
            u = self.uplift_scene().desc.contents
            d.uplift, d.jh_res, d.jh_scale, d.jh_data, d.meng = u.uplift, u.jh_res, u.jh_scale, u.jh_data, u.meng
        return d


VARIANTS = {
    "ours-1931": dict(observer=1931), "ours-2006": dict(observer=2006),
    "jh-16": dict(uplift="jh", jh_res=16), "jh-7": dict(uplift="jh", jh_res=7),
    "meng": dict(uplift="meng"), "rgb": dict(uplift="rgb"),
    "cornell-1931": dict(observer=1931), "cornell-2006": dict(observer=2006),
}
_made = {}


def variant(name):
    """the variant of that name, made once (its items are shared by the tests and not to be changed)"""
    if name not in _made:
        _made[name] = Variant(name, **VARIANTS[name])
    return _made[name]
