"""Rows for one iteration of the path loop (include/ssx.h ssx_debug_step) and what the oracle says about them (oracle.h orc_debug_level): what
tests/test_step_cpu.py (the oracle alone) and tests/test_step_gpu.py (the kernels against it) share.  A row is one lane's path in front of the trace; the
expected answer is composed from ONE level of L() under three rules, the ones the comments of path_step state:

  1. the kernel continues iff L() would recurse and not (explicit light sampling and depth + 2 >= MAX_DEPTH); the draws are made either way;
  2. the kernel parks a next-event term iff the recorder has ORC_FOLD_NEE and the term is not four zeros (== 0.0f; a NaN is not zero); a parked term has the
     recorder's bits and is visible iff the shadow ray's primitive is the sampled light;
  3. the emission term has the recorder's flag and bits, except that a material whose emission table is all zeros has none (is_emissive == 0).

Everything else is the oracle's, bit for bit (NaN against NaN counts as equal).  Everything is seeded."""
import ctypes as C

import numpy as np

import crafted
import custom_scene as cs
import oracle_lib as ol
from simple_spectral_amd import _capi as K

MAX_DEPTH, NO_SLOT = 10, K.SSX_STEP_NO_SLOT
ROW, OUT = K.SSX_STEP_ROW_WORDS, K.SSX_STEP_OUT_WORDS
# orc_level_out as words (oracle.h)
(L_HIT_PRIM, L_HIT_DIST, L_HIT_ST, L_RECURSE, L_NEXT_ORIG, L_NEXT_DIR, L_LIGHT, L_LIGHT_NDL, L_LIGHT_PDF, L_SHADOW, L_SHADOW_DIR, L_SHADOW_HIT, L_INTERACTIONS,
 L_HIT_WHICH, L_LIGHT_WHICH, L_SHADOW_WHICH, L_LEVEL) = 0, 1, 2, 4, 5, 8, 11, 12, 13, 14, 15, 18, 19, 20, 21, 22, 23
LEVEL_WORDS = 38
# orc_fold_level within it
F_FS, F_NDL, F_PDF, F_FLAGS, F_EMISSION, F_NEE = (L_LEVEL + o for o in (0, 4, 5, 6, 7, 11))
FOLD_EMISSION, FOLD_NEE, FOLD_NEE_VISIBLE = 1, 2, 4
FLAG_SETS = (0, 1, 2, 3)   # orc_render_sample's word: 1 indirect-only | 2 without explicit light sampling


def f2u(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def u2f(x):
    return np.ascontiguousarray(x, dtype=np.uint32).view(np.float32)


def bind(lib):
    lib.orc_debug_level.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(ol.Rng), C.c_void_p, C.c_void_p, C.c_int, C.c_uint, C.c_float, C.c_int, C.c_void_p,
                                    C.POINTER(ol.Stats)]
    lib.orc_debug_level.restype = None
    lib.orc_debug_set_level_log.argtypes = [C.c_void_p]
    lib.orc_debug_set_level_log.restype = None
    lib.orc_fold_levels.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p]
    lib.orc_fold_levels.restype = None
    return lib


def make_rows(orig, direction, ignore, depth, lambda_0, rng, prev_slot):
    n = len(depth)
    r = np.zeros((n, ROW), dtype=np.uint32)
    r[:, K.SSX_STEP_R_ORIG:K.SSX_STEP_R_ORIG + 3] = f2u(orig).reshape(n, 3)
    r[:, K.SSX_STEP_R_DIR:K.SSX_STEP_R_DIR + 3] = f2u(direction).reshape(n, 3)
    r[:, K.SSX_STEP_R_IGNORE] = np.asarray(ignore, dtype=np.int64).astype(np.int32).view(np.uint32)
    r[:, K.SSX_STEP_R_DEPTH] = depth
    r[:, K.SSX_STEP_R_LAMBDA0] = f2u(lambda_0)
    r[:, K.SSX_STEP_R_RNG:K.SSX_STEP_R_RNG + 4] = rng
    r[:, K.SSX_STEP_R_PREV_SLOT] = prev_slot
    return r


def rng_words(state, inc):
    return [state & 0xFFFFFFFF, state >> 32, inc & 0xFFFFFFFF, inc >> 32]


def oracle_levels(orc, rows, flags, stats=None):
    """orc_debug_level per row -> (levels uint32 [n, LEVEL_WORDS], PCG32 state afterwards uint32 [n, 2])"""
    lib = bind(orc.lib)
    rows = np.ascontiguousarray(rows, dtype=np.uint32)
    lev, after = np.zeros((len(rows), LEVEL_WORDS), dtype=np.uint32), np.zeros((len(rows), 2), dtype=np.uint32)
    assert lev.strides[0] == 4 * LEVEL_WORDS
    rng = ol.Rng()
    fl = u2f(rows)
    for i, x in enumerate(rows):
        w = x[K.SSX_STEP_R_RNG:K.SSX_STEP_R_RNG + 4]
        rng.state, rng.inc = int(w[0]) | (int(w[1]) << 32), int(w[2]) | (int(w[3]) << 32)
        lib.orc_debug_level(orc.color, orc.scene, C.byref(rng), fl[i, 0:3].ctypes.data, fl[i, 3:6].ctypes.data, int(np.int32(x[K.SSX_STEP_R_IGNORE])),
                            int(x[K.SSX_STEP_R_DEPTH]), C.c_float(fl[i, K.SSX_STEP_R_LAMBDA0]), flags, lev[i].ctypes.data, stats)
        after[i] = (rng.state & 0xFFFFFFFF, rng.state >> 32)
    return lev, after


class Material:
    """what the rules and the counts need to know about the scene, from its public description (ssx_scene_desc): per quad is_emissive, whether the albedo is a
    texture, whether it is a mirror, whether its constant albedo table is all zeros (black), whether it is a PrimTri, and its triangles' normals"""

    def __init__(self, desc):
        d = desc
        self.n_quads = d.n_quads
        self.emissive, self.textured = np.zeros(d.n_quads, dtype=bool), np.zeros(d.n_quads, dtype=bool)
        self.mirror, self.black, self.is_tri = np.zeros(d.n_quads, dtype=bool), np.zeros(d.n_quads, dtype=bool), np.zeros(d.n_quads, dtype=bool)
        self.normal = np.zeros((d.n_quads, 2, 3), dtype=np.float64)
        for q in range(d.n_quads):
            m = d.materials[d.quads[q].material]
            sp = d.spectra[m.emission_spectrum]
            self.emissive[q] = any(d.samples[sp.offset + k] != 0.0 for k in range(sp.n))
            self.textured[q] = m.albedo_mode != 0
            self.mirror[q] = m.kind == 1
            al = d.spectra[m.albedo_spectrum]
            self.black[q] = m.kind == 0 and m.albedo_mode == 0 and not any(d.samples[al.offset + k] != 0.0 for k in range(al.n))
            self.is_tri[q] = (d.quads[q].flags & K.SSX_PRIM_TRI) != 0
            self.normal[q, 0], self.normal[q, 1] = d.quads[q].normal0[:], d.quads[q].normal1[:]


def decisions(rows, lev, flags):
    """the three rules' booleans per row, from the oracle's level alone: hit, continued, parked, visible, emission-flag-of-L()"""
    depth = rows[:, K.SSX_STEP_R_DEPTH].astype(np.int64)
    els = not (flags & 2)
    hit = lev[:, L_HIT_PRIM].view(np.int32) >= 0
    cont = (lev[:, L_RECURSE] != 0) & ~((depth + 2 >= MAX_DEPTH) if els else np.zeros(len(rows), dtype=bool))
    nee = u2f(lev[:, F_NEE:F_NEE + 4])
    parked = ((lev[:, F_FLAGS] & FOLD_NEE) != 0) & ~(nee == 0.0).all(axis=1)
    visible = parked & (lev[:, L_SHADOW_HIT] == lev[:, L_LIGHT])
    em = (lev[:, F_FLAGS] & FOLD_EMISSION) != 0
    return hit, cont, parked, visible, em


def expected(rows, lev, after, flags, mat, narrow):
    """-> (answer uint32 [n, OUT], compare bool [n, OUT]): the words ssx_debug_step must return and which of them are defined for the row"""
    n = len(rows)
    hit, cont, parked, visible, em_l = decisions(rows, lev, flags)
    prim = lev[:, L_HIT_PRIM].view(np.int32)
    em = em_l & hit & mat.emissive[np.where(hit, prim, 0)]
    e, m = np.zeros((n, OUT), dtype=np.uint32), np.ones((n, OUT), dtype=bool)
    m[:, K.SSX_STEP_O_SLOT:] = False
    e[:, K.SSX_STEP_O_FLAGS] = hit * K.SSX_STEP_HIT | cont * K.SSX_STEP_CONTINUED | em * K.SSX_STEP_EMISSION | parked * K.SSX_STEP_PARKED | visible * K.SSX_STEP_VISIBLE
    # the hit: 2 * primitive + the triangle of it that the intersection accepted
    e[:, K.SSX_STEP_O_HIT_TRI] = np.where(hit, 2 * prim + lev[:, L_HIT_WHICH].astype(np.int32), -1).astype(np.int32).view(np.uint32)
    e[:, K.SSX_STEP_O_HIT_DIST] = np.where(hit, lev[:, L_HIT_DIST], f2u([np.inf])[0])
    tex = hit & mat.textured[np.where(hit, prim, 0)]
    e[:, K.SSX_STEP_O_HIT_ST:K.SSX_STEP_O_HIT_ST + 2] = np.where(tex[:, None], lev[:, L_HIT_ST:L_HIT_ST + 2], 0)
    e[:, K.SSX_STEP_O_EMISSION:K.SSX_STEP_O_EMISSION + 4] = np.where(em[:, None], lev[:, F_EMISSION:F_EMISSION + 4], 0)
    term = lev[:, F_NEE:F_NEE + 4]
    e[:, K.SSX_STEP_O_NEE:K.SSX_STEP_O_NEE + 4] = np.where((parked if narrow else visible)[:, None], term, 0)
    e[:, K.SSX_STEP_O_NEE_TERM:K.SSX_STEP_O_NEE_TERM + 4] = np.where(visible[:, None], term, 0)
    e[:, K.SSX_STEP_O_FS:K.SSX_STEP_O_PDF + 1] = np.where(cont[:, None], lev[:, F_FS:F_PDF + 1], 0)
    e[:, K.SSX_STEP_O_PREV_SLOT] = rows[:, K.SSX_STEP_R_PREV_SLOT]
    e[:, K.SSX_STEP_O_TAIL_DEPTH] = np.where(cont, 0, rows[:, K.SSX_STEP_R_DEPTH])
    e[:, K.SSX_STEP_O_TAIL_HIT] = np.where(cont, 0, (hit | (rows[:, K.SSX_STEP_R_DEPTH] > 0)).astype(np.uint32))
    e[:, K.SSX_STEP_O_NEXT_ORIG:K.SSX_STEP_O_NEXT_ORIG + 3] = lev[:, L_NEXT_ORIG:L_NEXT_ORIG + 3]
    e[:, K.SSX_STEP_O_NEXT_DIR:K.SSX_STEP_O_NEXT_DIR + 3] = lev[:, L_NEXT_DIR:L_NEXT_DIR + 3]
    e[:, K.SSX_STEP_O_NEXT_IGNORE] = lev[:, L_HIT_PRIM]
    e[:, K.SSX_STEP_O_NEXT_DEPTH] = rows[:, K.SSX_STEP_R_DEPTH] + 1
    m[:, K.SSX_STEP_O_NEXT_ORIG:K.SSX_STEP_O_NEXT_DEPTH + 1] = cont[:, None]   # the next ray exists where the path continues
    e[:, K.SSX_STEP_O_RNG:K.SSX_STEP_O_RNG + 2] = after
    return e, m


def compare(got, exp, mask):
    """rows that differ, as (row, word) pairs"""
    g = np.array(got, dtype=np.uint32)
    same = (g == exp) | (np.isnan(g.view(np.float32)) & np.isnan(exp.view(np.float32)))
    same[:, K.SSX_STEP_O_FLAGS] = g[:, K.SSX_STEP_O_FLAGS] == exp[:, K.SSX_STEP_O_FLAGS]
    same[:, K.SSX_STEP_O_HIT_TRI] = g[:, K.SSX_STEP_O_HIT_TRI] == exp[:, K.SSX_STEP_O_HIT_TRI]
    return np.argwhere(~same & mask)


# ---- contexts ---------------------------------------------------------------------------------------------------------------------------------------------

def _black_cornell():
    """the Cornell box (topology 1: BLACK compiled out) with a black floor, black texels, a mirror block and a wall that both emits and reflects"""
    c = cs.CustomScene("cornell-srgb")
    zero = c.add_spectrum(np.zeros(8, dtype=np.float32), 400.0, 700.0)
    black = c.add_material(kind=0, albedo_spectrum=zero)
    pos, st, _ = c.quads[0]
    c.quads[0] = (pos, st, black)
    c.textures[0][::2, :, :] = 0
    white = c.materials[crafted.WHITE]["albedo_spectrum"]
    mirror = c.add_material(kind=1, albedo_spectrum=white)
    for q in (9, 10, 11):
        pos, st, _ = c.quads[q]
        c.quads[q] = (pos, st, mirror)
    glow = c.add_material(kind=0, albedo_spectrum=white, emission_spectrum=c.materials[crafted.LIGHT]["emission_spectrum"])
    pos, st, _ = c.quads[2]
    c.quads[2] = (pos, st, glow)
    return c


def _plane_inf():
    """plane-srgb (topology 2) with a +inf sample in its light's emission table: black_ends_path is cleared, the black walls are evaluated in full and park NaN"""
    c = cs.CustomScene("plane-srgb")
    li = next(m for pos, st, m in c.quads if c.spectra[c.materials[m]["emission_spectrum"]][0].any())
    data, low, high = c.spectra[c.materials[li]["emission_spectrum"]]
    data = data.copy(); data[len(data) // 2] = np.inf
    c.materials[li] = dict(c.materials[li], emission_spectrum=c.add_spectrum(data, low, high))
    return c


def _folded_light():
    """A light quad folded along its diagonal v00-v11, in a closed room (generic kernel): tri1 lies flat under the ceiling, tri0 hangs down from the diagonal to
    a corner two units below.  From the floor and the walls on the flap's side a direction sampled toward one triangle meets the other first: the shadow ray
    ends on the sampled QUAD's other triangle, and the light is visible all the same (shadow_flush compares quads)."""
    c = cs.CustomScene("cornell", keep_quads=False)
    crafted._room(c)
    c.add_quad((-1, 3.5, -1), (1, 1.5, -1), (1, 3.5, 1), (-1, 3.5, 1), crafted.LIGHT)
    c.set_camera((3.2, -3.0, -3.2), (0.0, -1.0, 0.0), up=(0, 1, 0), vfov_deg=70.0)
    return c


def _two_mirrors(c):
    white = c.materials[crafted.WHITE]["albedo_spectrum"]
    mirror = c.add_material(kind=1, albedo_spectrum=white)
    for q in (1, 3):
        pos, st, _ = c.quads[q]
        c.quads[q] = (pos, st, mirror)
    return c


# name: (scene maker or None for the built-in scene, base scene, observer, renderer options, topology the context must report, black_ends_path)
CONTEXTS = {
    "cornell-srgb": (None, "cornell-srgb", 1931, {}, 1, True),
    "cornell-2006": (None, "cornell", 2006, {}, 1, True),
    "cornell-black": (_black_cornell, "cornell-srgb", 1931, {}, 1, True),
    "cornell-rgb": (None, "cornell-srgb", 1931, dict(render_mode="rgb"), 1, True),
    "cornell-glibc": (None, "cornell-srgb", 1931, dict(libm="glibc-2.35"), 1, True),
    "plane-srgb": (None, "plane-srgb", 1931, {}, 2, True),
    "plane-inf": (_plane_inf, "plane-srgb", 1931, {}, 2, False),
    "degenerate": (lambda: _two_mirrors(crafted.degenerate_light_scene("room")), "cornell", 1931, {}, 0, True),   # two lights, one with a zero-area triangle; mirrors
    "folded-light": (_folded_light, "cornell", 1931, {}, 0, True),                                           # a shadow ray that meets the sampled quad's other triangle
    "prims128-2006": (lambda: crafted.many_prims_scene(128, 2006), "cornell", 2006, {}, 0, True),             # six lights, the last of them quad 127
}
_ctx = {}


class Context:
    def __init__(self, name):
        make, base, observer, opts, topo, black = CONTEXTS[name]
        self.name, self.base, self.observer, self.opts, self.topology, self.black_ends_path = name, base, observer, opts, topo, black
        self.rgb = opts.get("render_mode") == "rgb"
        self.glibc = opts.get("libm") == "glibc-2.35"
        self.scene = make() if make else None
        tex = None if base == "cornell" else "test-img.png"
        if self.scene is not None:
            self.oracle = self.scene.oracle()
            self.desc = self.scene.desc(self.oracle)
        else:
            if self.glibc:
                import glibc_oracle as go
                self.oracle = go.Oracle(base, observer=observer, texture=tex)
            else:
                self.oracle = ol.Oracle(base, observer=observer, texture=tex, rgb=self.rgb)
            from simple_spectral_amd.renderer import Scene
            self._scene = Scene(base, observer=observer, texture=tex, **({"render_mode": "rgb"} if self.rgb else {}))
            self.desc = self._scene.desc.contents
        self.mat = Material(self.desc)
        self.lambda_min, self.lambda_step = (0.0, 0.0) if self.rgb else (float(self.desc.lambda_min), float(self.desc.lambda_step))
        self._cases = None

    def renderer(self):
        from simple_spectral_amd import Options, Renderer
        r = Renderer(Options(scene_name=self.base, observer=self.observer, res=(8, 8), spp=1, texture=None if self.base == "cornell" else "test-img.png", **self.opts))
        if self.scene is not None:
            r.upload_scene_desc(self.desc)
        return r

    def cases(self):
        if self._cases is None:
            self._cases = build_cases(self)
        return self._cases


def context(name):
    if name not in _ctx:
        _ctx[name] = Context(name)
    return _ctx[name]


# ---- case families ----------------------------------------------------------------------------------------------------------------------------------------

W, H, SEED, SPP = 16, 16, 2026, 1
TILES = ((0, 0), (8, 0), (0, 8), (8, 8))
REPLAY_TILES = {0: 3, 1: 1, 2: 1, 3: 1}   # tiles of 64 paths per flag word: 384 paths per scene (paths without explicit light sampling run ten levels)
PREV_SLOTS = (0, NO_SLOT - 1, NO_SLOT, 77, 4095)


class Case:
    def __init__(self, name, flags, n_rounds, rows):
        rows = np.ascontiguousarray(rows, dtype=np.uint32)
        assert rows.shape[1] == ROW and len(rows) % (64 * n_rounds) == 0 and len(rows) // (64 * n_rounds) <= 64, (name, rows.shape, n_rounds)
        self.name, self.flags, self.n_rounds, self.rows = name, flags, n_rounds, rows
        self._ref = {}

    def reference(self, ctx, stats=None):
        """(levels, stream afterwards) of the oracle, computed once and left alone"""
        if "lev" not in self._ref or stats is not None:
            lev, after = oracle_levels(ctx.oracle, self.rows, self.flags, stats)
            if "lev" not in self._ref:
                self._ref["lev"] = (lev, after)
        return self._ref["lev"]


def fill(rows, n_rounds, g):
    """whole tiles: the rows, the places left over filled with repeats, shuffled over (tile, round, lane) so that the lanes of a wave diverge"""
    unit = 64 * n_rounds
    need = -(-len(rows) // unit) * unit
    idx = np.concatenate([np.arange(len(rows)), g.integers(0, len(rows), size=need - len(rows))])
    return rows[g.permutation(idx)]


def replay(ctx, flags, tiles=TILES):
    """The oracle's own paths, level by level: orc_render_sample with the recorder on, then the same sample as a chain of orc_debug_level from the camera ray.
    -> (rows, records): records = per sample (first row, recorded orc_fold_sample, final PCG32 state, xyza, chained levels, chained final state)"""
    import fold_cases as fc
    orc = ctx.oracle
    lib = bind(orc.lib)
    cam = np.ctypeslib.as_array(lib.orc_scene_cam_pos(orc.scene), shape=(3,)).astype(np.float32)
    rec = np.zeros(fc.ROW, dtype=np.uint32)
    rng, out = ol.Rng(), (C.c_float * 4)()
    rows, records = [], []
    lev1 = np.zeros((1, LEVEL_WORDS), dtype=np.uint32)
    for (i0, j0) in tiles:
        for p in range(64):
            i, j = i0 + (p & 7), j0 + (p >> 3)
            for k in range(SPP):
                lib.orc_seed_sample(SEED, j * W + i, k, C.byref(rng))
                lib.orc_debug_set_level_log(rec.ctypes.data)
                try:
                    lib.orc_render_sample(orc.color, orc.scene, C.byref(rng), i, j, W, H, flags, out, None)
                finally:
                    lib.orc_debug_set_level_log(None)
                final = (rng.state & 0xFFFFFFFF, rng.state >> 32)
                # the sample's draws in front of L(): the subpixel (two binary64 draws) and, in a spectral build, lambda_0
                lib.orc_seed_sample(SEED, j * W + i, k, C.byref(rng))
                lib.orc_rand_1d(C.byref(rng)); lib.orc_rand_1d(C.byref(rng))
                if not ctx.rgb:
                    lib.orc_rand_1f(C.byref(rng))
                lam = u2f(rec[fc.LAMBDA0:fc.LAMBDA0 + 1])[0]
                orig, d, ignore, depth, prev = cam.copy(), u2f(rec[fc.CAM_DIR:fc.CAM_DIR + 3]).copy(), -1, 0, NO_SLOT
                first, chain = len(rows), []
                while True:
                    row = make_rows(orig[None], d[None], [ignore], [depth], [lam], [rng_words(rng.state, rng.inc)], [prev])[0]
                    rows.append(row)
                    lib.orc_debug_level(orc.color, orc.scene, C.byref(rng), orig.ctypes.data, d.ctypes.data, ignore, depth, C.c_float(lam), flags, lev1.ctypes.data, None)
                    chain.append(lev1[0].copy())
                    if not lev1[0, L_RECURSE]:
                        break
                    orig, d = u2f(lev1[0, L_NEXT_ORIG:L_NEXT_ORIG + 3]).copy(), u2f(lev1[0, L_NEXT_DIR:L_NEXT_DIR + 3]).copy()
                    ignore, depth = int(lev1[0, L_HIT_PRIM].view(np.int32)), depth + 1
                    prev = PREV_SLOTS[(len(rows) + depth) % len(PREV_SLOTS)]
                records.append((first, rec.copy(), final, f2u(out[:]).copy(), np.stack(chain), (rng.state & 0xFFFFFFFF, rng.state >> 32)))
    return np.stack(rows), records


def aimed(ctx, g, per_side=2, depths=(0, 1, 5, 8, 9)):
    """rays aimed at an inner point of every primitive, from its front and from behind, at several depths: every material and every light from both sides"""
    d = ctx.desc
    rows = []
    for q in range(d.n_quads):
        Q = d.quads[q]
        P = np.array([Q.v00.pos[:], Q.v10.pos[:], Q.v11.pos[:]], dtype=np.float64)
        nrm = np.array(Q.normal0[:], dtype=np.float64)
        if not np.isfinite(nrm).all() or not np.linalg.norm(nrm) > 0:
            continue
        for side in (1.0, -1.0):
            for _ in range(per_side):
                b = g.dirichlet((2.0, 2.0, 2.0))
                target = b @ P
                size = max(np.linalg.norm(P[1] - P[0]), 1e-3)
                o = target + side * nrm * size * g.uniform(0.3, 1.5) + g.normal(size=3) * 0.1 * size
                v = target - o; v /= np.linalg.norm(v)
                depth = int(depths[len(rows) % len(depths)])
                lam = ctx.lambda_min + g.uniform() * ctx.lambda_step
                rows.append(make_rows(o[None], v[None], [-1], [depth], [lam], [rng_words(int(g.integers(0, 2**63)), int(g.integers(0, 2**63)) | 1)],
                                      [NO_SLOT if depth == 0 else PREV_SLOTS[len(rows) % len(PREV_SLOTS)]])[0])
    return np.stack(rows)


def misses(ctx, g, n=32):
    """rays that leave the scene, at depth 0 and deeper: from far outside the scene's bounds, pointing away from it"""
    d = ctx.desc
    pts = np.array([v.pos[:] for q in range(d.n_quads) for v in (d.quads[q].v00, d.quads[q].v10, d.quads[q].v11, d.quads[q].v01)], dtype=np.float64)
    ctr, rad = pts.mean(axis=0), np.abs(pts - pts.mean(axis=0)).max() * 4.0 + 1.0
    rows = []
    for i in range(n):
        v = g.normal(size=3); v /= np.linalg.norm(v)
        depth = (0, 0, 1, 4, 9)[i % 5]
        rows.append(make_rows((ctr + v * rad)[None], v[None], [-1 if depth == 0 else i % d.n_quads], [depth], [ctx.lambda_min + g.uniform() * ctx.lambda_step],
                              [rng_words(int(g.integers(0, 2**63)), int(g.integers(0, 2**63)) | 1)], [NO_SLOT if depth == 0 else PREV_SLOTS[i % len(PREV_SLOTS)]])[0])
    return np.stack(rows)


def depth_ladder(base_rows, g, n_base=16):
    """the same rays -- the same hits -- at every depth 0..9"""
    pick = base_rows[g.choice(len(base_rows), size=min(n_base, len(base_rows)), replace=False)]
    out = []
    for depth in range(MAX_DEPTH):
        r = pick.copy()
        r[:, K.SSX_STEP_R_DEPTH] = depth
        r[:, K.SSX_STEP_R_PREV_SLOT] = NO_SLOT if depth == 0 else PREV_SLOTS[depth % len(PREV_SLOTS)]
        out.append(r)
    return np.concatenate(out)


# lanes of a round that park, per round; the running count of the queue passes through 63 -> 64 (a flush that leaves nothing), 64 + r (a flush that leaves a
# remainder below the rays it took from the top), 127, and the last round parks nothing (the drain alone empties the queue)
QUEUE_SEQUENCES = {"each-count": (0, 1, 31, 33, 64), "boundaries": (63, 1, 40, 40, 47, 64, 0), "drain-only": (17, 0)}


def queue_events(park_counts):
    """what a sequence of per-round park counts does to the queue, by the loop of flush_parked: the events it passes through"""
    count, ev = 0, set()
    for i, n in enumerate(park_counts):
        assert 0 <= n <= 64
        before = count
        count += n
        if before == 63 and count == 64:
            ev.add("63->64")
        if count == 127:
            ev.add("127")
        last = i + 1 == len(park_counts)
        while count >= 64 or (last and count):
            take = min(count, 64)
            count -= take
            if take == 64 and count:
                ev.add("remainder")
            if last and n == 0:
                ev.add("drain-alone")
            if take < 64:
                ev.add("partial")
    assert count == 0
    return ev


def queue_case(name, seq, parking, quiet, g):
    """one tile whose round k has seq[k] parking lanes, scattered over the wave, not a prefix"""
    rows = np.zeros((len(seq) * 64, ROW), dtype=np.uint32)
    for k, n in enumerate(seq):
        lanes = g.permutation(64)
        while 0 < n < 64 and lanes[:n].max() == n - 1:   # scattered: never the first n lanes of the wave
            lanes = g.permutation(64)
        rows[k * 64 + lanes[:n]] = parking[g.integers(0, len(parking), size=n)]
        rows[k * 64 + lanes[n:]] = quiet[g.integers(0, len(quiet), size=64 - n)]
    return rows


def build_cases(ctx):
    g = np.random.default_rng(2600 + sum(map(ord, ctx.name)))
    cases, ctx.replays = [], {}
    for flags in FLAG_SETS:
        n_tiles = REPLAY_TILES[flags] if ctx.desc.n_quads <= 40 else max(1, REPLAY_TILES[flags] // 2)
        rows, records = replay(ctx, flags, tiles=TILES[:n_tiles])
        ctx.replays[flags] = (rows, records)
        cases.append(Case("replay/flags%d" % flags, flags, 2, fill(rows, 2, g)))
    per_side = 2 if ctx.desc.n_quads <= 40 else 1
    base = np.concatenate([ctx.replays[0][0], aimed(ctx, g, per_side)])
    lev, _ = oracle_levels(ctx.oracle, base, 0)
    prim = lev[:, L_HIT_PRIM].view(np.int32)
    on_light = np.flatnonzero((prim >= 0) & ctx.mat.emissive[np.where(prim >= 0, prim, 0)])[:4]   # the ladder has rays that meet a light: its emission at every depth
    lad = np.concatenate([depth_ladder(base, g), depth_ladder(base[on_light], g)]) if len(on_light) else depth_ladder(base, g)
    for flags in FLAG_SETS:
        cases.append(Case("depth-ladder/flags%d" % flags, flags, 3, fill(lad, 3, g)))
    am = np.concatenate([aimed(ctx, g, per_side), misses(ctx, g)])
    for flags in (0, 2):
        cases.append(Case("aimed-and-misses/flags%d" % flags, flags, 1, fill(am, 1, g)))
    # queue shapes, from the oracle's park decisions (rule 2) on the rows at hand
    for flags in (0, 1):
        parked = decisions(base, lev if flags == 0 else oracle_levels(ctx.oracle, base, flags)[0], flags)[2]
        assert parked.any() and (~parked).any(), (ctx.name, flags)   # a context without both kinds of row has no queue cases: an error, not a smaller suite
        for name, seq in QUEUE_SEQUENCES.items():
            if flags == 0 or name == "boundaries":
                cases.append(Case("queue/%s/flags%d" % (name, flags), flags, len(seq), queue_case(name, seq, base[parked], base[~parked], g)))
    return cases


def reach(ctx):
    """what the context's rows reach, counted from the oracle's outputs and orc_stats (tests/test_step_cpu.py asserts per context what applies to it)"""
    c = dict(rows=0, hit=0, miss_depth0=0, miss_deeper=0, continued=0, recurse_but_stopped=0, depth9_no_draws=0, emission=0, emission_flag_not_emissive=0,
             emission_deeper=0, emission_suppressed_indirect_only=0, parked=0, parked_nan=0, zero_term_not_parked=0, visible=0, occluded=0, occluded_by_other_light=0,
             faces_away=0, pdf_inf=0, light_pdf_inf=0, mirror=0, textured=0, black=0, light_hit=0, emissive_and_continues=0, quad127_light=0, quad127_hit=0,
             light_front=0, light_back=0, mirror_front=0, mirror_back=0, other_triangle_visible=0, same_triangle_visible=0, hit_tri1=0,
             prev_slots=set(), depths=set(), lemire_redraws=0, coshemi_retries=0)
    for case in ctx.cases():
        st = ol.Stats()
        lev, _ = case.reference(ctx, C.byref(st))
        rows, flags = case.rows, case.flags
        hit, cont, parked, visible, em_l = decisions(rows, lev, flags)
        depth = rows[:, K.SSX_STEP_R_DEPTH].astype(np.int64)
        prim = np.where(hit, lev[:, L_HIT_PRIM].view(np.int32), 0)
        em = em_l & hit & ctx.mat.emissive[prim]
        nee_flag = (lev[:, F_FLAGS] & FOLD_NEE) != 0
        term = u2f(lev[:, F_NEE:F_NEE + 4])
        fs = u2f(lev[:, F_FS:F_FS + 4])
        sampled = lev[:, L_LIGHT].view(np.int32) >= 0
        els = not (flags & 2)
        c["rows"] += len(rows); c["hit"] += int(hit.sum())
        c["miss_depth0"] += int((~hit & (depth == 0)).sum()); c["miss_deeper"] += int((~hit & (depth > 0)).sum())
        c["continued"] += int(cont.sum()); c["recurse_but_stopped"] += int(((lev[:, L_RECURSE] != 0) & ~cont).sum())
        c["depth9_no_draws"] += int((hit & (depth == MAX_DEPTH - 1)).sum())
        c["emission"] += int(em.sum()); c["emission_flag_not_emissive"] += int((em_l & hit & ~ctx.mat.emissive[prim]).sum())
        c["emission_deeper"] += int((em & (depth > 0)).sum())
        c["emission_suppressed_indirect_only"] += int((hit & ctx.mat.emissive[prim] & (depth == 0) & ~em_l).sum()) if (flags & 1) and els else 0
        c["parked"] += int(parked.sum()); c["parked_nan"] += int((parked & np.isnan(term).any(axis=1)).sum())
        c["zero_term_not_parked"] += int((nee_flag & ~parked).sum())
        c["visible"] += int(visible.sum()); c["occluded"] += int((parked & ~visible).sum())
        other = parked & ~visible & (lev[:, L_SHADOW_HIT].view(np.int32) >= 0)
        c["occluded_by_other_light"] += int((other & ctx.mat.emissive[np.where(other, lev[:, L_SHADOW_HIT].view(np.int32), 0)]).sum())
        c["faces_away"] += int((sampled & ~(u2f(lev[:, L_LIGHT_NDL]) > 0)).sum())
        c["light_pdf_inf"] += int((sampled & np.isinf(u2f(lev[:, L_LIGHT_PDF]))).sum())
        shaded = hit & (lev[:, L_INTERACTIONS] != 0)
        mirror = shaded & ctx.mat.mirror[prim]
        # the side the ray meets: against the accepted triangle's normal is its front
        which = np.where(hit, lev[:, L_HIT_WHICH], 0).astype(np.int64)
        front = (u2f(rows[:, K.SSX_STEP_R_DIR:K.SSX_STEP_R_DIR + 3]).astype(np.float64) * ctx.mat.normal[prim, which]).sum(axis=1) < 0
        c["mirror"] += int(mirror.sum()); c["mirror_front"] += int((mirror & front).sum()); c["mirror_back"] += int((mirror & ~front).sum())
        # a delta BSDF's +inf pdf, logged as n_dot_l = pdf = 1 where the path continues
        c["pdf_inf"] += int((mirror & cont & (u2f(lev[:, F_PDF]) == 1.0) & (u2f(lev[:, F_NDL]) == 1.0)).sum())
        c["textured"] += int((hit & ctx.mat.textured[prim]).sum())
        c["black"] += int((shaded & ctx.mat.black[prim]).sum())
        c["light_front"] += int((hit & ctx.mat.emissive[prim] & front).sum()); c["light_back"] += int((hit & ctx.mat.emissive[prim] & ~front).sum())
        c["hit_tri1"] += int((hit & (which == 1)).sum())
        li = np.where(sampled, lev[:, L_LIGHT].view(np.int32), 0)
        on_quad = visible & ~ctx.mat.is_tri[li]
        c["other_triangle_visible"] += int((on_quad & (lev[:, L_LIGHT_WHICH] != lev[:, L_SHADOW_WHICH])).sum())
        c["same_triangle_visible"] += int((on_quad & (lev[:, L_LIGHT_WHICH] == lev[:, L_SHADOW_WHICH])).sum())
        c["light_hit"] += int((hit & ctx.mat.emissive[prim]).sum()); c["emissive_and_continues"] += int((hit & ctx.mat.emissive[prim] & cont).sum())
        # SSX_MAX_QUADS - 1 in either field of a parked ray's tag word, light << 8 | hit quad
        c["quad127_light"] += int((parked & (lev[:, L_LIGHT] == 127)).sum()); c["quad127_hit"] += int((parked & (prim == 127)).sum())
        c["prev_slots"] |= set(np.unique(rows[:, K.SSX_STEP_R_PREV_SLOT]).tolist()); c["depths"] |= set(np.unique(depth).tolist())
        c["lemire_redraws"] += st.lemire_redraws; c["coshemi_retries"] += st.coshemi_retries
    return c
